"""What the tests of the 16-bit token attention share (test_token_attention_16bit_cpu.py, test_gpu_token_attention_16bit.py):
the bound, derived from the kernel's arithmetic contract, and a tile-by-tile restatement of that contract in torch that
takes one named fault at a time.

The contract (include/waldo_hip.h "Token attention on 16-bit operands"): a score is an fp32 sum of exact 16-bit products;
scale, mask, running maximum and the running sum l are fp32, l sums the UNROUNDED p; p is rounded to the operand type
only as the operand of the second product; o is accumulated and rescaled in fp32; one rounding at the store.

The bound.  exact = ``token_attention_framework`` in fp64 on the 16-bit operands widened, A = the same with |v| in place
of v.  Rounding p_j to p_j (1 + e_j), |e_j| <= u, moves out by sum_j e_j p_j v_j / l, at most u A; the store's rounding
moves it by at most u |out|; everything else is fp32, for which the project's TOL stands, on the scale of the sum's
terms:

    |out - exact| <= u (A + |exact|) + TOL max(1, A)        u = 2^-8 (bf16), 2^-11 (fp16): the unit roundoff

A NaN anywhere -- in out, in exact -- fails the element."""
import torch

from parity import TOL

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTYPES = (torch.bfloat16, torch.float16)


def exact_and_abs(fw, q, k, v, k2=None, v2=None, scale=None):
    """(exact, A) in fp64 from the 16-bit operands widened; ``fw`` is ``token_attention_framework``."""
    w = lambda t: None if t is None else t.detach().double()
    exact = fw(w(q), w(k), w(v), w(k2), w(v2), scale=scale)
    a = fw(w(q), w(k), w(v).abs(), w(k2), None if v2 is None else w(v2).abs(), scale=scale)
    return exact, a


def bound_ratio(out, exact, a):
    """The worst |out - exact| / bound over the elements (inf where a NaN is involved) and the index of that element."""
    u = U[out.dtype]
    bound = u * (a + exact.abs()) + TOL * a.clamp_min(1.0)
    ratio = (out.detach().double() - exact).abs() / bound
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    worst = int(ratio.argmax())
    return ratio.reshape(-1)[worst].item(), tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), ratio.shape))


def within_bound(fw, out, ops, scale=None, what=""):
    """Assert the bound for ``out`` = the candidate's result on the 16-bit operands ``ops``; returns the worst ratio."""
    exact, a = exact_and_abs(fw, *ops, scale=scale)
    assert out.shape == exact.shape and out.dtype == ops[0].dtype and out.is_contiguous(), what
    worst, at = bound_ratio(out, exact.to(out.device), a.to(out.device))
    print(f"[bound16] {what} {str(out.dtype)[6:]}: worst {worst:.3g} x its bound at {at}")
    assert worst <= 1.0, f"{what}: {worst:.3g} x the bound at {at}"
    return worst


def to16(ops, dtype):
    return tuple(None if t is None else t.to(dtype) for t in ops)


# ---------------------------------------------------------------------------------------------------------------------
# the contract restated, with planted faults
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("last_key_of_a_full_tile_dropped", "no_rescale", "seam_key_from_the_first_segment", "scale_twice",
          "l_from_rounded_p")


def attention16(fault=None, kt=64):
    """fn(q, k, v, k2=None, v2=None, scale=None) on 16-bit (B, N, H, D) operands -> (B, Nq, H D) of their type: the
    contract tile by tile (``kt`` keys), every fp32 step in fp32.  ``fault``: one of FAULTS, or None."""
    assert fault is None or fault in FAULTS, fault

    def fn(q, k, v, k2=None, v2=None, scale=None):
        dtype = q.dtype
        b, nq, h, d = q.shape
        scale = d ** -0.5 if scale is None else scale
        scale = torch.tensor(scale, dtype=torch.float32)
        if k2 is not None:
            if fault == "seam_key_from_the_first_segment":
                k2, v2 = k2.clone(), v2.clone()
                k2[:, 0], v2[:, 0] = k[:, 0], v[:, 0]
            k, v = torch.cat([k, k2], 1), torch.cat([v, v2], 1)
        qh, kh, vh = (t.float().permute(0, 2, 1, 3) for t in (q, k, v))      # (B, H, N, D), widened exactly
        nk = kh.shape[2]
        o = torch.zeros(b, h, nq, d)
        m = torch.full((b, h, nq, 1), float("-inf"))
        l = torch.zeros(b, h, nq, 1)
        for t0 in range(0, nk, kt):
            kt_, vt = kh[:, :, t0:t0 + kt], vh[:, :, t0:t0 + kt]
            s = (qh @ kt_.transpose(2, 3)) * scale
            if fault == "scale_twice":
                s = s * scale
            if fault == "last_key_of_a_full_tile_dropped" and kt_.shape[2] == kt:
                s[..., kt - 1] = float("-inf")
            mnew = torch.maximum(m, s.amax(-1, keepdim=True))
            alpha = torch.exp(m - mnew)
            if fault == "no_rescale":
                alpha = torch.ones_like(alpha)
            p = torch.exp(s - mnew)
            p16 = p.to(dtype).float()
            l = l * alpha + (p16 if fault == "l_from_rounded_p" else p).sum(-1, keepdim=True)
            o = o * alpha + p16 @ vt
            m = mnew
        return (o / l).to(dtype).transpose(1, 2).reshape(b, nq, h * d)

    return fn
