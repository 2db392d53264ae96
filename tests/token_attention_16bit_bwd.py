"""What the tests of the 16-bit token attention's backward share (test_token_attention_16bit_bwd_cpu.py,
test_gpu_token_attention_16bit_bwd.py): the bound, derived from the kernels' arithmetic contract, a tile-by-tile
restatement of that contract in torch that takes one named fault at a time, and the operand lists as plain data.

The contract (include/waldo_hip.h "Token attention on 16-bit operands"): a recomputed score and dP = dO V^T are fp32 sums
of exact 16-bit products; P = exp(scale S - lse) is fp32, lse = m + log(l) the forward's fp32 row statistic; delta =
sum_d dO O is an fp32 fma chain over the 16-bit grad_out and the STORED 16-bit out; dS = P o (dP - delta) is fp32; dS and
P are rounded to the element type only as operands of dQ / dK and of dV; the three gradients are accumulated in fp32;
scale multiplies the fp32 accumulators of dQ and dK once, after the sum; one rounding at the store.

The bound.  In fp64 on the widened operands and the widened grad_out, per (b, h): P, O, dP, delta, dS exact, A = P |V|,
u = 2^-8 (bf16), 2^-11 (fp16), TOL the project's fp32 tolerance.

    E_i  = sum_d |dO_id| (u (A_id + |O_id|) + TOL max(1, A_id))      the forward's bound on the stored out, in delta
    W_ij = P_ij E_i + u |dS_ij|                                       what the dS operand can be off by
    |dQ - exact| <= |scale| (W |K|)   + u |dQ| + TOL max(1, |scale| |dS| |K|)
    |dK - exact| <= |scale| (W^T |Q|) + u |dK| + TOL max(1, |scale| |dS|^T |Q|)
    |dV - exact| <= u P^T |dO|        + u |dV| + TOL max(1, P^T |dO|)

A NaN on either side fails the element.  The bound's resolution is u: a 1 % bias of dQ is inside it in bf16 (u is 0.4 %)
and outside it in fp16.

``delta`` from the UNROUNDED forward output (o / l in fp32 instead of the stored 16-bit out) is NOT among the faults: it
moves delta by at most sum_d |dO| u |O|, which is inside E by construction -- the bound cannot tell the two apart, and
test_token_attention_16bit_bwd_cpu.py shows that it does not."""
import torch

import test_gpu_token_attention as FWD
from parity import TOL
from token_attention_16bit import DTYPES, U, attention16, to16   # noqa: F401  (DTYPES, to16: for the two test files)

QT = KT = 64   # the kernels' tiles; the GPU tests check the library's against them
NAMES = ("dq", "dk", "dv", "dk2", "dv2")


# ---------------------------------------------------------------------------------------------------------------------
# operand lists: plain data, one list for the GPU file and for the CPU replay
# ---------------------------------------------------------------------------------------------------------------------
def tile_edge_cases(d):
    """(b, h, nq, nk1, nk2, d, seed): every combination of Nq in {1, 63, 64, 65, 130}, Nk1 in {1, 63, 64, 65, 131} and
    Nk2 in {absent, 1, 37, 65} -- the seam inside a tile, on a tile boundary and in the last tile -- with B = 1 and 2
    in turn and H = 2."""
    grid = [(nq, nk1, nk2) for nq in (1, QT - 1, QT, QT + 1, 2 * QT + 2) for nk1 in (1, KT - 1, KT, KT + 1, 2 * KT + 3)
            for nk2 in (None, 1, 37, KT + 1)]
    return [(1 + i % 2, 2, nq, nk1, nk2, d, i + 1) for i, (nq, nk1, nk2) in enumerate(grid)]


def scale_cases():
    """((b, h, nq, nk1, nk2, d, seed), scale): the forward file's, its four SCALE_FACTORS at each D."""
    return FWD.scale_cases(QT, KT)


LARGE_SCORE_CASES = FWD.LARGE_SCORE_CASES


def grad_out_for(ops, seed=0):
    """A seeded fp32 (B, Nq, H D) gradient of out on the CPU (the caller rounds and moves it)."""
    b, nq, h, d = ops[0].shape
    return torch.randn(b, nq, h * d, generator=torch.Generator().manual_seed(1000 + seed))


def family(name, dev, dtype, dims=(16, 32, 64)):
    """[(ops, grad_out, scale, what)] of a family on ``dev``, rounded to ``dtype``."""
    out = []
    if name == "tile":
        for d in dims:
            for c in tile_edge_cases(d):
                ops = to16(FWD.operands(dev, *c[:6], seed=c[6]), dtype)
                out.append((ops, grad_out_for(ops, c[6]).to(dev, dtype), None, f"tile {c}"))
    elif name == "scale":
        for c, s in scale_cases():
            if c[5] in dims:
                ops = to16(FWD.operands(dev, *c[:6], seed=c[6]), dtype)
                out.append((ops, grad_out_for(ops, c[6]).to(dev, dtype), s, f"scale {c} {s:.3g}"))
    else:
        assert name == "large", name
        for low in LARGE_SCORE_CASES:
            ops = to16(FWD.large_score_operands(dev, KT, low), dtype)
            out.append((ops, grad_out_for(ops, 7).to(dev, dtype), None, f"large scores, low rows {low}"))
    return out


FAMILIES = ("tile", "scale", "large")


# ---------------------------------------------------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------------------------------------------------
def exact_and_bounds(ops, go, scale=None):
    """({name: exact}, {name: bound}) in fp64, in the operands' (B, N, H, D) layout, on their device; dk2 / dv2 are
    absent without a second segment."""
    q, k, v, k2, v2 = ops
    u = U[q.dtype]
    b, nq, h, d = q.shape
    scale = d ** -0.5 if scale is None else float(scale)
    w = lambda t: t.detach().double().permute(0, 2, 1, 3)   # (B, H, N, D)
    nk1 = k.shape[1]
    qh = w(q)
    kh = w(k) if k2 is None else torch.cat([w(k), w(k2)], 2)
    vh = w(v) if v2 is None else torch.cat([w(v), w(v2)], 2)
    do = w(go.view(b, nq, h, d))
    p = torch.softmax(scale * (qh @ kh.transpose(2, 3)), -1)
    o, a = p @ vh, p @ vh.abs()
    dp = do @ vh.transpose(2, 3)
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    dq, dk, dv = scale * (ds @ kh), scale * (ds.transpose(2, 3) @ qh), p.transpose(2, 3) @ do
    e = (do.abs() * (u * (a + o.abs()) + TOL * a.clamp_min(1.0))).sum(-1, keepdim=True)
    wds = p * e + u * ds.abs()
    s = abs(scale)
    bq = s * (wds @ kh.abs()) + u * dq.abs() + TOL * (s * (ds.abs() @ kh.abs())).clamp_min(1.0)
    bk = s * (wds.transpose(2, 3) @ qh.abs()) + u * dk.abs() + TOL * (s * (ds.abs().transpose(2, 3) @ qh.abs())).clamp_min(1.0)
    pdo = p.transpose(2, 3) @ do.abs()
    bv = u * pdo + u * dv.abs() + TOL * pdo.clamp_min(1.0)
    back = lambda t: t.permute(0, 2, 1, 3).contiguous()
    exact = {"dq": back(dq), "dk": back(dk[:, :, :nk1]), "dv": back(dv[:, :, :nk1])}
    bound = {"dq": back(bq), "dk": back(bk[:, :, :nk1]), "dv": back(bv[:, :, :nk1])}
    if k2 is not None:
        exact.update(dk2=back(dk[:, :, nk1:]), dv2=back(dv[:, :, nk1:]))
        bound.update(dk2=back(bk[:, :, nk1:]), dv2=back(bv[:, :, nk1:]))
    return exact, bound


def bound_ratios(grads, exact, bound):
    """{name: the worst |grad - exact| / bound over the elements}, inf where a NaN is involved; ``grads`` is the
    candidate's five gradients in NAMES' order (None for an absent segment)."""
    out = {}
    for name, g in zip(NAMES, grads):
        if name not in exact:
            assert g is None, name
            continue
        assert g is not None and g.shape == exact[name].shape, (name, None if g is None else g.shape)
        ratio = (g.detach().double().to(exact[name].device) - exact[name]).abs() / bound[name]
        ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
        out[name] = ratio.max().item()
    return out


def within_bound(grads, ops, go, scale=None, what="", ref=None):
    """Assert the bound for the candidate's five gradients; returns the ratios.  ``ref``: (exact, bound) computed
    before."""
    exact, bound = ref or exact_and_bounds(ops, go, scale)
    for name, g in zip(NAMES, grads):
        if g is not None:
            assert g.dtype == ops[0].dtype and g.is_contiguous(), (what, name)
    ratios = bound_ratios(grads, exact, bound)
    print(f"[bound16-bwd] {what} {str(ops[0].dtype)[6:]}: " + "  ".join(f"{k} {r:.3g}" for k, r in ratios.items()))
    bad = {k: r for k, r in ratios.items() if not r <= 1.0}
    assert not bad, f"{what}: beyond the bound: {bad}"
    return ratios


# ---------------------------------------------------------------------------------------------------------------------
# the contract restated, with planted faults
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("dk_ignores_the_scale", "delta_left_out", "lse_without_the_log", "seam_key_written_to_the_first_segment",
          "second_segment_dropped", "last_query_of_a_full_tile_dropped", "live_rows_past_nq", "dq_scaled_twice")
# not a fault the bound can see (the module's docstring); the CPU file shows that it passes
INDISTINGUISHABLE = ("delta_from_the_unrounded_out",)


def _forward_stats(qh, kh, scale, kt):
    """(m, l) of the forward's online softmax, tile by tile in fp32, and with them lse = m + log(l)."""
    m = torch.full(qh.shape[:3] + (1,), float("-inf"))
    l = torch.zeros_like(m)
    for t0 in range(0, kh.shape[2], kt):
        s = (qh @ kh[:, :, t0:t0 + kt].transpose(2, 3)) * scale
        mnew = torch.maximum(m, s.amax(-1, keepdim=True))
        l = l * torch.exp(m - mnew) + torch.exp(s - mnew).sum(-1, keepdim=True)
        m = mnew
    return m, l


def attention16_bwd(fault=None, qt=QT, kt=KT):
    """fn(q, k, v, k2, v2, grad_out, scale=None) on 16-bit CPU operands -> (dq, dk, dv, dk2, dv2) of their type (None
    for an absent segment): the two matrix kernels tile by tile (``qt`` queries, ``kt`` keys), every fp32 step in fp32,
    from the stored out of ``attention16()``.  ``fault``: one of FAULTS or INDISTINGUISHABLE, or None."""
    assert fault is None or fault in FAULTS + INDISTINGUISHABLE, fault

    def fn(q, k, v, k2=None, v2=None, grad_out=None, scale=None):
        dtype = q.dtype
        r16 = lambda t: t.to(dtype).float()
        b, nq, h, d = q.shape
        nk1 = k.shape[1]
        scale = torch.tensor(d ** -0.5 if scale is None else scale, dtype=torch.float32)
        out16 = attention16(None, kt)(q, k, v, k2, v2, scale=float(scale))                 # the STORED out
        w = lambda t: t.float().permute(0, 2, 1, 3)
        qh = w(q)
        kh = w(k) if k2 is None else torch.cat([w(k), w(k2)], 2)
        vh = w(v) if v2 is None else torch.cat([w(v), w(v2)], 2)
        nk = kh.shape[2]
        do, oh = w(grad_out.view(b, nq, h, d)), w(out16.view(b, nq, h, d))
        m, l = _forward_stats(qh, kh, scale, kt)
        lse = m + (l if fault == "lse_without_the_log" else torch.log(l))
        if fault == "delta_from_the_unrounded_out":
            oh = torch.softmax((qh.double() @ kh.double().transpose(2, 3)) * scale.double(), -1).float() @ vh
        delta = torch.zeros(b, h, nq, 1)
        for c in range(d):                                                                  # one fp32 chain over d
            delta = torch.addcmul(delta, do[..., c:c + 1], oh[..., c:c + 1])
        if fault == "delta_left_out":
            delta = torch.zeros_like(delta)

        # the dQ kernel: a lane owns a query row, the key tiles go by
        dq = torch.zeros(b, h, nq, d)
        for t0 in range(0, nk, kt):
            kt_, vt = kh[:, :, t0:t0 + kt], vh[:, :, t0:t0 + kt]
            p = torch.exp((qh @ kt_.transpose(2, 3)) * scale - lse)
            ds = p * (do @ vt.transpose(2, 3) - delta)
            dq = dq + r16(ds) @ kt_
        dq = dq * scale
        if fault == "dq_scaled_twice":
            dq = dq * scale

        # the dK/dV kernel: a lane owns a key, the query tiles go by
        dk, dv = torch.zeros(b, h, nk, d), torch.zeros(b, h, nk, d)
        for t0 in range(0, nq, qt):
            qt_, dot, lt, dt = qh[:, :, t0:t0 + qt], do[:, :, t0:t0 + qt], lse[:, :, t0:t0 + qt], delta[:, :, t0:t0 + qt]
            rows = qt_.shape[2]
            if fault == "live_rows_past_nq" and rows < qt:
                # the rows past Nq are staged as zeros, but their P is exp of an lse that was never written
                pad = lambda t, x: torch.cat([t, torch.full((b, h, qt - rows, t.shape[3]), x)], 2)
                qt_, dot, lt, dt = pad(qt_, 0.0), pad(dot, 0.0), pad(lt, float("nan")), pad(dt, 0.0)
            p = torch.exp((qt_ @ kh.transpose(2, 3)) * scale - lt)
            if fault == "last_query_of_a_full_tile_dropped" and rows == qt:
                p[:, :, qt - 1] = 0.0
            ds = p * (dot @ vh.transpose(2, 3) - dt)
            dv = dv + r16(p).transpose(2, 3) @ dot
            dk = dk + r16(ds).transpose(2, 3) @ qt_
        if fault != "dk_ignores_the_scale":
            dk = dk * scale

        back = lambda t: t.to(dtype).permute(0, 2, 1, 3).contiguous()
        dq, dk, dv = back(dq), back(dk), back(dv)
        if k2 is None:
            return dq, dk, dv, None, None
        dk1, dv1, dk2, dv2 = dk[:, :nk1].contiguous(), dv[:, :nk1].contiguous(), dk[:, nk1:].contiguous(), dv[:, nk1:].contiguous()
        if fault == "seam_key_written_to_the_first_segment":
            # the first key of segment two stores at ITS index 0 of segment one's gradients; its own row stays unwritten
            dk1[:, 0], dv1[:, 0] = dk2[:, 0], dv2[:, 0]
            dk2[:, 0], dv2[:, 0] = 0.0, 0.0
        if fault == "second_segment_dropped":
            dk2, dv2 = torch.zeros_like(dk2), torch.zeros_like(dv2)
        return dq, dk1, dv1, dk2, dv2

    return fn


def framework_chain(fw):
    """fn like ``attention16_bwd()``'s from the framework's own 16-bit chain differentiated by autograd."""
    def fn(q, k, v, k2=None, v2=None, grad_out=None, scale=None):
        leaves = [None if t is None else t.detach().clone().requires_grad_() for t in (q, k, v, k2, v2)]
        fw(*leaves, scale=scale).backward(grad_out)
        return tuple(None if t is None else t.grad for t in leaves)
    return fn
