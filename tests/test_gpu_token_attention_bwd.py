"""GPU: the backward kernels of ``WF.token_attention`` (waldo_token_attention_bwd, csrc/token_attention_bwd.hip) and the
forward that hands them its row statistics (waldo_token_attention_fwd_lse), under
``WF.token_attention_backward_route("kernel")``.  The yardstick is the gradient parity rule of this suite,
``parity.close(got, r32, rel=True, exact=r64)``: 1e-4 of the tensor's largest value plus four times the fp32 framework
route's own distance from fp64, per element; the references are ``WF.token_attention_framework`` differentiated in fp32
and fp64 on the same operands.  Gradients are taken through packed leaves (a (B, N, 2, H, D) kv projection, a
(B, N, 3, H, D) qkv projection), so that the slices' gradients meet.  Every case asserts that the KERNELS served it."""
import pytest
import torch

import lvd_nets_ref as R
from parity import close
from test_gpu_token_attention import (SCALE_FACTORS, large_score_operands, operands, recipe_ops, scale_cases,
                                      scale_moves_the_output, tile_edge_cases)

pytestmark = pytest.mark.gpu


def WF():
    from waldo_amd import functional
    return functional


def kernel(q, k, v, k2=None, v2=None, scale=None):
    """WF.token_attention on a call that the kernel serves, under the kernel route of the backward."""
    assert WF()._token_attention_served(q, k, v, k2, v2) is not None
    with WF().token_attention_backward_route("kernel"):
        return WF().token_attention(q, k, v, k2, v2, scale)


def launches(fn):
    """(fn(), {entry point: calls})."""
    from waldo_amd import _lib
    with _lib.KernelTimer() as timer:
        out = fn()
    return out, {k: len(v) for k, v in timer.pairs.items()}


def served(calls, fwd=1, bwd=1):
    assert calls.get("waldo_token_attention_fwd_lse", 0) == fwd and calls.get("waldo_token_attention_bwd", 0) == bwd, calls
    assert "waldo_token_attention_fwd" not in calls, calls


def leaves_of(ops):
    """(q, kv, kv2 or None) packed from q, k, v[, k2, v2]: detached CPU-independent copies."""
    q, k, v, k2, v2 = ops
    return q.detach().clone(), torch.stack([k, v], 2), None if k2 is None else torch.stack([k2, v2], 2)


def run(fn, packed, go, dtype=torch.float32, scale=None):
    """(out, grad q, grad kv, grad kv2) of ``fn`` on the slices of fresh leaves."""
    q, kv, kv2 = (None if t is None else t.detach().to(dtype).clone().requires_grad_() for t in packed)
    ops = (q, *kv.unbind(2)) if kv2 is None else (q, *kv.unbind(2), *kv2.unbind(2))
    out = fn(*ops, scale=scale)
    out.backward(go.to(dtype))
    return out.detach(), q.grad, kv.grad, None if kv2 is None else kv2.grad


def check(ops, what, scale=None, seed=0, fn=None):
    """The kernel's gradients in q, k, v, k2, v2 against the framework's in fp32 and fp64; returns the kernel's.
    ``fn``: another candidate for the same yardstick (test_token_attention_sensitivity_cpu.py)."""
    packed = leaves_of(ops)
    b, nq, h, d = ops[0].shape
    go = torch.randn(b, nq, h * d, generator=torch.Generator().manual_seed(1000 + seed)).to(ops[0].device)
    if fn is None:
        got, calls = launches(lambda: run(kernel, packed, go, scale=scale))
        served(calls)
    else:
        got = run(fn, packed, go, scale=scale)
    fw = WF().token_attention_framework
    r32, r64 = run(fw, packed, go, scale=scale), run(fw, packed, go, torch.float64, scale=scale)
    close(got[0], r32[0], exact=r64[0], what=f"{what} out")
    for i, name in ((1, "q"), (2, "kv"), (3, "kv2")):
        if got[i] is not None or r32[i] is not None:
            assert torch.isfinite(got[i]).all(), name
            close(got[i], r32[i], rel=True, exact=r64[i], what=f"{what} grad {name}")
    return got


@pytest.mark.parametrize("d", [16, 32, 64])
def test_tile_edges(dev, d):
    """Nq in {1, QT-1, QT, QT+1} x Nk1 in {1, KT-1, KT, KT+1, 2 KT+3} x Nk2 in {absent, 1, KT+1}, QT and KT the
    backward's own tiles: a key tail, a query tail, a seam inside a tile, a seam on a tile boundary, a second segment
    that is all of the last tile."""
    lim = WF().token_attention_bwd_limits()
    assert d in lim["head_dims"]
    for b, h, nq, nk1, nk2, d, seed in tile_edge_cases(lim["q_tile"], lim["k_tile"], d):
        check(operands(dev, b, h, nq, nk1, nk2, d, seed), f"D={d} Nq={nq} Nk1={nk1} Nk2={nk2}", seed=seed)


@pytest.mark.parametrize("d", [16, 32, 64])
@pytest.mark.parametrize("f", SCALE_FACTORS)
def test_a_scale_that_is_not_the_default(dev, d, f):
    """The forward's scale family with the backward's tiles: dQ, dK and P each take the scale that was passed."""
    lim = WF().token_attention_bwd_limits()
    (shape, scale), = [c for c in scale_cases(lim["q_tile"], lim["k_tile"]) if c[0][5] == d and c[1] == f * d ** -0.5]
    ops = operands(dev, *shape[:6], seed=shape[6])
    scale_moves_the_output(ops, scale)
    check(ops, f"D={d} scale={f} D^-1/2", scale=scale)


def test_many_heads_query_blocks_and_key_blocks(dev):
    lim = WF().token_attention_bwd_limits()
    qt, kt = lim["q_tile"], lim["k_tile"]
    check(operands(dev, 3, 8, 2 * qt + 5, 2 * kt + 6, kt + 9, 32, seed=3), "B H = 24, three query blocks, four key blocks")


@pytest.mark.parametrize("shape", [(2, 2, 20, 20, 32, 16), (10, 2, 28, 28, None, 16), (2, 1, 20, 20, 32, 64),
                                   (10, 1, 28, 28, None, 64)])
def test_the_fixture_networks_shapes(dev, shape):
    b, h, nq, nk1, nk2, d = shape
    check(operands(dev, b, h, nq, nk1, nk2, d, seed=7), f"{shape}")


@pytest.mark.parametrize("which", ["pose", "layer"])
def test_the_recipe_shapes(dev, which):
    check(recipe_ops(dev, which), which)


def packed_views(dev, b=3, n=70, m=37, h=2, d=32):
    g = torch.Generator().manual_seed(11)
    big = torch.randn(b, n + 5, 3 * h * d, generator=g).to(dev).requires_grad_()
    kvbig = torch.randn(b, m + 3, 2 * h * d, generator=g).to(dev).requires_grad_()
    qkv = big[:, 2:n + 2].view(b, n, 3, h, d)
    kv = kvbig[:, 3:].view(b, m, 2, h, d)
    go = torch.randn(b, n, h * d, generator=g).to(dev)
    return big, kvbig, qkv, kv, go


def test_operands_in_place_give_the_bits_of_contiguous_copies(dev):
    """q, k, v the slices of a (B, N, 3 H D) tensor that is itself a slice of a longer one, k2, v2 the slices of a
    (B, M, 2 H D) one: the gradients, in place in the long tensors, bit-equal to those of the call on copies."""
    big, kvbig, qkv, kv, go = packed_views(dev)
    q, k, v = qkv.unbind(2)
    k2, v2 = kv.unbind(2)
    assert not q.is_contiguous() and q.stride(0) != q.shape[1] * q.stride(1)
    _, calls = launches(lambda: kernel(q, k, v, k2, v2).backward(go))
    served(calls)
    copies = [t.detach().contiguous().requires_grad_() for t in (q, k, v, k2, v2)]
    kernel(*copies).backward(go)
    b, n, m = q.shape[0], q.shape[1], k2.shape[1]
    assert torch.equal(big.grad[:, 2:n + 2].view(b, n, 3, *q.shape[2:]), torch.stack([t.grad for t in copies[:3]], 2))
    assert torch.equal(kvbig.grad[:, 3:].view(b, m, 2, *q.shape[2:]), torch.stack([t.grad for t in copies[3:]], 2))
    assert not big.grad[:, :2].any() and not big.grad[:, n + 2:].any() and not kvbig.grad[:, :3].any()


def test_broadcast_keys_sum_their_gradients_over_the_batch(dev):
    b, n, m, h, d = 3, 70, 37, 2, 32
    g = torch.Generator().manual_seed(12)
    q0 = (torch.randn(b, n, h, d, generator=g) * 1.4).to(dev)
    kv0 = (torch.randn(1, m, 2, h, d, generator=g) * 1.4).to(dev)
    go = torch.randn(b, n, h * d, generator=g).to(dev)

    def grads(fn, dtype, expand):
        q, kv = (t.detach().to(dtype).clone().requires_grad_() for t in (q0, kv0))
        k, v = expand(kv).unbind(2)
        fn(q, k, v).backward(go.to(dtype))
        return q.grad, kv.grad

    view = lambda kv: kv.expand(b, -1, -1, -1, -1)
    (gq, gkv), calls = launches(lambda: grads(kernel, torch.float32, view))
    served(calls)
    assert view(kv0).stride(0) == 0 and gkv.shape == kv0.shape
    fw = WF().token_attention_framework
    r32, r64 = grads(fw, torch.float32, view), grads(fw, torch.float64, view)
    close(gq, r32[0], rel=True, exact=r64[0], what="broadcast keys: grad q")
    close(gkv, r32[1], rel=True, exact=r64[1], what="broadcast keys: grad kv")
    # the batch sum of the per-element gradients of a contiguous copy
    kvc = kv0.detach().expand(b, -1, -1, -1, -1).contiguous().requires_grad_()
    kernel(q0, *kvc.unbind(2)).backward(go)
    close(gkv, kvc.grad.sum(0, keepdim=True), rel=True, exact=r64[1], what="broadcast keys: the batch sum")


def test_a_grad_out_that_is_not_contiguous(dev):
    ops = operands(dev, 2, 2, 70, 65, 9, 32, seed=14)
    packed = leaves_of(ops)
    go2 = torch.randn(2, 70, 2 * 64, generator=torch.Generator().manual_seed(15)).to(dev)
    go = go2[..., ::2]
    assert not go.is_contiguous()
    a = run(kernel, packed, go)
    c = run(kernel, packed, go.contiguous())
    for x, y in zip(a, c):
        assert torch.equal(x, y)


def test_a_contiguous_grad_out_off_the_16_byte_boundary(dev):
    """``out.backward(go)`` with go a contiguous view one float into a buffer: the kernel serves it, with the bits of
    the call on an aligned copy."""
    ops = operands(dev, 2, 2, 70, 65, 9, 32, seed=44)
    packed = leaves_of(ops)
    n = 2 * 70 * 64
    buf = torch.randn(n + 4, generator=torch.Generator().manual_seed(45)).to(dev)
    go = buf[1:1 + n].view(2, 70, 64)
    assert go.is_contiguous() and go.data_ptr() % 16 == 4
    got, calls = launches(lambda: run(kernel, packed, go))
    served(calls)
    aligned = go.clone()
    assert aligned.data_ptr() % 16 == 0
    for x, y in zip(got, run(kernel, packed, aligned)):
        assert torch.equal(x, y)


def test_the_gradient_of_a_cat_is_a_view_off_the_16_byte_boundary(dev):
    """``cat([p, out.reshape(-1)])`` with p one element: autograd hands ``out`` a narrow view one float into the
    gradient of the cat."""
    ops = operands(dev, 2, 2, 70, 65, 9, 32, seed=46)
    packed = leaves_of(ops)
    w = torch.randn(1 + 2 * 70 * 64, generator=torch.Generator().manual_seed(47)).to(dev)
    seen = []

    def through_cat(*a, **kw):
        out = kernel(*a, **kw)
        out.register_hook(lambda g: seen.append((g.is_contiguous(), g.data_ptr() % 16)))
        p = torch.zeros(1, device=dev, requires_grad=True)
        return torch.cat([p, out.reshape(-1)])

    got, calls = launches(lambda: run(through_cat, packed, w))
    served(calls)
    assert seen == [(True, 4)], seen
    want = run(kernel, packed, w[1:].clone().view(2, 70, 64))
    for x, y in zip(got[1:], want[1:]):
        assert torch.equal(x, y)
    assert torch.equal(got[0][1:].view(2, 70, 64), want[0])


def test_broadcast_queries_and_a_broadcast_second_segment(dev):
    """q and k2 / v2 expanded over the batch (batch stride 0), k / v per batch element: the gradients at the
    un-expanded leaves against the framework's, and against the batch sum of the gradients of contiguous copies."""
    b, n, m, m2, h, d = 3, 70, 37, 41, 2, 32
    g = torch.Generator().manual_seed(48)
    q0 = (torch.randn(1, n, h, d, generator=g) * 1.4).to(dev)
    kv0 = (torch.randn(b, m, 2, h, d, generator=g) * 1.4).to(dev)
    kv20 = (torch.randn(1, m2, 2, h, d, generator=g) * 1.4).to(dev)
    go = torch.randn(b, n, h * d, generator=g).to(dev)

    def grads(fn, dtype, expand):
        q, kv, kv2 = (t.detach().to(dtype).clone().requires_grad_() for t in (q0, kv0, kv20))
        qe, kv2e = expand(q), expand(kv2)
        fn(qe, *kv.unbind(2), *kv2e.unbind(2)).backward(go.to(dtype))
        return q.grad, kv.grad, kv2.grad

    view = lambda t: t.expand(b, *t.shape[1:])
    got, calls = launches(lambda: grads(kernel, torch.float32, view))
    served(calls)
    assert view(q0).stride(0) == 0 and view(kv20).stride(0) == 0
    assert got[0].shape == q0.shape and got[2].shape == kv20.shape
    fw = WF().token_attention_framework
    r32, r64 = grads(fw, torch.float32, view), grads(fw, torch.float64, view)
    for i, name in enumerate(("q", "kv", "kv2")):
        close(got[i], r32[i], rel=True, exact=r64[i], what=f"broadcast q and kv2: grad {name}")
    # the batch sum of the per-element gradients of contiguous copies
    qc, kv2c = (view(t).contiguous().requires_grad_() for t in (q0, kv20))
    kvc = kv0.clone().requires_grad_()
    kernel(qc, *kvc.unbind(2), *kv2c.unbind(2)).backward(go)
    close(got[0], qc.grad.sum(0, keepdim=True), rel=True, exact=r64[0], what="broadcast q: the batch sum")
    close(got[2], kv2c.grad.sum(0, keepdim=True), rel=True, exact=r64[2], what="broadcast kv2: the batch sum")
    assert torch.equal(got[1], kvc.grad)


ONE_KEY_FACTORS = (None, 0.37)   # of D ** -0.5; None: the default scale


def one_key_cases(qt):
    """((b, h, nq, nk1, nk2, d, seed), scale): rows with ONE key, where P = 1, out = v and dS = 0 hold exactly."""
    return [((2, 2, nq, 1, None, d, 50 + i), None if f is None else f * d ** -0.5)
            for i, (d, nq) in enumerate((d, nq) for d in (16, 32, 64) for nq in (1, 17, qt + 1)) for f in ONE_KEY_FACTORS]


def check_one_key(ops, scale, fn, seed):
    """out IS v, whatever the query; grad q and grad k have no non-zero element -- delta and dP are one fma chain on
    the same operands, so dS = P (dP - delta) is exactly 0 --, grad v is the sum of grad_out over the queries."""
    q, k, v, _, _ = ops
    b, nq, h, d = q.shape
    assert k.shape[1] == 1
    go = torch.randn(b, nq, h * d, generator=torch.Generator().manual_seed(2000 + seed)).to(q.device)
    out, gq, gkv, _ = run(fn, leaves_of(ops), go, scale=scale)
    print(f"[one key] D={d} Nq={nq} scale={scale}: |out - v| {(out - v.reshape(b, 1, h * d)).abs().max().item():.3e}  "
          f"|grad q| {gq.abs().max().item():.3e}  |grad k| {gkv[:, :, 0].abs().max().item():.3e}")
    assert torch.equal(out, v.reshape(b, 1, h * d).expand(b, nq, h * d))
    assert torch.count_nonzero(gq) == 0
    assert torch.count_nonzero(gkv[:, :, 0]) == 0
    want = go.view(b, nq, h, d).double().sum(1, keepdim=True)
    close(gkv[:, :, 1], go.view(b, nq, h, d).sum(1, keepdim=True), rel=True, exact=want, what=f"one key: grad v D={d} Nq={nq}")


@pytest.mark.parametrize("d", [16, 32, 64])
def test_one_key(dev, d):
    qt = WF().token_attention_bwd_limits()["q_tile"]
    for shape, scale in one_key_cases(qt):
        if shape[5] != d:
            continue
        ops = operands(dev, *shape[:6], seed=shape[6])
        _, calls = launches(lambda: check_one_key(ops, scale, kernel, shape[6]))
        served(calls)
        with torch.no_grad():   # the plain forward too
            assert torch.equal(kernel(*ops, scale=scale), ops[2].reshape(2, 1, 2 * d).expand(2, shape[2], 2 * d))


def nan_operands(dev):
    lim = WF().token_attention_bwd_limits()
    ops = operands(dev, 2, 2, lim["q_tile"] + 1, lim["k_tile"] + 1, 9, 32, seed=43)
    go = torch.randn(2, lim["q_tile"] + 1, 64, generator=torch.Generator().manual_seed(49)).to(dev)
    return ops, go


def non_finite(t):
    return ~torch.isfinite(t)


def test_a_nan_in_one_query_row_stays_visible_and_stays_in_its_row(dev):
    """One NaN in q[0, 7, head 1]: that row of out and of grad q, and the gradients of every key and value of (0, head 1),
    are non-finite -- in the framework and in the kernels alike --, everything else is finite, within the bound of its
    references, and where the NaN cannot be seen, the bits of the run without it."""
    ops, go = nan_operands(dev)
    d = 32
    bad = [t.clone() for t in ops]
    bad[0][0, 7, 1, 3] = float("nan")
    fw = WF().token_attention_framework
    r32, r64 = run(fw, leaves_of(bad), go), run(fw, leaves_of(bad), go, torch.float64)
    expect = [torch.zeros_like(t, dtype=torch.bool) for t in r32]
    expect[0][0, 7, d:2 * d] = True
    expect[1][0, 7, 1, :] = True
    expect[2][0, :, :, 1, :] = True
    expect[3][0, :, :, 1, :] = True
    assert [int(e.sum()) for e in expect] == [32, 32, 2080 + 2080, 288 + 288]
    for t, e in zip(r32, expect):
        assert torch.equal(non_finite(t), e)
    got, calls = launches(lambda: run(kernel, leaves_of(bad), go))
    served(calls)
    for name, t, e in zip(("out", "grad q", "grad kv", "grad kv2"), got, expect):
        assert torch.equal(non_finite(t), e), (name, int(non_finite(t).sum()), int(e.sum()))
    zero = lambda t, e: torch.where(e, torch.zeros_like(t), t)
    for i, name in enumerate(("out", "grad q", "grad kv", "grad kv2")):
        close(zero(got[i], expect[i]), zero(r32[i], expect[i]), rel=i > 0, exact=zero(r64[i], expect[i]),
              what=f"NaN in a query row: the finite part of {name}")
    clean = run(kernel, leaves_of(ops), go)
    for i in (0, 1):
        assert torch.equal(zero(got[i], expect[i]), zero(clean[i], expect[i]))


def test_a_nan_in_one_key_of_the_second_segment_takes_its_batch_and_head_only(dev):
    ops, go = nan_operands(dev)
    d = 32
    bad = [t.clone() for t in ops]
    bad[3][1, 4, 0, 5] = float("nan")
    expect = [torch.zeros_like(t, dtype=torch.bool) for t in run(WF().token_attention_framework, leaves_of(ops), go)]
    expect[0][1, :, 0:d] = True
    expect[1][1, :, 0, :] = True
    expect[2][1, :, :, 0, :] = True
    expect[3][1, :, :, 0, :] = True
    r32 = run(WF().token_attention_framework, leaves_of(bad), go)
    got, calls = launches(lambda: run(kernel, leaves_of(bad), go))
    served(calls)
    clean = run(kernel, leaves_of(ops), go)
    for name, t, r, c, e in zip(("out", "grad q", "grad kv", "grad kv2"), got, r32, clean, expect):
        assert torch.equal(non_finite(r), e), name
        assert torch.equal(non_finite(t), e), (name, int(non_finite(t).sum()), int(e.sum()))
        assert torch.equal(torch.where(e, torch.zeros_like(t), t), torch.where(e, torch.zeros_like(c), c)), name


def test_large_scores(dev):
    """The operands of the forward's test_large_scores_and_the_online_rescale: scores from below -60 to above +60, the
    row maximum rising in every tile."""
    kt = WF().token_attention_limits()["k_tile"]
    q, k, v, k2, v2 = large_score_operands(dev, kt)
    scores = torch.einsum("bihd,bjhd->bhij", q.double(), torch.cat([k, k2], 1).double()) * 64 ** -0.5
    assert scores.max() > 60 and scores.min() < -60
    got = check((q, k, v, k2, v2), "scores up to +-60")
    for t in got:
        assert torch.isfinite(t).all()


def test_large_scores_with_two_rows_far_below_zero(dev):
    """The same with every score of the first and of the last query row 160 lower: their lse is near -100, and
    exp(-lse) is beyond fp32.  Nq = 70 leaves 58 dead rows in the last query tile of the dK/dV kernel, which are read
    through a clamped index: a P of theirs that were exp(0 - lse) of such a row, not 0, is infinite and meets their
    zero operands."""
    kt = WF().token_attention_limits()["k_tile"]
    got = check(large_score_operands(dev, kt, low_rows=True), "scores up to +-60, two rows 160 lower")
    for t in got:
        assert torch.isfinite(t).all()


def test_equal_scores_give_every_key_the_mean_of_grad_out(dev):
    """Zero q: P is uniform, 1 / Nk, and with Nq = Nk the gradient of every value row is the mean of grad_out over the
    queries (Nq = 126 terms of order 1 summed in fp32: far below 1e-5)."""
    kt = WF().token_attention_bwd_limits()["k_tile"]
    b, h, nk1, nk2, d = 2, 2, kt + 3, kt - 5, 32
    nq = nk1 + nk2
    q, k, v, k2, v2 = operands(dev, b, h, nq, nk1, nk2, d, seed=19)
    go = torch.randn(b, nq, h * d, generator=torch.Generator().manual_seed(20)).to(dev)
    _, gq, gkv, gkv2 = run(kernel, leaves_of((torch.zeros_like(q), k, v, k2, v2)), go)
    mean = go.double().mean(1).view(b, 1, h, d)
    assert (gkv[:, :, 1].double() - mean).abs().max().item() < 1e-5
    assert (gkv2[:, :, 1].double() - mean).abs().max().item() < 1e-5


@pytest.mark.parametrize("wanted", [("v",), ("q",), ("k2", "v2"), ("k",), ("q", "v2")])
def test_only_what_is_asked_for(dev, monkeypatch, wanted):
    names = ("q", "k", "v", "k2", "v2")
    ops = operands(dev, 2, 2, 70, 65, 37, 32, seed=21)
    go = torch.randn(2, 70, 64, generator=torch.Generator().manual_seed(22)).to(dev)
    every = [t.clone().requires_grad_() for t in ops]
    kernel(*every).backward(go)

    def boom(*a, **kw):
        raise AssertionError("token_attention_framework called from the kernel route")

    some = [t.clone().requires_grad_(n in wanted) for t, n in zip(ops, names)]
    out = kernel(*some)
    monkeypatch.setattr(WF(), "token_attention_framework", boom)
    _, calls = launches(lambda: out.backward(go))
    assert calls == {"waldo_token_attention_bwd": 1}, calls
    for t, full, n in zip(some, every, names):
        if n in wanted:
            assert torch.equal(t.grad, full.grad), n
        else:
            assert t.grad is None, n


def row_statistics(ops, scale=None):
    """(the forward's saved lse, its output) with the bits of the plain forward, and lse against torch.logsumexp of the
    scaled scores in fp32 and fp64 through ``close``."""
    b, nq, h, d = ops[0].shape
    with torch.no_grad():
        plain, calls = launches(lambda: kernel(*ops, scale=scale))
    assert calls == {"waldo_token_attention_fwd": 1}, calls   # no gradient wanted: no row statistics
    out, calls = launches(lambda: kernel(ops[0].clone().requires_grad_(), *ops[1:], scale=scale))
    assert calls == {"waldo_token_attention_fwd_lse": 1}, calls
    assert torch.equal(out.detach(), plain)
    lse = out.grad_fn.saved_tensors[-1]
    assert lse.shape == (b, h, nq) and lse.dtype == torch.float32
    scale = d ** -0.5 if scale is None else scale
    want = [torch.logsumexp(torch.einsum("bihd,bjhd->bhij", ops[0].to(t), torch.cat([ops[1], ops[3]], 1).to(t)) * scale,
                            dim=-1) for t in (torch.float32, torch.float64)]
    close(lse, want[0], exact=want[1], what=f"lse D={d} scale={scale:.4f}")
    return lse, want[1]


@pytest.mark.parametrize("f", [None, 0.37])
@pytest.mark.parametrize("d", [16, 32, 64])
def test_forward_bits_and_row_statistics(dev, d, f):
    ops = operands(dev, 2, 3, 70, 65, 37, d, seed=23)
    lse, want = row_statistics(ops, None if f is None else f * d ** -0.5)
    if d == 64 and f is None:
        assert (lse.double() - want).abs().max().item() < 1e-5


def test_row_statistics_of_large_scores(dev):
    """lse of about 60 (and of about -100 in the two low rows): m carries it, log(l) is small."""
    kt = WF().token_attention_limits()["k_tile"]
    for low_rows in (False, True):
        lse, want = row_statistics(large_score_operands(dev, kt, low_rows))
        assert want[..., 1:-1].min() > 55 and (want[..., 0].max() < -95) == low_rows


def test_same_bits_from_run_to_run_in_both_deterministic_modes(dev):
    ops = operands(dev, 3, 4, 130, 100, 77, 64, seed=29)
    packed = leaves_of(ops)
    go = torch.randn(3, 130, 4 * 64, generator=torch.Generator().manual_seed(30)).to(dev)
    runs = []
    for mode in (False, True):
        with WF().deterministic(mode):
            runs += [run(kernel, packed, go) for _ in range(3)]
    for r in runs[1:]:
        for x, y in zip(r, runs[0]):
            assert torch.equal(x, y)


def test_forward_and_backward_replay_from_one_graph_with_the_eager_bits(dev):
    ops = operands(dev, 2, 4, 70, 65, 9, 64, seed=31)
    q0, kv, kv2 = leaves_of(ops)
    go = torch.randn(2, 70, 4 * 64, generator=torch.Generator().manual_seed(32)).to(dev)
    kv.requires_grad_(), kv2.requires_grad_()

    def step(q):
        out = kernel(q, *kv.unbind(2), *kv2.unbind(2))
        return (out, *torch.autograd.grad(out, [q, kv, kv2], go))

    eager = [t.detach().clone() for t in step(q0.clone().requires_grad_())]
    static_q = q0.clone().requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # (warm-up off the default stream, as capture asks for)
        step(static_q)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step(static_q)
    with torch.no_grad():
        static_q.zero_()
    graph.replay()
    zeros = [t.detach().clone() for t in static]
    with torch.no_grad():
        static_q.copy_(q0)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(static, eager):
        assert torch.equal(got.detach(), want)
    assert not torch.equal(zeros[2], eager[2])   # the replay read its input anew


def test_the_copy_of_an_unaligned_grad_out_replays_from_a_graph(dev):
    ops = operands(dev, 2, 2, 70, 65, 9, 32, seed=51)
    q, kv, kv2 = leaves_of(ops)
    q.requires_grad_(), kv.requires_grad_(), kv2.requires_grad_()
    n = 2 * 70 * 64
    buf = torch.randn(n + 4, generator=torch.Generator().manual_seed(52)).to(dev)
    go = buf[1:1 + n].view(2, 70, 64)
    assert go.is_contiguous() and go.data_ptr() % 16 == 4

    def step():
        out = kernel(q, *kv.unbind(2), *kv2.unbind(2))
        return torch.autograd.grad(out, [q, kv, kv2], go)

    eager = [t.clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # (warm-up off the default stream, as capture asks for)
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    buf.mul_(2.0)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(static, eager):   # the replay copied grad_out anew: twice the gradients, exactly
        assert torch.equal(got, 2.0 * want)


def test_no_score_tensor(dev):
    """Self-attention of 2048 tokens, 8 heads, through a packed leaf: forward + backward stay below the bytes of ONE
    (B, H, Nq, Nk) fp32 score tensor, 128 MiB, above the level before the forward.  The kernel route needs about
    32 MiB (out, grad_out, three gradients, the packed gradient); a route that holds the softmax output and its
    gradient cannot pass."""
    b, h, n, d = 1, 8, 2048, 64
    g = torch.Generator().manual_seed(33)
    qkv = (torch.randn(b, n, 3, h, d, generator=g) * 1.4).to(dev).requires_grad_()
    go = torch.randn(b, n, h * d, generator=g).to(dev)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    _, calls = launches(lambda: kernel(*qkv.unbind(2)).backward(go))
    torch.cuda.synchronize()
    served(calls)
    peak = torch.cuda.max_memory_allocated() - before
    print(f"[memory] forward + backward: {peak / 2 ** 20:.1f} MiB above the inputs")
    assert peak < b * h * n * n * 4
    assert torch.isfinite(qkv.grad).all()


def test_the_switch_and_the_route_of_a_node(dev, monkeypatch):
    wf = WF()
    ops = operands(dev, 2, 2, 70, 65, 37, 32, seed=35)
    go = torch.randn(2, 70, 64, generator=torch.Generator().manual_seed(36)).to(dev)
    # "framework": the parent's gradients, the recompute differentiated by hand
    leaves = [t.clone().requires_grad_() for t in ops]
    with wf.token_attention_backward_route("framework"):
        assert wf._token_attention_served(*leaves) is not None
        out, calls = launches(lambda: wf.token_attention(*leaves))
    assert calls == {"waldo_token_attention_fwd": 1}, calls
    with wf.token_attention_backward_route("kernel"):   # the node keeps the route of its forward
        _, calls = launches(lambda: out.backward(go))
    assert "waldo_token_attention_bwd" not in calls, calls
    hand = [t.detach().clone().requires_grad_() for t in ops]
    want = torch.autograd.grad(wf.token_attention_framework(*hand), hand, go)
    for t, w in zip(leaves, want):
        assert torch.equal(t.grad, w)
    # and the other way round
    leaves = [t.clone().requires_grad_() for t in ops]
    out = kernel(*leaves)
    monkeypatch.setattr(wf, "token_attention_framework", lambda *a, **kw: pytest.fail("the framework route ran"))
    with wf.token_attention_backward_route("framework"):
        _, calls = launches(lambda: out.backward(go))
    assert calls == {"waldo_token_attention_bwd": 1}, calls
    for t, w in zip(leaves, want):
        close(t.grad, w, rel=True, what="kernel against framework")


def test_lvd_parameter_gradients_under_the_kernel_route(dev):
    """The bound of test_fused_and_framework_routes_agree_on_outputs_and_parameter_gradients, with the attention's
    backward in the kernel."""
    prefix = R.CASES[0]
    opt, keys, d = R.case(prefix)
    g = torch.Generator().manual_seed(41)
    weights = {k: torch.randn(d[k + "32"].shape, generator=g) for k in R.OUTPUTS}

    def grads(net, inp):
        net.zero_grad(set_to_none=True)
        out = R.run(net, inp, opt["ctx_len"])
        sum((out[k] * weights[k].to(out[k])).sum() for k in R.OUTPUTS).backward()
        return {k: p.grad for k, p in net.named_parameters()}

    with WF().token_attention_backward_route("kernel"):
        fused, calls = launches(lambda: grads(R.build(prefix, dev, fused=True), d["input"].to(dev)))
    n = opt["oe_depth"] + opt["pe_depth"]
    assert calls.get("waldo_token_attention_fwd_lse") == n and calls.get("waldo_token_attention_bwd") == n, calls
    plain = grads(R.build(prefix, dev, fused=False), d["input"].to(dev))
    exact = grads(R.build(prefix, "cpu", fused=False, dtype=torch.float64), d["input"].double())
    for k in keys:
        assert fused[k] is not None, k
        close(fused[k], plain[k], rel=True, exact=exact[k], what=f"{prefix} grad {k}")


def test_lvd_step_with_the_networks_under_the_kernel_route(dev):
    from waldo_amd.tools.lvd_step import LvdStep
    step = LvdStep(1, dev, seed=1, nets="reference")
    with WF().token_attention_backward_route("kernel"):
        loss, calls = launches(step)
    assert torch.isfinite(loss)
    assert calls.get("waldo_token_attention_fwd_lse") == 4 and calls.get("waldo_token_attention_bwd") == 4, calls
    assert "waldo_token_attention_fwd" not in calls, calls
    missing = [k for k, p in step.net.named_parameters() if p.grad is None]
    assert not missing, missing
    assert step.grads_finite()
