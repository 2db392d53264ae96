"""GPU: the 16-bit token attention's backward (waldo_token_attention_fwd_lse_dt / waldo_token_attention_bwd_dt,
csrc/token_attention_16_bwd.hip) under ``WF.token_attention_16bit_route("kernel")`` and
``WF.token_attention_16bit_backward_route("kernel")``, in bf16 and fp16, against the bound of
tests/token_attention_16bit_bwd.py -- derived from the kernels' arithmetic contract there, and shown on the CPU
(test_token_attention_16bit_bwd_cpu.py) to refuse the framework's own 16-bit chain and eight planted faults.  Every call
asserts that the 16-bit predicate served it and that its launches were exactly one ``waldo_token_attention_fwd_lse_dt``
and one ``waldo_token_attention_bwd_dt``."""
import pytest
import torch

import test_gpu_token_attention as FWD
from token_attention_16bit_bwd import DTYPES, KT, NAMES, QT, exact_and_bounds, family, grad_out_for, to16, within_bound

pytestmark = pytest.mark.gpu

LAUNCHES = {"waldo_token_attention_fwd_lse_dt": 1, "waldo_token_attention_bwd_dt": 1}


def WF():
    from waldo_amd import functional
    return functional


def launches(fn):
    from waldo_amd import _lib
    with _lib.KernelTimer() as timer:
        out = fn()
    return out, {k: len(v) for k, v in timer.pairs.items()}


def run(ops, go, scale=None, need=(True,) * 5, calls=LAUNCHES, bwd_route="kernel"):
    """(out, the five gradients) of ``WF.token_attention`` on leaves that are clones of ``ops``, under both switches,
    after making sure that the 16-bit kernel serves the call; the launches made were ``calls``."""
    wf = WF()
    leaves = [None if t is None else t.detach().clone().requires_grad_(n) for t, n in zip(ops, need)]

    def both():
        with wf.token_attention_16bit_route("kernel"), wf.token_attention_16bit_backward_route(bwd_route):
            assert wf._token_attention_served(*leaves) is None
            assert wf._token_attention_served_16bit(*leaves) is not None
            out = wf.token_attention(*leaves, scale)
        out.backward(go)   # (outside the switches: the route travels with the node)
        return out.detach()

    out, made = launches(both)
    assert made == calls, made
    return out, tuple(None if t is None else t.grad for t in leaves)


def check(ops, go, what, scale=None):
    _, grads = run(ops, go, scale)
    return within_bound(grads, ops, go, scale, what)


def test_the_tiles_are_the_helpers():
    lim = WF().token_attention_16bit_limits()
    assert (lim["q_tile"], lim["k_tile"]) == (QT, KT) and lim == WF().token_attention_bwd_limits()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [16, 32, 64])
def test_tile_edges(dev, d, dtype):
    worst = {}
    for ops, go, scale, what in family("tile", dev, dtype, dims=(d,)):
        for k, r in check(ops, go, what, scale).items():
            worst[k] = max(worst.get(k, 0.0), r)
    print(f"[bound16-bwd] tile edges D={d} {dtype}: worst {({k: round(r, 3) for k, r in worst.items()})}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_scales_that_are_not_the_default(dev, dtype):
    cases = family("scale", dev, dtype)
    assert len(cases) == 3 * len(FWD.SCALE_FACTORS)
    for ops, go, scale, what in cases:
        ratios = check(ops, go, what, scale)
        if scale == 0.0:   # uniform weights: no gradient in q and k
            _, grads = run(ops, go, scale)
            assert all(not g.any() for g in (grads[0], grads[1], grads[3]))
        assert set(ratios) == set(NAMES)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("low_rows", FWD.LARGE_SCORE_CASES)
def test_large_scores(dev, low_rows, dtype):
    (ops, go, scale, what), = [c for c in family("large", dev, dtype) if c[3].endswith(str(low_rows))]
    check(ops, go, what, scale)


@pytest.mark.parametrize("dtype", DTYPES)
def test_only_the_wanted_gradients(dev, dtype):
    ops = to16(FWD.operands(dev, 2, 2, 70, 65, 37, 32, seed=23), dtype)
    go = grad_out_for(ops, 23).to(dev, dtype)
    _, full = run(ops, go)
    for wanted in ((0,), (1, 2), (3, 4), (2,)):
        need = tuple(i in wanted for i in range(5))
        _, grads = run(ops, go, need=need)
        for i in range(5):
            if need[i]:
                assert torch.equal(grads[i], full[i]), (wanted, NAMES[i])
            else:
                assert grads[i] is None, (wanted, NAMES[i])


@pytest.mark.parametrize("dtype", DTYPES)
def test_operands_are_read_where_they_lie(dev, dtype):
    """The slices of packed ``qkv`` / ``kv`` projections as leaves' views: the gradients arrive in the packed leaves and
    are those of the call on contiguous copies; keys broadcast over the batch: the ``expand``ed leaf's gradient, which
    autograd sums over the batch, is within the bound summed over the batch."""
    wf = WF()
    b, n, m, h, d = 3, 70, 37, 2, 32
    g = torch.Generator().manual_seed(11)
    qkv0 = (torch.randn(b, n, 3, h, d, generator=g) * 1.4).to(dev, dtype)
    kv0 = (torch.randn(b, m, 2, h, d, generator=g) * 1.4).to(dev, dtype)
    go = torch.randn(b, n, h * d, generator=g).to(dev, dtype)
    qkv, kv = qkv0.clone().requires_grad_(), kv0.clone().requires_grad_()

    def packed():
        with wf.token_attention_16bit_route("kernel"), wf.token_attention_16bit_backward_route("kernel"):
            ops = (*qkv.unbind(2), *kv.unbind(2))
            assert not ops[0].is_contiguous() and wf._token_attention_served_16bit(*ops) is not None
            wf.token_attention(*ops).backward(go)

    _, made = launches(packed)
    assert made == LAUNCHES, made
    ops = (*qkv0.unbind(2), *kv0.unbind(2))
    _, want = run(tuple(t.contiguous() for t in ops), go)
    assert torch.equal(qkv.grad, torch.stack(want[:3], 2)) and torch.equal(kv.grad, torch.stack(want[3:], 2))
    within_bound(want, ops, go, what="packed views")

    # one key sequence for the whole batch
    k1, v1 = kv0[:1, :, 0].clone().requires_grad_(), kv0[:1, :, 1].clone().requires_grad_()
    q = qkv0[:, :, 0].contiguous()

    def broadcast():
        with wf.token_attention_16bit_route("kernel"), wf.token_attention_16bit_backward_route("kernel"):
            ke, ve = k1.expand(b, -1, -1, -1), v1.expand(b, -1, -1, -1)
            assert ke.stride(0) == 0 and wf._token_attention_served_16bit(q, ke, ve, None, None) is not None
            wf.token_attention(q, ke, ve).backward(go)

    _, made = launches(broadcast)
    assert made == LAUNCHES, made
    full = (q, k1.detach().expand(b, -1, -1, -1), v1.detach().expand(b, -1, -1, -1), None, None)
    exact, bound = exact_and_bounds(full, go)
    for name, got in (("dk", k1.grad), ("dv", v1.grad)):
        ratio = ((got.double() - exact[name].sum(0, keepdim=True)).abs() / bound[name].sum(0, keepdim=True)).max().item()
        print(f"[bound16-bwd] broadcast keys {dtype} {name}: {ratio:.3g} x the bound summed over the batch")
        assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_grad_out_that_is_not_dense_rows_on_16_bytes(dev, dtype):
    """The gradient that arrives through a ``cat`` (a contiguous view off the 16-byte boundary) and a strided one give
    the gradients of their contiguous copy, bit for bit; one of another dtype those of its rounding."""
    wf = WF()
    ops = to16(FWD.operands(dev, 2, 2, 70, 65, 9, 32, seed=29), dtype)
    go = grad_out_for(ops, 29).to(dev, dtype)
    _, want = run(ops, go)

    def through(post, upstream):
        leaves = [t.detach().clone().requires_grad_() for t in ops]

        def both():
            with wf.token_attention_16bit_route("kernel"), wf.token_attention_16bit_backward_route("kernel"):
                out = wf.token_attention(*leaves)
            post(out).backward(upstream)

        _, made = launches(both)
        assert made == LAUNCHES, made
        return tuple(t.grad for t in leaves)

    # the gradient of a cat's second part starts 2 * 4 bytes into the upstream gradient
    pad = torch.zeros(4, device=dev, dtype=dtype)
    up = torch.cat([pad, go.reshape(-1)])
    assert (up.data_ptr() + 2 * 4) % 16 != 0
    got = through(lambda out: torch.cat([pad, out.reshape(-1)]), up)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # a strided gradient: out is read through a transpose
    got = through(lambda out: out.transpose(0, 1), go.transpose(0, 1).contiguous())
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # an fp32 gradient: rounded once to the operands' type
    go32 = grad_out_for(ops, 31).to(dev)
    leaves = [t.detach().clone().requires_grad_() for t in ops]
    with wf.token_attention_16bit_route("kernel"), wf.token_attention_16bit_backward_route("kernel"):
        out = wf.token_attention(*leaves)
    got = torch.autograd.grad(out.float(), leaves, go32)
    _, want32 = run(ops, go32.to(dtype))
    assert all(torch.equal(a, b) for a, b in zip(got, want32))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [16, 32, 64])
def test_out_of_the_node_has_the_bits_of_the_plain_forward(dev, d, dtype):
    wf = WF()
    for c in ((2, 2, 65, 70, 9, d, 41), (1, 2, 130, 1, None, d, 42)):
        ops = to16(FWD.operands(dev, *c[:6], seed=c[6]), dtype)
        out, _ = run(ops, grad_out_for(ops, 1).to(dev, dtype))
        with torch.no_grad(), wf.token_attention_16bit_route("kernel"), wf.token_attention_16bit_backward_route("kernel"):
            plain, made = launches(lambda: wf.token_attention(*ops))
        assert made == {"waldo_token_attention_fwd_dt": 1}, made   # no node: no lse
        assert torch.equal(out.view(torch.int16), plain.view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES)
def test_same_bits_from_run_to_run_in_either_deterministic_mode_and_in_a_graph(dev, dtype):
    wf = WF()
    ops = to16(FWD.operands(dev, 2, 4, 70, 65, 9, 64, seed=31), dtype)
    go = grad_out_for(ops, 31).to(dev, dtype)
    _, eager = run(ops, go)
    _, again = run(ops, go)
    assert all(torch.equal(a, b) for a, b in zip(eager, again))
    was = wf.is_deterministic()
    for mode in (True, False):
        wf.set_deterministic(mode)
        try:
            _, got = run(ops, go)
        finally:
            wf.set_deterministic(was)
        assert all(torch.equal(a, b) for a, b in zip(eager, got)), mode

    # forward + backward captured in one graph
    static = [t.clone().requires_grad_() for t in ops]

    def step():
        with wf.token_attention_16bit_route("kernel"), wf.token_attention_16bit_backward_route("kernel"):
            out = wf.token_attention(*static)
        return torch.autograd.grad(out, static, go)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # (warm-up off the default stream, as capture asks for)
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grads = step()
    with torch.no_grad():
        static[0].zero_()
    graph.replay()
    zeros = [g.clone() for g in grads]
    with torch.no_grad():
        static[0].copy_(ops[0])
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, grads))
    assert not torch.equal(zeros[1], eager[1])   # the replay read its input anew


def test_no_score_sized_memory(dev):
    """1 x 2 heads x 1024 x 1024 x 64 in bf16: forward + backward allocate less than 2 MB above the operands at their
    peak -- out, lse, delta, the three gradients and the loss's gradient are 1.3 MB; the score tensor alone would be
    4 MB."""
    wf = WF()
    ops = to16(FWD.operands(dev, 1, 2, 1024, 1024, None, 64, seed=3), torch.bfloat16)[:3]
    go = grad_out_for(ops + (None, None), 3).to(dev, torch.bfloat16)
    leaves = [t.clone().requires_grad_() for t in ops]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with wf.token_attention_16bit_route("kernel"), wf.token_attention_16bit_backward_route("kernel"):
        out = wf.token_attention(*leaves)
    out.backward(go)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"[bound16-bwd] peak allocation of forward + backward above the operands: {peak / 1e6:.2f} MB")
    assert all(t.grad is not None for t in leaves)
    assert peak < 2e6, peak


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_other_switches(dev, dtype):
    """Under the new switch's default nothing changes: one ``waldo_token_attention_fwd_dt`` and the framework route's
    gradients; ``token_attention_backward_route("kernel")`` alone still does not reach 16-bit calls."""
    wf = WF()
    assert wf.get_token_attention_16bit_backward_route() == "framework"
    ops = to16(FWD.operands(dev, 2, 2, 70, 65, 37, 32, seed=37), dtype)
    go = grad_out_for(ops, 37).to(dev, dtype)
    leaves = [t.clone().requires_grad_() for t in ops]
    wf.token_attention_framework(*leaves).backward(go)
    want = [t.grad for t in leaves]
    _, got = run(ops, go, calls={"waldo_token_attention_fwd_dt": 1}, bwd_route="framework")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    with wf.token_attention_backward_route("kernel"):
        _, got = run(ops, go, calls={"waldo_token_attention_fwd_dt": 1}, bwd_route="framework")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # fp32 operands do not see the new switch
    f32 = FWD.operands(dev, 2, 2, 70, 65, 37, 32, seed=37)
    with wf.token_attention_16bit_route("kernel"), wf.token_attention_16bit_backward_route("kernel"):
        leaves = [t.clone().requires_grad_() for t in f32]
        _, made = launches(lambda: wf.token_attention(*leaves).backward(go.float()))
    assert made == {"waldo_token_attention_fwd": 1}, made
    # ... and neither does the default 16-bit route
    with wf.token_attention_16bit_backward_route("kernel"):
        leaves = [t.clone().requires_grad_() for t in ops]
        _, made = launches(lambda: wf.token_attention(*leaves).backward(go))
    assert made == {} and all(torch.equal(t.grad, w) for t, w in zip(leaves, want))


def test_lvd_step_in_bf16_under_the_switch(dev):
    from test_gpu_unet_16bit import rms
    from waldo_amd.tools.lvd_step import LvdStep
    wf = WF()

    def grads_of(act_dtype, route):
        with wf.token_attention_16bit_backward_route(route):
            step = LvdStep(2, dev, nets="reference", act_dtype=act_dtype)
            loss, calls = launches(step)
        assert torch.isfinite(loss).all()
        return calls, {n: p.grad for n, p in step.net.named_parameters() if p.grad is not None}

    calls, new = grads_of(torch.bfloat16, "kernel")
    assert calls.get("waldo_token_attention_fwd_lse_dt", 0) > 0 and calls.get("waldo_token_attention_bwd_dt", 0) > 0, calls
    assert calls["waldo_token_attention_bwd_dt"] == calls["waldo_token_attention_fwd_lse_dt"]
    assert "waldo_token_attention_bwd" not in calls and "waldo_token_attention_fwd" not in calls, calls
    assert len(new) > 10 and all(g.dtype == torch.float32 and bool(torch.isfinite(g).all()) for g in new.values())
    calls, old = grads_of(torch.bfloat16, "framework")
    assert "waldo_token_attention_bwd_dt" not in calls and "waldo_token_attention_fwd_lse_dt" not in calls, calls
    _, f32 = grads_of(None, "framework")
    assert set(new) == set(old) == set(f32)
    bad, worst = {}, (0.0, None)
    for n in f32:
        d_new, d_old = rms(new[n], f32[n]), rms(old[n], f32[n])
        ratio = d_new / d_old if d_old > 0 else (0.0 if d_new == 0 else float("inf"))
        worst = max(worst, (ratio, n))
        if not ratio <= 2.0:
            bad[n] = (d_new, d_old)
    print(f"[2x] LvdStep parameter gradients, kernel route against the default's distance from fp32: the largest ratio "
          f"{worst[0]:.3f} ({worst[1]})")
    assert not bad, bad
