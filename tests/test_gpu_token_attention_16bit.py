"""GPU: the 16-bit token attention (waldo_token_attention_fwd_dt / _clips_fwd_dt, csrc/token_attention_16.hip) under
``WF.token_attention_16bit_route("kernel")``, in bf16 and fp16, against the bound of tests/token_attention_16bit.py:

    |out - exact| <= u (A + |exact|) + TOL max(1, A)

with exact = ``token_attention_framework`` in fp64 on the 16-bit operands widened and A the same with |v| -- derived
from the kernel's arithmetic contract there, and shown on the CPU (test_token_attention_16bit_cpu.py) to refuse the
framework's own 16-bit chain and five planted faults.  The operand recipes are test_gpu_token_attention.py's; every
call asserts that the 16-bit predicate served it."""
import itertools

import pytest
import torch

import test_gpu_token_attention as FWD
from token_attention_16bit import DTYPES, bound_ratio, to16, within_bound

pytestmark = pytest.mark.gpu


def WF():
    from waldo_amd import functional
    return functional


def launches(fn):
    from waldo_amd import _lib
    with _lib.KernelTimer() as timer:
        out = fn()
    return out, {k: len(v) for k, v in timer.pairs.items()}


def served(q, k, v, k2=None, v2=None, scale=None):
    """WF.token_attention under the "kernel" route, after making sure that the 16-bit kernel serves the call."""
    with WF().token_attention_16bit_route("kernel"):
        assert WF()._token_attention_served(q, k, v, k2, v2) is None
        assert WF()._token_attention_served_16bit(q, k, v, k2, v2) is not None
        return WF().token_attention(q, k, v, k2, v2, scale)


def kernel(*ops, **kw):
    """``served``, and the one launch it made was the 16-bit entry point's."""
    out, calls = launches(lambda: served(*ops, **kw))
    assert calls == {"waldo_token_attention_fwd_dt": 1}, calls
    return out


def check(ops, what, scale=None):
    return within_bound(WF().token_attention_framework, kernel(*ops, scale=scale), ops, scale, what)


def tiles():
    lim = WF().token_attention_16bit_limits()
    assert lim == WF().token_attention_limits()
    return lim["q_tile"], lim["k_tile"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_default_route_is_unchanged(dev, dtype):
    """Nothing switched on: 16-bit operands ARE ``token_attention_framework``, bit for bit, with or without autocast,
    and the 16-bit predicate says so."""
    wf = WF()
    assert wf.get_token_attention_16bit_route() == "framework"
    ops = to16(FWD.operands(dev, 2, 2, 65, 70, 9, 32, seed=41), dtype)
    assert wf._token_attention_served_16bit(*ops) is None and wf._token_attention_served(*ops) is None
    out, calls = launches(lambda: wf.token_attention(*ops))
    assert calls == {} and out.dtype == dtype and torch.equal(out, wf.token_attention_framework(*ops))
    with torch.autocast("cuda", dtype=dtype):
        out, calls = launches(lambda: wf.token_attention(*ops))
        assert calls == {} and torch.equal(out, wf.token_attention_framework(*ops))
    # fp32 operands do not see the switch: the fp32 kernel outside autocast, the framework route inside, as ever
    f32 = FWD.operands(dev, 2, 2, 65, 70, 9, 32, seed=41)
    plain = wf.token_attention(*f32)
    with wf.token_attention_16bit_route("kernel"):
        assert wf._token_attention_served_16bit(*f32) is None
        out, calls = launches(lambda: wf.token_attention(*f32))
        assert calls == {"waldo_token_attention_fwd": 1} and torch.equal(out, plain)
        with torch.autocast("cuda", dtype=dtype):
            out, calls = launches(lambda: wf.token_attention(*f32))
            assert calls == {} and torch.equal(out, wf.token_attention_framework(*f32))
            # ... and 16-bit operands are served inside autocast
            assert wf._token_attention_served_16bit(*ops) is not None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [16, 32, 64])
def test_tile_edges(dev, d, dtype):
    qt, kt = tiles()
    worst = 0.0
    for b, h, nq, nk1, nk2, d, seed in FWD.tile_edge_cases(qt, kt, d):
        worst = max(worst, check(to16(FWD.operands(dev, b, h, nq, nk1, nk2, d, seed), dtype),
                                 f"D={d} Nq={nq} Nk1={nk1} Nk2={nk2}"))
    print(f"[bound16] tile edges D={d} {dtype}: worst {worst:.3g} x its bound")


@pytest.mark.parametrize("dtype", DTYPES)
def test_scales_that_are_not_the_default(dev, dtype):
    for shape, scale in FWD.scale_cases(*tiles()):
        ops = FWD.operands(dev, *shape[:6], seed=shape[6])
        FWD.scale_moves_the_output(ops, scale)
        check(to16(ops, dtype), f"D={shape[5]} scale={scale:.3g}", scale=scale)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("low_rows", FWD.LARGE_SCORE_CASES)
def test_large_scores_and_the_online_rescale(dev, low_rows, dtype):
    check(to16(FWD.large_score_operands(dev, tiles()[1], low_rows), dtype), f"scores up to +-60, low rows {low_rows}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_many_heads_query_blocks_and_the_network_shapes(dev, dtype):
    qt = tiles()[0]
    check(to16(FWD.operands(dev, 3, 8, 2 * qt + 5, 70, 9, 32, seed=3), dtype), "B H = 24, three query blocks")
    for shape in ((2, 2, 20, 20, 32, 16), (10, 1, 28, 28, None, 64), (2, 8, 384, 384, 512, 64)):
        check(to16(FWD.operands(dev, *shape, seed=7), dtype), f"{shape}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [16, 32, 64])
def test_one_key_gives_the_bits_of_its_value(dev, d, dtype):
    for nq in (1, 17, 65):
        q, k, v, _, _ = to16(FWD.operands(dev, 2, 2, nq, 1, None, d, seed=3), dtype)
        assert torch.equal(kernel(q, k, v), v.reshape(2, 1, 2 * d).expand(2, nq, 2 * d))


@pytest.mark.parametrize("dtype", DTYPES)
def test_equal_scores_give_the_mean(dev, dtype):
    kt = tiles()[1]
    q, k, v, k2, v2 = to16(FWD.operands(dev, 2, 2, 19, kt + 3, kt - 5, 32, seed=19), dtype)
    ops = (torch.zeros_like(q), k, v, k2, v2)
    check(ops, "q = 0")
    out = kernel(*ops)
    mean = torch.cat([v, v2], 1).double().mean(1).reshape(2, 1, 64).expand(2, 19, 64)
    # (the bound against the mean itself: exact IS the mean when every score is 0)
    a = torch.cat([v, v2], 1).double().abs().mean(1).reshape(2, 1, 64).expand(2, 19, 64)
    assert bound_ratio(out, mean, a)[0] <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_operands_are_read_where_they_lie(dev, dtype):
    """The slices of a packed (B, N, 3 H D) projection that is itself a slice of a longer tensor, a second segment with
    strides of its own, a broadcast batch: the bits of the call on contiguous copies."""
    b, n, m, h, d = 3, 70, 37, 2, 32
    g = torch.Generator().manual_seed(11)
    big = torch.randn(b, n + 5, 3 * h * d, generator=g).to(dev, dtype)
    qkv = big[:, 2:n + 2].view(b, n, 3, h, d)
    kv = torch.randn(b, m + 3, 2 * h * d, generator=g).to(dev, dtype)[:, 3:].view(b, m, 2, h, d)
    q, k, v = qkv.unbind(2)
    k2, v2 = kv.unbind(2)
    assert not q.is_contiguous() and q.stride(0) != n * q.stride(1) and k2.stride(0) != m * k2.stride(1)
    for ops in ((q, k, v, None, None), (q, k, v, k2, v2)):
        out = kernel(*ops)
        within_bound(WF().token_attention_framework, out, ops, what="packed views")
        assert torch.equal(out, kernel(*(None if t is None else t.contiguous() for t in ops)))
    ke, ve = k[:1].expand(b, -1, -1, -1), v[:1].expand(b, -1, -1, -1)
    assert ke.stride(0) == 0
    assert torch.equal(kernel(q, ke, ve), kernel(q, ke.contiguous(), ve.contiguous()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_stays_where_the_arithmetic_puts_it(dev, dtype):
    ops = to16(FWD.operands(dev, 2, 2, 70, 65, 9, 32, seed=43), dtype)
    clean = kernel(*ops)
    assert torch.isfinite(clean).all()
    # one NaN in q[0, 7, head 1]: that row of that head, nothing else
    bad = [None if t is None else t.clone() for t in ops]
    bad[0][0, 7, 1, 3] = float("nan")
    out = kernel(*bad).view(2, 70, 2, 32)
    hit = torch.zeros(2, 70, 2, 32, dtype=torch.bool, device=dev)
    hit[0, 7, 1] = True
    assert torch.equal(torch.isnan(out), hit) and torch.equal(out[~hit], clean.view(2, 70, 2, 32)[~hit])
    # one NaN in a value of the second segment, v2[1, 4, head 0, 5]: every query of (1, head 0) weighs that key, so
    # column 5 of their outputs is NaN; no other column, head or batch element sees it
    bad = [None if t is None else t.clone() for t in ops]
    bad[4][1, 4, 0, 5] = float("nan")
    weight = torch.softmax(torch.einsum("ihd,jhd->hij", ops[0][1].double(), torch.cat([ops[1][1], ops[3][1]]).double())
                           * 32 ** -0.5, -1)[0, :, 65 + 4]
    assert weight.min() > 1e-30   # (from the reference alone: the key has weight in every row)
    out = kernel(*bad).view(2, 70, 2, 32)
    hit.zero_()
    hit[1, :, 0, 5] = True
    assert torch.equal(torch.isnan(out), hit) and torch.equal(out[~hit], clean.view(2, 70, 2, 32)[~hit])


@pytest.mark.parametrize("dtype", DTYPES)
def test_same_bits_from_run_to_run_and_in_a_graph_replay(dev, dtype):
    ops = to16(FWD.operands(dev, 2, 4, 70, 65, 9, 64, seed=31), dtype)
    with torch.no_grad():
        eager = kernel(*ops).clone()
        assert torch.equal(kernel(*ops), eager)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # (warm-up off the default stream, as capture asks for)
            kernel(*ops)
        torch.cuda.current_stream().wait_stream(side)
        static_q = ops[0].clone()
        graph = torch.cuda.CUDAGraph()
        with WF().token_attention_16bit_route("kernel"), torch.cuda.graph(graph):
            static_out = WF().token_attention(static_q, *ops[1:])
        static_q.zero_()
        graph.replay()
        zeros = static_out.clone()
        static_q.copy_(ops[0])
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(static_out, eager)
    assert not torch.equal(zeros, eager)   # the replay read its input anew


@pytest.mark.parametrize("dtype", DTYPES)
def test_what_the_kernel_does_not_serve_takes_the_framework_route(dev, dtype):
    wf = WF()
    g = torch.Generator().manual_seed(13)
    w = torch.randn(2, 9, 2, 96, generator=g).to(dev, dtype)
    with wf.token_attention_16bit_route("kernel"):
        for q, k in ((w[..., :48], w[..., 48:]),                       # D = 48
                     (w[..., ::2][..., :32], w[..., 1::2][..., :32]),  # a non-unit inner stride
                     (w[..., 4:36], w[..., 36:68]),                    # rows off the 16-byte boundaries (8 bytes)
                     (w[..., :32], w[..., 32:64].float()),             # mixed dtypes
                     (w[..., :32], w[..., 32:64].to(torch.float16 if dtype is torch.bfloat16 else torch.bfloat16))):
            assert wf._token_attention_served_16bit(q, k, k, None, None) is None
            if q.dtype == k.dtype:
                out, calls = launches(lambda: wf.token_attention(q, k, k))
                assert calls == {} and torch.equal(out, wf.token_attention_framework(q, k, k))


# ---------------------------------------------------------------------------------------------------------------------
# clips
# ---------------------------------------------------------------------------------------------------------------------
def clip_lengths():
    """(queries, keys): a full tile of queries, an EMPTY clip, a clip of one row past a tile with exactly one tile of
    keys, queries WITHOUT keys, one query over two tiles and a tail."""
    qt, kt = tiles()
    return [(qt, kt + 1), (0, 0), (qt + 1, kt), (3, 0), (1, 2 * kt + 3)]


def clips_served(q, k, v, qo, ko, mq, mk, scale=None):
    with WF().token_attention_16bit_route("kernel"):
        assert WF()._token_attention_clips_served(q, k, v, qo, ko) is None
        assert WF()._token_attention_clips_served_16bit(q, k, v, qo, ko) is not None
        return WF().token_attention_clips(q, k, v, qo, ko, mq, mk, scale)


def clips_kernel(*args, **kw):
    out, calls = launches(lambda: clips_served(*args, **kw))
    assert calls == {"waldo_token_attention_clips_fwd_dt": 1}, calls
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [16, 64])
def test_clips_are_the_dense_call_clip_by_clip(dev, d, dtype):
    qt, kt = tiles()
    lens, h = clip_lengths(), 2
    rq, rk = sum(n for n, _ in lens), sum(n for _, n in lens)
    qo = torch.tensor([0] + list(itertools.accumulate(n for n, _ in lens)), dtype=torch.int32, device=dev)
    ko = torch.tensor([0] + list(itertools.accumulate(n for _, n in lens)), dtype=torch.int32, device=dev)
    p = (torch.randn(max(rq, rk) + 8, 3, h, d, generator=torch.Generator().manual_seed(47)) * 1.2).to(dev, dtype)
    q, k, v = p[3:3 + rq, 0], p[5:5 + rk, 1], p[5:5 + rk, 2]   # the slices of one packed projection, off its first row
    assert not q.is_contiguous()
    out = clips_kernel(q, k, v, qo, ko, 3 * qt, 4 * kt)
    assert out.shape == (rq, h * d) and out.dtype == dtype
    again = clips_kernel(q, k, v, qo, ko, 3 * qt, 4 * kt)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16))   # (the bits: the rows without keys are NaN)
    for b, (nq, nk) in enumerate(lens):
        rows = out[int(qo[b]):int(qo[b + 1])]
        if nq and not nk:
            assert torch.isnan(rows).all()   # the softmax of rows whose keys are all masked
        elif nq:
            ops = tuple(t[int(o[b]):int(o[b + 1])].unsqueeze(0) for t, o in ((q, qo), (k, ko), (v, ko)))
            assert torch.equal(rows, kernel(*ops)[0]), (b, nq, nk)
            within_bound(WF().token_attention_framework, rows.unsqueeze(0).contiguous(), ops + (None, None),
                         what=f"clip {b}: {nq} x {nk}")
    assert torch.isnan(out).sum().item() == 3 * h * d


# ---------------------------------------------------------------------------------------------------------------------
# gradients
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_gradients_are_the_framework_routes_whatever_the_backward_switch_says(dev, dtype):
    wf = WF()
    b, n, m, h, d = 2, 70, 37, 2, 32
    g = torch.Generator().manual_seed(37)
    qkv0 = (torch.randn(b, n, 3, h, d, generator=g) * 1.4).to(dev, dtype)
    kv0 = (torch.randn(b, m, 2, h, d, generator=g) * 1.4).to(dev, dtype)
    go = torch.randn(b, n, h * d, generator=g).to(dev, dtype)

    def run(fn):
        qkv, kv = qkv0.clone().requires_grad_(), kv0.clone().requires_grad_()
        out = fn(*qkv.unbind(2), *kv.unbind(2))
        out.backward(go)
        return out.detach(), qkv.grad, kv.grad

    want = run(wf.token_attention_framework)
    for route in wf.TOKEN_ATTENTION_BACKWARD_ROUTES:
        with wf.token_attention_backward_route(route):
            (out, gqkv, gkv), calls = launches(lambda: run(served))
        assert calls == {"waldo_token_attention_fwd_dt": 1}, calls   # no fp32 kernel, forward or backward
        assert gqkv.dtype == dtype and gkv.dtype == dtype
        assert torch.equal(gqkv, want[1]) and torch.equal(gkv, want[2]), route
        within_bound(wf.token_attention_framework, out, (*qkv0.unbind(2), *kv0.unbind(2)), what="out of the node")

    # the per-clip form: one clip is the dense call
    qo = torch.tensor([0, n], dtype=torch.int32, device=dev)

    def run_clips(fn):
        qkv = qkv0[0].clone().requires_grad_()
        fn(*qkv.unbind(1), qo, qo, n, n).backward(go[0])
        return qkv.grad

    with wf.token_attention_backward_route("kernel"):
        got, calls = launches(lambda: run_clips(clips_served))
    assert calls == {"waldo_token_attention_clips_fwd_dt": 1}, calls
    assert got.dtype == dtype and torch.equal(got, run_clips(wf.token_attention_clips_framework))
