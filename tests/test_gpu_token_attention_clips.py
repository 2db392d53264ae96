"""GPU: ``WF.token_attention_clips`` (waldo_token_attention_clips_fwd / _fwd_lse / _bwd: the token attention's kernels over
per-clip segments of packed rows) against ``WF.token_attention_clips_framework`` in fp32 and fp64 on the same operands,
through the suite's yardsticks: ``parity.close(out, r32, exact=r64)`` for outputs and, for gradients, the rule of
test_gpu_token_attention_bwd.py, ``close(got, r32, rel=True, exact=r64)``.  The operands are the slices of ONE packed
(R, 3 H D) projection, q's rows and the keys' rows at different places of it, and gradients are taken at that leaf so
that the three views' gradients meet.  Every case asserts that the KERNELS served it.

The clips of a case, as (queries, keys) with QT and KT the kernels' tiles: (1, KT+1), (QT+1, 1), (0, 5),
(QT-1, 2 KT+3) -- every clip but the first starts off a tile boundary, and the tail of a clip's last query block and of
its last key tile lies inside the NEXT clip's rows.  No test feeds a malformed table: what the kernels do with one is
read in their code (ta_segment)."""
import itertools

import pytest
import torch

from parity import close

pytestmark = pytest.mark.gpu

H = 2
Q_PAD, K_PAD = 3, 5       # the rows of the projection in front of q's and of the keys' rows: owned by no clip
FACTORS = (None, 0.37, -1.0)   # of D ** -0.5; None: the default scale


def WF():
    from waldo_amd import functional
    return functional


def tiles():
    lim, blim = WF().token_attention_limits(), WF().token_attention_bwd_limits()
    assert (lim["q_tile"], lim["k_tile"]) == (blim["q_tile"], blim["k_tile"]) == (64, 64)
    return lim["q_tile"], lim["k_tile"]


def clip_lengths(nan_clip=False):
    qt, kt = tiles()
    lens = [(1, kt + 1), (qt + 1, 1), (0, 5), (qt - 1, 2 * kt + 3)]
    if nan_clip:
        lens.insert(1, (3, 0))   # queries without keys
    return lens


def offsets(lens, dev):
    q = torch.tensor([0] + list(itertools.accumulate(n for n, _ in lens)), dtype=torch.int32)
    k = torch.tensor([0] + list(itertools.accumulate(n for _, n in lens)), dtype=torch.int32)
    return q.to(dev), k.to(dev)


def projection(lens, d, seed, planted=None):
    """The packed (R, 3, H, D) leaf on the CPU.  ``planted``: a clip WITHOUT queries, whose keys -- the rows right
    after the keys of the clip before it and right before those of the clip after it -- get a component 0 that scores
    +40, at the default scale, with the queries of those two clips (component 0 = 64; their own keys' is 0), and
    values of 1e3: one of them let into a neighbour's softmax takes it over.  The projection's rows in front of and
    behind the keys, which belong to no clip, carry the same.  (The planted keys are those of a clip without queries
    because an output of the order of 1e3 has an fp32 rounding error above the yardstick's absolute 1e-4.)"""
    rq, rk = sum(n for n, _ in lens), sum(n for _, n in lens)
    rows = max(Q_PAD + rq, K_PAD + rk) + 2
    p = torch.randn(rows, 3, H, d, generator=torch.Generator().manual_seed(seed)) * 1.2
    if planted is not None:
        qo, ko = offsets(lens, "cpu")
        assert lens[planted][0] == 0 and lens[planted][1] > 0 and 0 < planted < len(lens) - 1
        for b in (planted - 1, planted + 1):
            assert lens[b][0] > 0 and lens[b][1] > 0
            p[Q_PAD + qo[b]:Q_PAD + qo[b + 1], 0, :, 0] = 64.0
            p[K_PAD + ko[b]:K_PAD + ko[b + 1], 1, :, 0] = 0.0
        plant = torch.zeros(rows, dtype=torch.bool)
        plant[K_PAD + ko[planted]:K_PAD + ko[planted + 1]] = True
        plant[:K_PAD] = True
        plant[K_PAD + rk:] = True
        p[plant, 1, :, 0] = 40.0 / (d ** -0.5 * 64.0)
        p[plant, 2] = 1e3
    return p


def views(p, lens):
    rq, rk = sum(n for n, _ in lens), sum(n for _, n in lens)
    return p[Q_PAD:Q_PAD + rq, 0], p[K_PAD:K_PAD + rk, 1], p[K_PAD:K_PAD + rk, 2]


def launches(fn):
    from waldo_amd import _lib
    with _lib.KernelTimer() as timer:
        out = fn()
    return out, {k: len(v) for k, v in timer.pairs.items()}


def kernel(q, k, v, qo, ko, mq, mk, scale=None):
    assert WF()._token_attention_clips_served(q, k, v, qo, ko) is not None
    with WF().token_attention_backward_route("kernel"):
        return WF().token_attention_clips(q, k, v, qo, ko, mq, mk, scale)


def run(fn, p0, lens, go, dev, dtype=torch.float32, scale=None, backward=True):
    """(out, the gradient at the packed leaf) of ``fn`` on the three views of a fresh leaf."""
    qt, kt = tiles()
    p = p0.to(dev).to(dtype).requires_grad_(backward)
    qo, ko = offsets(lens, dev)
    q, k, v = views(p, lens)
    assert not q.is_contiguous() and q.stride(0) == 3 * H * p0.shape[3]
    out = fn(q, k, v, qo, ko, 3 * qt, 4 * kt, scale=scale)   # bounds well above every clip: some blocks leave at once
    if not backward:
        return out.detach(), None
    out.backward(go.to(dev).to(dtype))
    return out.detach(), p.grad


def check(dev, d, seed, scale=None, planted=None):
    lens = clip_lengths()
    p0 = projection(lens, d, seed, planted)
    rq = sum(n for n, _ in lens)
    go = torch.randn(rq, H * d, generator=torch.Generator().manual_seed(1000 + seed))
    got, calls = launches(lambda: run(kernel, p0, lens, go, dev, scale=scale))
    assert calls == {"waldo_token_attention_clips_fwd_lse": 1, "waldo_token_attention_clips_bwd": 1}, calls
    fw = WF().token_attention_clips_framework
    r32 = run(fw, p0, lens, go, dev, scale=scale)
    r64 = run(fw, p0, lens, go, dev, torch.float64, scale=scale)
    what = f"D={d} scale={scale} planted={planted}"
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
    close(got[0], r32[0], exact=r64[0], what=f"{what} out")
    for i, name in enumerate(("q", "k", "v")):
        close(got[1][:, i], r32[1][:, i], rel=True, exact=r64[1][:, i], what=f"{what} grad {name}")
    # placement: nothing outside the three views, and exact zeros for the keys and values of the clip without queries
    qo, ko = offsets(lens, "cpu")
    rk = int(ko[-1])
    g = got[1].cpu()
    assert not g[:Q_PAD, 0].any() and not g[Q_PAD + rq:, 0].any()
    assert not g[:K_PAD, 1:].any() and not g[K_PAD + rk:, 1:].any()
    empty = [b for b, (nq, nk) in enumerate(lens) if nq == 0 and nk > 0]
    assert empty
    for b in empty:
        assert torch.count_nonzero(g[K_PAD + ko[b]:K_PAD + ko[b + 1], 1:]) == 0
    # the plain forward (no gradient wanted: no row statistics) has the same bits, and so has a second run
    with torch.no_grad():
        plain, calls = launches(lambda: run(kernel, p0, lens, go, dev, scale=scale, backward=False))
    assert calls == {"waldo_token_attention_clips_fwd": 1}, calls
    assert torch.equal(plain[0], got[0])
    again = run(kernel, p0, lens, go, dev, scale=scale)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    return got, r64


@pytest.mark.parametrize("f", FACTORS)
@pytest.mark.parametrize("d", [16, 32, 64])
def test_clips_forward_and_backward(dev, d, f):
    scale = None if f is None else f * d ** -0.5
    check(dev, d, seed=3 * d + FACTORS.index(f), scale=scale)
    if f is not None:   # the scale that was passed is the one that was used
        lens = clip_lengths()
        p0 = projection(lens, d, 3 * d + FACTORS.index(f))
        a = run(kernel, p0, lens, None, dev, scale=scale, backward=False)[0]
        b = run(kernel, p0, lens, None, dev, backward=False)[0]
        assert (a - b).abs().max().item() > 1e-2


@pytest.mark.parametrize("d", [16, 32, 64])
def test_a_leaked_key_of_a_neighbouring_clip_would_show(dev, d):
    """The five keys of clip 2, which has no queries, score +40 with the queries of clip 1 (QT+1 queries, one key: the
    planted rows are the rest of its only key tile) and of clip 3 (they lie right before its first key), and carry
    values of 1e3.  Both clips' outputs and gradients stay within the yardstick, and clip 1's output is its one value
    row, exactly."""
    lens = clip_lengths()
    got, _ = check(dev, d, seed=77 + d, planted=2)
    p0 = projection(lens, d, 77 + d, planted=2)
    qo, ko = offsets(lens, "cpu")
    own = p0[K_PAD + ko[1], 2].reshape(1, H * d).to(dev)
    rows = got[0][qo[1]:qo[2]]
    assert torch.equal(rows, own.expand_as(rows))
    assert got[0].abs().max().item() < 10
    # the plant is live: with clip 2's keys let in, the framework's output of either clip's rows is near 1e3
    q, k, v = (t.to(dev) for t in views(p0, lens))
    for b, keys in ((1, slice(int(ko[1]), int(ko[3]))), (3, slice(int(ko[2]), int(ko[4])))):
        s = torch.einsum("ihd,jhd->hij", q[qo[b]:qo[b + 1]], k[keys]) * d ** -0.5
        assert s.max().item() > 35
        leaked = torch.einsum("hij,jhd->ihd", s.softmax(-1), v[keys])
        assert leaked.abs().min().item() > 900


@pytest.mark.parametrize("d", [16, 64])
def test_queries_without_keys_are_nan_in_exactly_their_rows(dev, d):
    lens = clip_lengths(nan_clip=True)
    p0 = projection(lens, d, seed=5 + d)
    got, calls = launches(lambda: run(kernel, p0, lens, None, dev, backward=False))
    assert calls == {"waldo_token_attention_clips_fwd": 1}, calls
    fw = WF().token_attention_clips_framework
    r32 = run(fw, p0, lens, None, dev, backward=False)[0]
    r64 = run(fw, p0, lens, None, dev, torch.float64, backward=False)[0]
    qo, _ = offsets(lens, "cpu")
    expect = torch.zeros_like(r32, dtype=torch.bool)
    expect[qo[1]:qo[2]] = True
    assert int(expect.sum()) == 3 * H * d
    assert torch.equal(torch.isnan(r32), expect) and torch.equal(torch.isnan(got[0]), expect)
    zero = lambda t: torch.where(expect.to(t.device), torch.zeros_like(t), t)
    close(zero(got[0]), zero(r32), exact=zero(r64), what=f"D={d}: the rows of the other clips")
    # ... and the other clips' gradients do not see that clip: the bits of the run on the layout without it
    rq = int(qo[-1])
    go = torch.randn(rq, H * d, generator=torch.Generator().manual_seed(9))
    with_nan = run(kernel, p0, lens, go, dev)
    keep = torch.ones(rq, dtype=torch.bool)
    keep[qo[1]:qo[2]] = False
    lens0 = clip_lengths()
    p1 = torch.cat([p0[:Q_PAD], p0[Q_PAD:Q_PAD + rq][keep], p0[Q_PAD + rq:], p0[:3]])
    p1[:, 1:] = p0[:, 1:]     # (the keys' rows stay where they are: the clip has none)
    without = run(kernel, p1, lens0, go[keep], dev)
    assert torch.equal(with_nan[0][keep.to(dev)], without[0])
    assert torch.equal(with_nan[1][:, 1:], without[1][:, 1:])
    gq = with_nan[1][Q_PAD:Q_PAD + rq, 0]
    assert torch.equal(gq[keep.to(dev)], without[1][Q_PAD:Q_PAD + rq - 3, 0])
    assert torch.isfinite(gq[keep.to(dev)]).all()


def test_only_the_wanted_gradients(dev):
    lens = clip_lengths()
    qt, kt = tiles()
    p0 = projection(lens, 32, seed=21).to(dev)
    qo, ko = offsets(lens, dev)
    go = torch.randn(int(qo[-1]), H * 32, generator=torch.Generator().manual_seed(22)).to(dev)
    full = [t.detach().clone().requires_grad_() for t in views(p0, lens)]
    kernel(*full, qo, ko, 2 * qt, 3 * kt).backward(go)
    for wanted in (("q",), ("v",), ("k", "v")):
        some = [t.detach().clone().requires_grad_(n in wanted) for t, n in zip(views(p0, lens), "qkv")]
        out = kernel(*some, qo, ko, 2 * qt, 3 * kt)
        _, calls = launches(lambda: out.backward(go))
        assert calls == {"waldo_token_attention_clips_bwd": 1}, calls
        for t, f, n in zip(some, full, "qkv"):
            assert (t.grad is None) if n not in wanted else torch.equal(t.grad, f.grad), n


def test_the_framework_route_of_the_backward(dev):
    lens = clip_lengths()
    qt, kt = tiles()
    p0 = projection(lens, 16, seed=31).to(dev)
    qo, ko = offsets(lens, dev)
    go = torch.randn(int(qo[-1]), H * 16, generator=torch.Generator().manual_seed(32)).to(dev)
    leaves = [t.detach().clone().requires_grad_() for t in views(p0, lens)]
    with WF().token_attention_backward_route("framework"):
        out, calls = launches(lambda: WF().token_attention_clips(*leaves, qo, ko, 2 * qt, 3 * kt))
    assert calls == {"waldo_token_attention_clips_fwd": 1}, calls
    _, calls = launches(lambda: out.backward(go))
    assert "waldo_token_attention_clips_bwd" not in calls, calls
    hand = [t.detach().clone().requires_grad_() for t in views(p0, lens)]
    want = torch.autograd.grad(WF().token_attention_clips_framework(*hand, qo, ko, 2 * qt, 3 * kt), hand, go)
    for t, w in zip(leaves, want):
        assert torch.equal(t.grad, w)


def test_forward_and_backward_replay_from_one_graph_with_the_eager_bits(dev):
    """The capture is the proof that nothing reads the tables on the host; the replay reads them anew."""
    lens = clip_lengths()
    qt, kt = tiles()
    d = 64
    p0 = projection(lens, d, seed=41).to(dev)
    qo, ko = offsets(lens, dev)
    go = torch.randn(int(qo[-1]), H * d, generator=torch.Generator().manual_seed(42)).to(dev)

    def step(p):
        q, k, v = views(p, lens)
        out = kernel(q, k, v, qo, ko, 2 * qt, 3 * kt)
        return (out, *torch.autograd.grad(out, [p], go))

    eager = [t.detach().clone() for t in step(p0.clone().requires_grad_())]
    static_p = p0.clone().requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # (warm-up off the default stream, as capture asks for)
        step(static_p)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step(static_p)
    with torch.no_grad():
        static_p.zero_()
    graph.replay()
    zeros = static[0].detach().clone()
    with torch.no_grad():
        static_p.copy_(p0)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(static, eager):
        assert torch.equal(got.detach(), want)
    assert not torch.equal(zeros, eager[0])
