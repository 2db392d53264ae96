"""GPU: ``WF.token_attention`` (waldo_token_attention_fwd, csrc/token_attention.hip) against the reference's sequence of
ops (``WF.token_attention_framework``) on the same operands in fp32 (``r32``) and fp64 (``r64``), through
``parity.close(out, r32, exact=r64)``: 1e-4 plus twice the fp32 reference's own distance from fp64, per element.  The
shapes sit on the kernel's tile edges (``WF.token_attention_limits()``); every call asserts that the KERNEL served it."""
import pytest
import torch

from parity import TOL, close

pytestmark = pytest.mark.gpu


def WF():
    from waldo_amd import functional
    return functional


def kernel(q, k, v, k2=None, v2=None, scale=None):
    """WF.token_attention, after making sure that the call is one the kernel serves (no framework route in disguise)."""
    assert WF()._token_attention_served(q, k, v, k2, v2) is not None
    return WF().token_attention(q, k, v, k2, v2, scale)


def refs(q, k, v, k2=None, v2=None, scale=None):
    fw = WF().token_attention_framework
    ops = (q, k, v) if k2 is None else (q, k, v, k2, v2)
    return fw(*ops, scale=scale), fw(*(t.double() for t in ops), scale=scale)


def operands(dev, b, h, nq, nk1, nk2, d, seed=0, amp=1.4):
    """q, k, v[, k2, v2] as (B, N, H, D) tensors with logits of standard deviation amp^2 (D ** -0.5 scale)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    mk = lambda n, a: (torch.randn(b, n, h, d, generator=g) * a).to(dev)
    q, k, v = mk(nq, amp), mk(nk1, amp), mk(nk1, 1.0)
    if nk2 is None:
        return q, k, v, None, None
    return q, k, v, mk(nk2, amp), mk(nk2, 1.0)


def check(ops, what, scale=None, fn=None):
    """``fn``: the candidate, the kernel unless a restatement is judged by the same yardstick
    (test_token_attention_sensitivity_cpu.py)."""
    out = (fn or kernel)(*ops, scale=scale)
    r32, r64 = refs(*ops, scale=scale)
    assert out.shape == r32.shape and out.is_contiguous()
    close(out, r32, exact=r64, what=what)
    return out


# The operand recipes of the families that test_token_attention_sensitivity_cpu.py replays on a tile-by-tile
# restatement with planted faults: plain lists, one list for both sides.
def tile_edge_cases(qt, kt, d):
    """(b, h, nq, nk1, nk2, d, seed): every combination of Nq in {1, QT-1, QT, QT+1}, Nk1 in {1, KT-1, KT, KT+1,
    2 KT+3} and Nk2 in {absent, 1, KT+1}."""
    grid = [(nq, nk1, nk2) for nq in (1, qt - 1, qt, qt + 1) for nk1 in (1, kt - 1, kt, kt + 1, 2 * kt + 3)
            for nk2 in (None, 1, kt + 1)]
    return [(1, 2, nq, nk1, nk2, d, i + 1) for i, (nq, nk1, nk2) in enumerate(grid)]


SCALE_FACTORS = (0.0, -1.0, 0.37, 2.5)   # of D ** -0.5: uniform weights, a negative scale, a smaller and a larger one


def scale_cases(qt, kt):
    """((b, h, nq, nk1, nk2, d, seed), scale): a query tail, a key tail and a seam inside the last tile, at scales
    away from the default."""
    return [((1, 2, qt + 1, kt + 1, 9, d, 5), f * d ** -0.5) for d in (16, 32, 64) for f in SCALE_FACTORS]


LARGE_SCORE_CASES = (False, True)   # low_rows of large_score_operands


def large_score_operands(dev, kt, low_rows=False):
    """Scores from below -60 to above +60; the running maximum of every row rises in the first tile (a planted 40), in
    the second segment (45), in the last tile (58) and once more at the very last key (60): every tile rescales.
    ``low_rows``: component 1 then moves EVERY score of the first and of the last query row down by 160, so that their
    row statistic lse is near -100 and exp(-lse) beyond fp32 -- the softmax of those rows is what it was."""
    b, h, nq, nk1, nk2, d = 2, 2, 70, kt + 7, 2 * kt + 5, 64
    q, k, v, k2, v2 = operands(dev, b, h, nq, nk1, nk2, d, seed=17)            # logits of std ~ 2
    q[..., 0], k[..., 0], k2[..., 0] = 8.0, 0.0, 0.0                           # component 0 carries the planted scores
    plant = lambda score: score / (d ** -0.5 * 8.0)
    k[:, 0, :, 0] = plant(-60.0)
    k[:, 5, :, 0] = plant(40.0)
    k2[:, 3, :, 0] = plant(45.0)
    k2[:, nk2 - 9, :, 0] = plant(58.0)      # in the last tile
    k2[:, nk2 - 1, :, 0] = plant(60.0)      # the last key of all
    scores = torch.einsum("bihd,bjhd->bhij", q.double(), torch.cat([k, k2], 1).double()) * d ** -0.5
    assert scores.max() > 60 and scores.min() < -60 and scores[..., nk1 + 3].min() > 35
    assert (scores.argmax(-1) >= nk1 + nk2 - 9).all()
    if low_rows:
        q[..., 1], k[..., 1], k2[..., 1] = 0.0, 1.0, 1.0
        q[:, 0, :, 1] = q[:, nq - 1, :, 1] = -160.0 / d ** -0.5
        scores = torch.einsum("bihd,bjhd->bhij", q.double(), torch.cat([k, k2], 1).double()) * d ** -0.5
        lse = torch.logsumexp(scores, -1)
        assert lse[..., 0].max() < -95 and lse[..., nq - 1].max() < -95 and lse[..., 1:nq - 1].min() > 50
    return q, k, v, k2, v2


def scale_moves_the_output(ops, scale):
    """From the reference alone: the fp32 framework output at ``scale`` is more than 100 TOL from the one at the
    default scale, so a kernel that ignored the argument cannot pass."""
    moved = (refs(*ops, scale=scale)[0] - refs(*ops)[0]).abs().max().item()
    assert moved > 100 * TOL, moved


@pytest.mark.parametrize("d", [16, 32, 64])
def test_tile_edges(dev, d):
    """Every combination of Nq in {1, QT-1, QT, QT+1}, Nk1 in {1, KT-1, KT, KT+1, 2 KT+3} and Nk2 in {absent, 1, KT+1}:
    key tails, a seam inside a tile, a seam on a tile boundary, a second segment that is all of the last tile."""
    lim = WF().token_attention_limits()
    assert d in lim["head_dims"]
    for b, h, nq, nk1, nk2, d, seed in tile_edge_cases(lim["q_tile"], lim["k_tile"], d):
        check(operands(dev, b, h, nq, nk1, nk2, d, seed), f"D={d} Nq={nq} Nk1={nk1} Nk2={nk2}")


@pytest.mark.parametrize("d", [16, 32, 64])
@pytest.mark.parametrize("f", SCALE_FACTORS)
def test_a_scale_that_is_not_the_default(dev, d, f):
    """f = 0 pins uniform weights, f = -1 that nothing assumes a positive scale."""
    lim = WF().token_attention_limits()
    (shape, scale), = [c for c in scale_cases(lim["q_tile"], lim["k_tile"]) if c[0][5] == d and c[1] == f * d ** -0.5]
    ops = operands(dev, *shape[:6], seed=shape[6])
    scale_moves_the_output(ops, scale)
    check(ops, f"D={d} scale={f} D^-1/2", scale=scale)


def test_many_heads_and_query_blocks(dev):
    qt = WF().token_attention_limits()["q_tile"]
    check(operands(dev, 3, 8, 2 * qt + 5, 70, 9, 32, seed=3), "B H = 24, three query blocks")
    check(operands(dev, 24, 1, qt + 1, 33, None, 16, seed=4), "B = 24, H = 1")


@pytest.mark.parametrize("shape", [(2, 2, 20, 20, 32, 16), (10, 2, 28, 28, None, 16), (2, 1, 20, 20, 32, 64),
                                   (10, 1, 28, 28, None, 64)])
def test_the_fixture_networks_shapes(dev, shape):
    b, h, nq, nk1, nk2, d = shape
    check(operands(dev, b, h, nq, nk1, nk2, d, seed=7), f"{shape}")


def test_packed_projections_are_read_in_place(dev):
    """q, k, v as the three slices of one (B, N, 3 H D) tensor, k2, v2 as the two of a (B, M, 2 H D) one, and the
    packed tensor itself a slice of a longer one (a batch stride that is not N times the token stride): the bits of
    the call on contiguous copies."""
    b, n, m, h, d = 3, 70, 37, 2, 32
    g = torch.Generator().manual_seed(11)
    big = torch.randn(b, n + 5, 3 * h * d, generator=g).to(dev)
    qkv = big[:, 2:n + 2].view(b, n, 3, h, d)
    kv = torch.randn(b, m + 3, 2 * h * d, generator=g).to(dev)[:, 3:].view(b, m, 2, h, d)
    q, k, v = qkv.unbind(2)
    k2, v2 = kv.unbind(2)
    assert not q.is_contiguous() and q.stride(0) != n * q.stride(1) and k2.stride(0) != m * k2.stride(1)
    for ops in ((q, k, v, None, None), (q, k, v, k2, v2)):
        out = check(ops, "packed views")
        copies = tuple(None if t is None else t.contiguous() for t in ops)
        assert torch.equal(out, kernel(*copies))
    # a batch of broadcast keys: batch stride 0
    ke, ve = k[:1].expand(b, -1, -1, -1), v[:1].expand(b, -1, -1, -1)
    assert torch.equal(kernel(q, ke, ve), kernel(q, ke.contiguous(), ve.contiguous()))


def test_what_the_kernel_does_not_serve_takes_the_framework_route(dev):
    fw, served = WF().token_attention_framework, WF()._token_attention_served
    g = torch.Generator().manual_seed(13)
    w = torch.randn(2, 9, 2, 96, generator=g).to(dev)
    for q, k in ((w[..., :48], w[..., 48:]),                       # D = 48
                 (w[..., ::2][..., :32], w[..., 1::2][..., :32]),  # a non-unit inner stride
                 (w[..., 1:33], w[..., 33:65]),                    # rows off the 16-byte boundaries
                 (w[..., :32].bfloat16(), w[..., 32:64].bfloat16())):
        assert served(q, k, k, None, None) is None
        assert torch.equal(WF().token_attention(q, k, k), fw(q, k, k))


def test_large_scores_and_the_online_rescale(dev):
    """The operands of large_score_operands: scores from below -60 to above +60, the row maximum rising in every
    tile."""
    kt = WF().token_attention_limits()["k_tile"]
    check(large_score_operands(dev, kt), "scores up to +-60")


def test_large_scores_with_two_rows_far_below_zero(dev):
    kt = WF().token_attention_limits()["k_tile"]
    check(large_score_operands(dev, kt, low_rows=True), "scores up to +-60, two rows 160 lower")


def test_equal_scores_give_the_mean_and_a_far_ahead_key_gives_its_row(dev):
    kt = WF().token_attention_limits()["k_tile"]
    b, h, nq, nk1, nk2, d = 2, 2, 19, kt + 3, kt - 5, 32
    q, k, v, k2, v2 = operands(dev, b, h, nq, nk1, nk2, d, seed=19)
    mean = torch.cat([v, v2], 1).double().mean(1).reshape(b, 1, h * d).expand(b, nq, h * d)
    out = kernel(torch.zeros_like(q), k, v, k2, v2)
    # n = 122 values of order 1 summed in fp32 and divided: a few ulp of the partial sums, far below 1e-5
    assert (out.double() - mean).abs().max().item() < 1e-5
    # one key ahead of every other by 80: the others weigh exp(-80) = 1.8e-35 each
    q[..., 1:] = 0.0
    q[..., 0] = 4.0
    k[..., 0], k2[..., 0] = 0.0, 0.0
    j = 7
    k2[:, j, :, 0] = 80.0 / (d ** -0.5 * 4.0)
    out = kernel(q, k, v, k2, v2)
    want = v2[:, j].reshape(b, 1, h * d).expand(b, nq, h * d)
    assert (out - want).abs().max().item() < 1e-6


def recipe_ops(dev, which):
    g = torch.Generator().manual_seed(23)
    if which == "pose":   # PoseEstimator: self-attention over 512 tokens, q / k / v the slices of qkv
        qkv = (torch.randn(10, 512, 3, 8, 64, generator=g) * 1.4).to(dev)
        return (*qkv.unbind(2), None, None)
    q = (torch.randn(2, 384, 8, 64, generator=g) * 1.4).to(dev)   # LayerEstimator: 384 queries, 384 + 512 keys
    kv1 = (torch.randn(2, 384, 2, 8, 64, generator=g) * 1.4).to(dev)
    kv2 = (torch.randn(2, 512, 2, 8, 64, generator=g) * 1.4).to(dev)
    return (q, *kv1.unbind(2), *kv2.unbind(2))


@pytest.mark.parametrize("which", ["pose", "layer"])
def test_the_recipe_shapes(dev, which):
    check(recipe_ops(dev, which), which)


def test_same_bits_from_run_to_run_in_both_deterministic_modes(dev):
    ops = operands(dev, 3, 4, 130, 100, 77, 64, seed=29)
    runs = []
    for mode in (False, True):
        with WF().deterministic(mode):
            runs += [kernel(*ops) for _ in range(3)]
    for out in runs[1:]:
        assert torch.equal(out, runs[0])


def test_one_call_replays_from_a_graph_with_the_same_bits(dev):
    ops = operands(dev, 2, 4, 70, 65, 9, 64, seed=31)
    with torch.no_grad():
        eager = kernel(*ops).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # (warm-up off the default stream, as capture asks for)
            kernel(*ops)
        torch.cuda.current_stream().wait_stream(side)
        static_q = ops[0].clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = kernel(static_q, *ops[1:])
        static_q.zero_()
        graph.replay()
        zeros = static_out.clone()
        static_q.copy_(ops[0])
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(static_out, eager)
    assert not torch.equal(zeros, eager)   # the replay read its input anew


def test_backward_is_the_framework_routes(dev):
    """Gradients of a seeded linear functional in q, k, v, k2, v2 -- packed leaves, so that the slices' gradients meet
    -- against the framework route's in fp32 and fp64."""
    b, n, m, h, d = 2, 70, 37, 2, 32
    g = torch.Generator().manual_seed(37)
    qkv0 = torch.randn(b, n, 3, h, d, generator=g) * 1.4
    kv0 = torch.randn(b, m, 2, h, d, generator=g) * 1.4
    go = torch.randn(b, n, h * d, generator=g)

    def run(fn, dtype):
        qkv = qkv0.to(dev, dtype).requires_grad_()
        kv = kv0.to(dev, dtype).requires_grad_()
        out = fn(*qkv.unbind(2), *kv.unbind(2))
        out.backward(go.to(dev, dtype))
        return out.detach(), qkv.grad, kv.grad

    got = run(kernel, torch.float32)
    r32 = run(WF().token_attention_framework, torch.float32)
    r64 = run(WF().token_attention_framework, torch.float64)
    close(got[0], r32[0], exact=r64[0], what="out")
    close(got[1], r32[1], rel=True, exact=r64[1], what="grad qkv")
    close(got[2], r32[2], rel=True, exact=r64[2], what="grad kv")
    # only what is asked for is computed
    q, k, v = (t.detach() for t in qkv0.to(dev).unbind(2))
    v = v.clone().requires_grad_()
    kernel(q, k, v).backward(go.to(dev))
    assert v.grad is not None and torch.isfinite(v.grad).all()
