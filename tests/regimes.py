"""Operands chosen for the path a single-op kernel takes on them, and the host-side predicates that say so.

The single-op parity tests draw every operand i.i.d. (``rand`` alphas, ``randn`` logits, ``rand * 2.4 - 1.2`` grids).
Several kernels choose a path, or have a numerical hazard, that depends on the VALUES: the wave-uniform early exit of
the four-pixel grid_sample forward (256 consecutive pixels with every tap outside), the run merging of its backward
(equal texel addresses in neighbouring lanes), the max subtraction of the WIF softmax (logits spread by more than 88),
the occlusion product at many layers (a product of ~L factors: with ``rand`` operands almost every output is below
the absolute tolerance).  The builders below make such operands; every one is seeded.  The predicates restate the
formulas of csrc/waldo_common.hip.h (un-normalise, clamp, floor, tap validity) in torch, so that a test can assert
from the operands themselves that they take the path it is named after -- a later change of seed or shape cannot
quietly leave the path again.  The criteria at the end are the comparisons of tests/test_gpu_regimes.py, shared with
tests/test_operand_regimes_cpu.py, which runs them on the oracle alone.  Pure torch on the CPU."""
import functools

import torch

from oracle import warper_oracle as WO
from oracle import wif_oracle as O
from parity import close


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------ occ_composite / compute_occ
OCC_LAYERS = (1, 2, 8, 12, 17, 21, 32)
# scores planted next to a pair of equal ones: exp(-s^2) is 1, below eps = 1e-6 (|s| = 4), far below it (6), zero in
# fp32 (12: exp(-144)) and zero in fp64 as well (1e4); +s and -s give the same exp(-s^2): more exact ties
PLANTED_SCORES = (0.0, 4.0, -4.0, 6.0, -6.0, 12.0, -12.0, 1e4, -1e4)


def sparse_alphas(m, nl, h, w, seed):
    """(m, nl, h, w) alphas of a layered scene: per pixel min(3, nl) layers chosen at random are present (alpha in
    [0.3, 1]), every other one is nearly transparent (U(0, 0.02)) -- the occlusion product then keeps outputs of
    order 0.1 in every layer at every layer count.  Pixel column 0 is exactly 0 in every layer, column 1 exactly 1."""
    assert w >= 2
    g = _gen(seed)
    a = torch.rand(m, nl, h, w, generator=g) * 0.02
    k = min(3, nl)
    pick = torch.rand(m, nl, h, w, generator=g).argsort(dim=1)[:, :k]
    a.scatter_(1, pick, 0.3 + 0.7 * torch.rand(m, k, h, w, generator=g))
    a[..., 0] = 0.0
    a[..., 1] = 1.0
    return a


def planted_scores(m, no, seed):
    """(m, 1, no) occlusion scores 1.5 * randn with, at random positions of every row, two equal scores and as many of
    PLANTED_SCORES as fit."""
    g = _gen(seed)
    s = 1.5 * torch.randn(m, 1, no, generator=g)
    for i in range(m):
        pos = torch.randperm(no, generator=g).tolist()
        if no >= 2:
            s[i, 0, pos[1]] = s[i, 0, pos[0]]
        for v, p in zip(PLANTED_SCORES, pos[2:]):
            s[i, 0, p] = v
    return s


def ordering_occ(m, nl, seed):
    """(m, nl, nl) occlusion matrices of planted_scores: entries of exactly 0.5 off the diagonal (ties), within 1e-6
    of 0 and of 1 (an object behind / in front of everything), a zero diagonal."""
    return O.compute_occ(planted_scores(m, nl - 1, seed))[:, 0]


# ------------------------------------------------------------------------------------------ sampling maps (8 x 8 input)
def affine_map(ho=32, wo=64, n=1):
    """(n, ho, wo, 2): gx = -1.5 + 3 (c + .5) / wo, gy likewise -- the frame seen through an object canvas that covers
    its middle.  No jitter: for ho = 32, wo = 64 every coordinate is a multiple of 2^-7, exact in fp32, and over an
    8 x 8 input its un-normalised coordinates stay 1/32 px away from every integer, so every floor is the oracle's in
    fp32 and fp64.  The first and the last four rows have every tap outside."""
    gx = -1.5 + 3 * (torch.arange(wo) + 0.5) / wo
    gy = -1.5 + 3 * (torch.arange(ho) + 0.5) / ho
    grid = torch.stack([gx.expand(ho, wo), gy[:, None].expand(ho, wo)], dim=-1)
    return grid[None].repeat(n, 1, 1, 1)


def constant_map(ho, wo, point, n=1):
    """(n, ho, wo, 2): every pixel samples the one point (gx, gy): every lane of the backward hits the same texels."""
    return torch.tensor(point, dtype=torch.float32).expand(n, ho, wo, 2).contiguous()


def dyadic_coords(size=8):
    """22 coordinates that are exact in fp32 under any contraction of the un-normalisation over `size` texels: the
    image border and beyond it (-1, 1, +-1.25, 1.5), wild ones (+-1e30: finite after un-normalising), the texel centres
    (integer pixel coordinates: fx = 0) and the texel boundaries (half-integer ones)."""
    assert size == 8
    far = [-1.0, 1.0, -1.25, 1.25, 1.5, 1e30, -1e30]
    centres = [-1 + (2 * k + 1) / size for k in range(size)]
    bounds = [-1 + 2 * k / size for k in range(1, size)]  # (k = 0 and k = size are the -1 and 1 above)
    c = torch.tensor(far + centres + bounds, dtype=torch.float32)
    assert c.numel() == 22 and c.unique().numel() == 22
    return c


def dyadic_map(size=8, n=1):
    """(n, 22, 22, 2): the outer product of dyadic_coords; Ho * Wo = 484 is a multiple of 4 (the four-pixel forward)."""
    c = dyadic_coords(size)
    k = c.numel()
    grid = torch.stack([c.expand(k, k), c[:, None].expand(k, k)], dim=-1)
    return grid[None].repeat(n, 1, 1, 1)


def iid_map(n, ho, wo, seed, span=1.2):
    """The grid of the existing single-op tests: i.i.d. uniform in [-span, span]."""
    return (torch.rand(n, ho, wo, 2, generator=_gen(seed)) * 2 - 1) * span


# ------------------------------------------------------------------------------------------ path predicates
def corners(grid, hi, wi):
    """tap_core() of waldo_common.hip.h in fp32: (x0, y0) integer corners of every pixel, after the clamp to
    [-2, size + 1] that keeps wild coordinates defined.  Finite coordinates only."""
    g = grid.float()
    assert torch.isfinite(g).all()
    ix = ((g[..., 0] + 1.0) * float(wi) - 1.0) * 0.5
    iy = ((g[..., 1] + 1.0) * float(hi) - 1.0) * 0.5
    assert torch.isfinite(ix).all() and torch.isfinite(iy).all()
    x0 = ix.clamp(-2.0, wi + 1.0).floor().long()
    y0 = iy.clamp(-2.0, hi + 1.0).floor().long()
    return x0, y0


def any_tap_valid(grid, hi, wi):
    """(n, ho, wo) bool: some corner of the pixel's footprint lies inside the input (`touches` of the forward, a
    non-zero weight being possible in the backward)."""
    x0, y0 = corners(grid, hi, wi)
    vx = ((x0 >= 0) & (x0 < wi)) | ((x0 + 1 >= 0) & (x0 + 1 < wi))
    vy = ((y0 >= 0) & (y0 < hi)) | ((y0 + 1 >= 0) & (y0 + 1 < hi))
    return vx & vy


def _span_state(grid, hi, wi, span):
    """Per map and per `span`-pixel piece of the flattened map (the pixels of one wavefront: 256 in the four-pixel
    forward, 64 in the backward; pieces start at the map's first pixel, the last may be short): (none valid, all
    valid)."""
    v = any_tap_valid(grid, hi, wi).flatten(1)
    pieces = v.split(span, dim=1)
    none = torch.stack([~p.any(dim=1) for p in pieces], dim=1)
    every = torch.stack([p.all(dim=1) for p in pieces], dim=1)
    return none, every


def spans_all_outside(grid, hi, wi, span):
    """How many `span`-pixel pieces of the flattened maps have no valid tap at all."""
    return int(_span_state(grid, hi, wi, span)[0].sum())


def spans_straddling(grid, hi, wi, span):
    """How many `span`-pixel pieces hold both pixels with and pixels without a valid tap."""
    none, every = _span_state(grid, hi, wi, span)
    return int((~none & ~every).sum())


def outside_span_mask(grid, hi, wi, span):
    """(n, ho, wo) bool: the pixels of the pieces spans_all_outside counts."""
    n, ho, wo, _ = grid.shape
    none = _span_state(grid, hi, wi, span)[0]
    return none.repeat_interleave(span, dim=1)[:, :ho * wo].reshape(n, ho, wo)


def address_runs(grid, hi, wi, row=16):
    """Lengths of the runs of equal clamped (y0, x0) -- the texel address of the first tap -- in consecutive pixels of
    the flattened maps, cut at every `row`-pixel boundary: what run_sum() of the backward merges into one atomic."""
    x0, y0 = corners(grid, hi, wi)
    key = (y0.clamp(0, hi - 1) * wi + x0.clamp(0, wi - 1)).flatten(1)
    out = []
    for k in key:
        idx = torch.arange(k.numel())
        start = torch.ones(k.numel(), dtype=torch.bool)
        start[1:] = (k[1:] != k[:-1]) | (idx[1:] % row == 0)
        first = idx[start]
        out.append(torch.diff(first, append=torch.tensor([k.numel()])))
    return torch.cat(out)


def pair_shifts(grid, hi, wi):
    """`shift` of pair_off() (csrc/grid_sample.hip) on the pixels with a valid tap: x0 - clamp(x0, 0, wi - 2)."""
    assert wi >= 2
    x0, _ = corners(grid, hi, wi)
    return (x0 - x0.clamp(0, wi - 2))[any_tap_valid(grid, hi, wi)]


# ------------------------------------------------------------------------------------------ wif_fuse
WIF_SHAPES = ((1, 2, 5, 8, 5, 3, 5), (1, 1, 1, 5, 4, 9, 13), (2, 1, 4, 40, 5, 8, 16))  # (b, t, tc, c, co, h, w)
MASKED_ROW, TIED_ROW = 0, 1  # pixel rows: context 0 has a -inf logit / contexts 0 and 1 share the largest logit


def wif_regime(seed, b, t, tc, c, co, h, w):
    """vid (b, t, tc, c, h, w), net (b, t, tc, co, h, w) of a trained model rather than of randn: the gate's logit
    vid[..., 4] = -5 + 6 randn (sigmoid(. + 5) from ~1e-9 to 1), the score net[..., 3] = 40 randn (a softmax that is
    non-finite without its max subtraction); with more than one context, context 0 is masked (-inf) on pixel row
    MASKED_ROW and contexts 0 and 1 are two equal maxima of at least 100 on pixel row TIED_ROW."""
    g = _gen(seed)
    vid = torch.randn(b, t, tc, c, h, w, generator=g)
    vid[:, :, :, 4] = -5 + 6 * torch.randn(b, t, tc, h, w, generator=g)
    net = torch.randn(b, t, tc, co, h, w, generator=g)
    net[:, :, :, 3] = 40 * torch.randn(b, t, tc, h, w, generator=g)
    if tc >= 2:
        assert h >= 2
        net[:, :, 0, 3, MASKED_ROW] = float("-inf")
        top = net[:, :, :, 3, TIED_ROW].amax(dim=2).clamp_min(100.0)  # (exp(100) is past fp32)
        net[:, :, 0, 3, TIED_ROW] = top
        net[:, :, 1, 3, TIED_ROW] = top
    return vid, net


def wif_fuse_naive(vid, net, ab=True):
    """oracle/warper_oracle.py:wif_fuse with ONE planted error: the softmax without its max subtraction."""
    e = net[:, :, :, 3:4].exp()
    score = e / e.sum(dim=2, keepdim=True)
    a = torch.sigmoid(vid[:, :, :, 4:5] + 5) if ab else 0
    return ((a * vid[:, :, :, :3] + net[:, :, :, :3]) * score).sum(dim=2)


# ------------------------------------------------------------------------------------------ cases: operands + oracle
def _leaf(x, dt):
    return x.detach().to(dt, copy=True).requires_grad_()


def _both(run):
    return run(torch.float32), run(torch.float64)


@functools.lru_cache(maxsize=None)
def occ_case(nl, m=4, div=2, h=9, w=31):
    """(alpha, occ, wgt, ref32, ref64) with ref = (out, grad_alpha, grad_occ) of the oracle.  Shared: do not modify."""
    alpha, occ = sparse_alphas(m, nl, h, w, seed=nl), ordering_occ(m // div, nl, seed=100 + nl)
    wgt = torch.randn(m, nl, h, w, generator=_gen(200 + nl))

    def run(dt):
        a, o = _leaf(alpha, dt), _leaf(occ, dt)
        out = O.occlusion_product(a, o.repeat_interleave(div, dim=0))
        (out * wgt.to(dt)).sum().backward()
        return out.detach(), a.grad, o.grad

    return (alpha, occ, wgt) + _both(run)


@functools.lru_cache(maxsize=None)
def score_case(no, m=3):
    """(score, wgt, ref32, ref64) with ref = (occ, grad_score) of O.compute_occ on planted_scores."""
    score = planted_scores(m, no, seed=300 + no)
    wgt = torch.randn(m, 1, no + 1, no + 1, generator=_gen(400 + no))

    def run(dt):
        s = _leaf(score, dt)
        occ = O.compute_occ(s)
        (occ * wgt.to(dt)).sum().backward()
        return occ.detach(), s.grad

    return (score, wgt) + _both(run)


@functools.lru_cache(maxsize=None)
def wif_case(shape, ab):
    """(vid, net, wgt, ref32, ref64) with ref = (out, grad_vid, grad_net) of WO.wif_fuse on wif_regime."""
    b, t, tc, c, co, h, w = shape
    vid, net = wif_regime(500 + c, *shape)
    wgt = torch.randn(b, t, 3, h, w, generator=_gen(600 + c))

    def run(dt):
        v, n = _leaf(vid, dt), _leaf(net, dt)
        out = WO.wif_fuse(v, n, ab=ab)
        (out * wgt.to(dt)).sum().backward()
        return out.detach(), v.grad, n.grad

    return (vid, net, wgt) + _both(run)


GS_INPUT = (2, 3, 8, 8)
GS_DELTAS = (0.0, 0.5, 1.0)
GS_MAPS = ("affine", "constant", "dyadic")


@functools.lru_cache(maxsize=None)
def gs_map(name):
    n = GS_INPUT[0]
    if name == "affine":
        return affine_map(32, 64, n)
    if name == "constant":  # (180 pixels: three wavefronts of the backward, the last one short)
        return constant_map(9, 20, (0.3, -0.2), n)
    assert name == "dyadic"
    return dyadic_map(8, n)


def gs_oracle(x, grid, wgt, delta):
    def run(dt):
        xi, gr = _leaf(x, dt), _leaf(grid, dt)
        out = O.grid_sample_delta(xi, gr, delta)
        (out * wgt.to(dt)).sum().backward()
        return out.detach(), xi.grad, gr.grad

    return _both(run)


@functools.lru_cache(maxsize=None)
def gs_case(name, delta):
    """(x, grid, wgt, ref32, ref64) with ref = (out, grad_x, grad_grid) of O.grid_sample_delta."""
    grid = gs_map(name)
    x = torch.randn(*GS_INPUT, generator=_gen(700))
    wgt = torch.randn(GS_INPUT[0], GS_INPUT[1], *grid.shape[1:3], generator=_gen(701))
    return (x, grid, wgt) + gs_oracle(x, grid, wgt, delta)


DEGENERATE_INPUTS = ((1, 1), (1, 2), (2, 1), (2, 2), (1, 7), (5, 1))


@functools.lru_cache(maxsize=None)
def degenerate_case(hi, wi, delta=0.5):
    """Inputs of one or two texels a side under dense i.i.d. grids in [-1.3, 1.3]: an 8 x 8 grid (the four-pixel
    forward) and the 7 x 9 one (the one-pixel forward) whose first 8 columns are the first 7 rows of the other, so
    that 56 sample points go through both forms.  (x, wgt8, wgt9, grid8, grid9, refs8, refs9)."""
    n, c = 2, 3
    x = torch.randn(n, c, hi, wi, generator=_gen(800 + 10 * hi + wi))
    grid8 = iid_map(n, 8, 8, seed=810 + 10 * hi + wi, span=1.3)
    extra = iid_map(n, 7, 1, seed=820 + 10 * hi + wi, span=1.3)
    grid9 = torch.cat([grid8[:, :7], extra], dim=2).contiguous()
    wgt8 = torch.randn(n, c, 8, 8, generator=_gen(830))
    wgt9 = torch.randn(n, c, 7, 9, generator=_gen(831))
    return x, wgt8, wgt9, grid8, grid9, gs_oracle(x, grid8, wgt8, delta), gs_oracle(x, grid9, wgt9, delta)


# ------------------------------------------------------------------------------------------ criteria
# Every comparison is tests/parity.py:close at the project's TOL, the fp32 oracle as the reference and the fp64 oracle
# as `exact`.  got / ref32 / ref64 are the tuples of the cases above.
def check_occ(got, ref32, ref64, tag=""):
    # every layer against its own magnitude: the absolute 1e-4 does not see a layer whose outputs are below it
    close(got[0], ref32[0], rel=True, what=tag + "occ_composite out", exact=ref64[0], slice_dims=(1,))
    close(got[1], ref32[1], rel=True, what=tag + "occ_composite grad_alpha", exact=ref64[1])
    close(got[2], ref32[2], rel=True, what=tag + "occ_composite grad_occ", exact=ref64[2])


def check_scores(got, ref32, ref64, tag=""):
    close(got[0], ref32[0], what=tag + "compute_occ occ", exact=ref64[0])
    close(got[1], ref32[1], rel=True, what=tag + "compute_occ grad_score", exact=ref64[1])


def check_wif(got, ref32, ref64, tag=""):
    close(got[0], ref32[0], what=tag + "wif_fuse out", exact=ref64[0])
    # per channel: the gate's channel 4 and the score's channel 3 against themselves
    close(got[1], ref32[1], rel=True, what=tag + "wif_fuse grad_vid", exact=ref64[1], slice_dims=(3,))
    close(got[2], ref32[2], rel=True, what=tag + "wif_fuse grad_net", exact=ref64[2], slice_dims=(3,))


def check_gs(got, ref32, ref64, tag=""):
    close(got[0], ref32[0], what=tag + "grid_sample out", exact=ref64[0])
    close(got[1], ref32[1], rel=True, what=tag + "grid_sample grad_x", exact=ref64[1])
    close(got[2], ref32[2], rel=True, what=tag + "grid_sample grad_grid", exact=ref64[2])
