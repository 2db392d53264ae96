"""GPU: ``supervision.pose_terms`` through its kernels (include/waldo_hip.h "Pose objective") against the reference's
spelling (tests/pose_terms_ref.py) on the same inputs, in fp32 on the device and in fp64 on the CPU, under
``parity.close``: the bound is 1e-4 of the tensor's magnitude plus the measured fp32 noise of the reference itself.

The shapes (B, T, No, Lo, L): frames of 24, 12 and 3 elements (odd, under one 16-byte piece, unaligned rows); the
recipe's per-frame sizes with 17 objects (544, 256 and 17: one partial for occ_score, several for obj_pose); and one whose largest term
(1 015 808 elements) spans 496 workgroups, more partials than the finishing pass has lanes."""
import functools

import pytest
import torch

import pose_terms_ref as R
from parity import close

pytestmark = pytest.mark.gpu
SHAPES = {"tiny": (2, 3, 3, 4, 6), "recipe": (3, 5, 17, 16, 128), "large": (8, 32, 31, 64, 8)}
CASES = [(s, k) for s in ("tiny", "recipe") for k in R.MASKS if k != "all"] + [("large", "holes")]


def _kernel(real, pred, ctx_mask):
    from waldo_amd import supervision as S
    return S.pose_terms(real, pred, ctx_mask)


@functools.lru_cache(maxsize=None)
def reference(shape, kind):
    """The inputs and the reference's terms and gradients, fp32 on the device and fp64 on the CPU: computed once."""
    real, pred = R.inputs(*SHAPES[shape])
    m = R.mask(kind, *SHAPES[shape][:2])
    ref32 = R.terms_and_grads(R.pose_terms, real, pred, m, device="cuda:0")
    ref64 = R.terms_and_grads(R.pose_terms, real, pred, m, dtype=torch.float64)
    return real, pred, m, ref32, ref64


def kernel_calls(fn):
    from waldo_amd import _lib
    with _lib.KernelTimer() as timer:
        out = fn()
    torch.cuda.synchronize()
    return out, {k: len(v) for k, v in timer.pairs.items()}


@pytest.mark.parametrize("shape,kind", CASES)
def test_kernel_equals_the_references_spelling(dev, shape, kind):
    real, pred, m, ref32, ref64 = reference(shape, kind)
    got, calls = kernel_calls(lambda: R.terms_and_grads(_kernel, real, pred, m, device=dev))
    assert calls == {"waldo_pose_l1_fwd": 1, "waldo_pose_l1_bwd": 1}, calls   # the three terms: one call each way
    for k in R.NAMES:
        assert got[0][k].ndim == 0 and got[0][k].dtype == torch.float32
        close(got[0][k], ref32[0][k], rel=True, exact=ref64[0][k], what=f"{shape} {kind} {k}")
    for side, name in ((1, "real"), (2, "pred")):
        for i, k in enumerate(R.NAMES):
            g = got[side][i].cpu()
            close(g, ref32[side][i], rel=True, exact=ref64[side][i], what=f"{shape} {kind} grad {name} {k}")
            assert (g[m] == 0).all(), (name, k)                                       # context frames: exact zeros
            planted = (torch.arange(g.numel()) % 5 == 0).view(g.shape)
            assert (g[planted] == 0).all(), (name, k)                                 # sgn(0) = 0 on kept frames too
            assert (g[~m][~planted[~m]] != 0).all(), (name, k)                        # and nowhere else
    for i in range(3):
        assert torch.equal(got[1][i], -got[2][i])


@pytest.mark.parametrize("differ", ["kept", "context"])
def test_the_mask_is_neither_inverted_nor_ignored(dev, differ):
    """pred == real on one side of the mask and a large difference on the other: an inverted mask exchanges the two
    results, an ignored one gives neither."""
    from waldo_amd import supervision as S
    shape = SHAPES["tiny"]
    real, _ = R.inputs(*shape)
    m = R.mask("holes", *shape[:2])
    side = ~m if differ == "kept" else m
    pred = tuple(torch.where(side.view(*m.shape, *([1] * (r.ndim - 2))), r + 100.0, r) for r in real)
    to = lambda xs: tuple(x.to(dev) for x in xs)  # noqa: E731
    got = S.pose_terms(to(real), to(pred), m.to(dev))
    want = R.pose_terms(real, pred, m)
    for k in R.NAMES:
        assert abs(float(want[k]) - (100.0 if differ == "kept" else 0.0)) < 1e-3
        if differ == "kept":
            close(got[k], want[k], rel=True, what=f"differ on {differ} {k}")
        else:
            assert float(got[k]) == 0.0, k


def test_an_all_context_mask_gives_nan_terms_and_zero_gradients(dev):
    real, pred = R.inputs(*SHAPES["tiny"])
    m = R.mask("all", *SHAPES["tiny"][:2])
    terms, grad_real, grad_pred = R.terms_and_grads(_kernel, real, pred, m, device=dev)
    for k in R.NAMES:
        assert torch.isnan(terms[k]), k
    for g in grad_real + grad_pred:
        assert g is not None and (g == 0).all()


def test_bits_repeat_and_a_strided_pred_is_its_contiguous_copy(dev):
    real, pred, m, _, _ = reference("recipe", "holes")
    first = R.terms_and_grads(_kernel, real, pred, m, device=dev)
    again = R.terms_and_grads(_kernel, real, pred, m, device=dev)
    # pred as every second element of a tensor twice as long: the same values behind other strides
    wide = tuple(torch.stack([p, torch.full_like(p, 7.0)], dim=-1).to(dev) for p in pred)
    strided = tuple(w[..., 0] for w in wide)
    assert not any(s.is_contiguous() for s in strided)

    def through_views(real, _, mask):
        views = tuple(s.detach().requires_grad_() for s in strided)
        through_views.leaves = views
        return _kernel(real, views, mask)

    other = R.terms_and_grads(through_views, real, pred, m, device=dev)
    for k in R.NAMES:
        assert torch.equal(first[0][k], again[0][k]) and torch.equal(first[0][k], other[0][k]), k
    for i in range(3):
        assert torch.equal(first[1][i], again[1][i]) and torch.equal(first[2][i], again[2][i])
        assert torch.equal(first[1][i], other[1][i]) and torch.equal(first[2][i], through_views.leaves[i].grad)


def test_grad_real_only_when_asked_and_a_plan_as_the_mask(dev):
    """``real`` under ``no_grad`` (the step's case): one forward and one backward call, gradients in ``pred`` alone, the
    bits of the run that also produced ``grad_real``; the integer-built plan gives the bits of its mask."""
    from waldo_amd import supervision as S
    from waldo_amd.nets.flp import FlpPlan
    shape = SHAPES["recipe"]
    b, t, no = shape[:3]
    real, pred = R.inputs(*shape)
    m = (torch.arange(t) < 2).expand(b, t)
    both = R.terms_and_grads(_kernel, real, pred, m, device=dev)
    real_d = tuple(x.to(dev) for x in real)
    leaves = tuple(x.to(dev).requires_grad_() for x in pred)
    plan = FlpPlan.first_frames(b, t, 2, no + 1, device=dev)

    def run():
        terms = S.pose_terms(real_d, leaves, plan)
        sum(R.weights()[k] * terms[k] for k in R.NAMES).backward()
        return terms

    terms, calls = kernel_calls(run)
    assert calls == {"waldo_pose_l1_fwd": 1, "waldo_pose_l1_bwd": 1}, calls
    assert all(x.grad is None for x in real_d)
    for i, k in enumerate(R.NAMES):
        assert torch.equal(terms[k].detach(), both[0][k]) and torch.equal(leaves[i].grad, both[2][i]), k
    # a term left out of the loss: its tensors get zeros, the others their gradients
    for x in leaves:
        x.grad = None
    S.pose_terms(real_d, leaves, plan)["rec_bg_pose"].mul(0.7).backward()
    assert torch.equal(leaves[1].grad, both[2][1])
    assert (leaves[0].grad == 0).all() and (leaves[2].grad == 0).all()
