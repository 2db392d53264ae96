"""The reference's spelling of the future layer predictor's objective (models/synthesizer.py:752-754 with ``to_ctx`` of
tools/utils.py:84-88), dtype-agnostic: the oracle of ``waldo_amd.supervision.pose_terms`` in fp32 and fp64, and the
inputs and masks its CPU and GPU tests share.  ``to_ctx`` reads ``any()`` on the host and indexes with a boolean mask
(a second host read); that is what the product path avoids, and what is wanted here."""
import torch

NAMES = ("rec_obj_pose", "rec_bg_pose", "rec_occ_score")
MASKS = ("leading", "holes", "none", "all", "one_clip_all")


def to_ctx(tensor, ctx_mask):
    if torch.any(~ctx_mask):
        return tensor[ctx_mask]
    return tensor.reshape(-1, *tensor.shape[2:])


def pose_terms(real, pred, ctx_mask):
    return {name: (to_ctx(r, ~ctx_mask) - to_ctx(p, ~ctx_mask)).abs().mean() for name, r, p in zip(NAMES, real, pred)}


def mask(kind, b, t):
    """A boolean (B, T) ``ctx_mask``: True = context frame (not part of the objective)."""
    steps = torch.arange(t)
    if kind == "leading":
        return (steps < max(t // 3, 1)).expand(b, t).clone()
    if kind == "none":
        return torch.zeros(b, t, dtype=torch.bool)
    if kind == "all":
        return torch.ones(b, t, dtype=torch.bool)
    if kind == "one_clip_all":       # clip 0 has nothing to predict, the others do
        m = (steps < max(t // 3, 1)).expand(b, t).clone()
        m[0] = True
        return m
    assert kind == "holes", kind
    # not only leading frames, and another number of context frames in every clip
    m = torch.zeros(b, t, dtype=torch.bool)
    for i in range(b):
        m[i, 1:2 + i % (t - 1)] = True
    return m


def shapes(b, t, no, lo, l):
    return (b, t, no, lo, 2), (b, t, 1, l, 2), (b, t, no)


def inputs(b, t, no, lo, l, seed=0, dtype=torch.float32):
    """Seeded ``(real, pred)`` 3-tuples of fp32 values (cast to ``dtype``); every fifth element of ``pred`` equals
    ``real`` exactly: sgn(0) = 0 is part of every gradient check."""
    g = torch.Generator().manual_seed(seed)
    real = [torch.randn(*s, generator=g) for s in shapes(b, t, no, lo, l)]
    pred = []
    for r in real:
        p = r + 0.3 * torch.randn(r.shape, generator=g)
        same = (torch.arange(r.numel()) % 5 == 0).view(r.shape)
        pred.append(torch.where(same, r, p))
    return tuple(x.to(dtype) for x in real), tuple(x.to(dtype) for x in pred)


def weights():
    """Another weight per term: a gradient that lands on the wrong tensor shows."""
    return dict(zip(NAMES, (1.0, 0.7, 0.01)))


def terms_and_grads(fn, real, pred, ctx_mask, device=None, dtype=None):
    """``fn(real, pred, ctx_mask)`` on copies of the inputs on ``device`` in ``dtype`` that all require grad: the terms
    (detached), and the gradients of the weighted sum in ``real`` and ``pred`` (None where the terms are not finite and
    ``fn`` is the reference: its mean of an empty selection has nothing to differentiate that is worth comparing)."""
    leaf = lambda x: x.detach().to(device=device, dtype=dtype or x.dtype).clone().requires_grad_()  # noqa: E731
    real, pred = tuple(leaf(x) for x in real), tuple(leaf(x) for x in pred)
    terms = fn(real, pred, ctx_mask.to(device) if torch.is_tensor(ctx_mask) else ctx_mask)
    w = weights()
    sum(w[k] * terms[k] for k in NAMES).backward()
    return ({k: terms[k].detach() for k in NAMES}, tuple(x.grad for x in real), tuple(x.grad for x in pred))
