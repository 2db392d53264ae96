"""One optimizer step restated in plain torch ops, dtype-agnostic (the parameters' dtype: fp32 or fp64), with Python
control flow: unscale, gradient norm, clip, the non-finite skip, ``torch.optim.Adam`` / ``AdamW``'s single-tensor update
and ``GradScaler.update``'s rule for the scale.  The reference of the optimizer tests; reads the host freely."""
import math

import torch


def new_state(init_scale=1.0):
    return dict(step=0, grad_norm=0.0, clip_coef=1.0, skipped=0, skipped_in_a_row=0, growth=0, scale=float(init_scale))


def grad_norm(grads):
    """sqrt of the sum of squares over all tensors, accumulated in the gradients' dtype."""
    sq = [g.square().sum() for g in grads if g.numel()]
    return float(torch.stack(sq).sum().sqrt()) if sq else 0.0


def step(params, grads, exp_avgs, exp_avg_sqs, st, *, lr, betas, eps, max_norm=0.0, weight_decays=None, adamw=False,
         loss=None, growth_factor=1.0, backoff_factor=1.0, growth_interval=0):
    """In place on ``params``, ``exp_avgs``, ``exp_avg_sqs`` and the dict ``st`` (``new_state``).  ``grads`` carry the
    loss scale ``st["scale"]``.  Returns True for a finite step."""
    b1, b2 = betas
    scale = st["scale"]
    bad = any(not bool(torch.isfinite(g).all()) for g in grads if g.numel())
    if loss is not None and bool(torch.isnan(loss).any()):
        bad = True
    norm = grad_norm(grads) / scale
    coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    st["grad_norm"], st["clip_coef"] = norm, coef
    if bad:
        st["skipped"] += 1
        st["skipped_in_a_row"] += 1
        st["growth"] = 0
        st["scale"] = scale * backoff_factor
        return False
    mult = coef / scale
    st["step"] += 1
    st["skipped_in_a_row"] = 0
    k = st["step"]
    bc1, bc2 = 1 - b1 ** k, 1 - b2 ** k
    wds = [0.0] * len(params) if weight_decays is None else weight_decays
    with torch.no_grad():
        for p, g, m, v, wd in zip(params, grads, exp_avgs, exp_avg_sqs, wds):
            if p.numel() == 0:
                continue
            if adamw and wd != 0:
                p.mul_(1 - lr * wd)
            g = g * mult
            m.lerp_(g, 1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
            p.addcdiv_(m, denom, value=-(lr / bc1))
    st["growth"] += 1
    if growth_interval > 0 and st["growth"] >= growth_interval:
        st["scale"] = scale * growth_factor
        st["growth"] = 0
    return True


# the scale test of the CPU and of the GPU suite: growth_interval = 2 from 1024; an inf step halves the scale, two clean
# steps in a row double it, an inf step in between starts the count again
SCALER = dict(init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2)
SCALE_STEPS_BAD = (True, False, False, False, True, False, True, False, False)
SCALE_AFTER = (512.0, 512.0, 1024.0, 1024.0, 512.0, 512.0, 256.0, 256.0, 512.0)


def run(params, grad_steps, *, dtype, **kw):
    """``optim_ref.step`` over the list of per-step gradient lists on copies of ``params`` in ``dtype`` on the CPU; returns
    per step (params, exp_avgs, exp_avg_sqs, dict(st)) as clones.  ``kw``: ``step``'s keywords and ``init_scale``."""
    st = new_state(kw.pop("init_scale", 1.0))
    ps = [p.detach().cpu().to(dtype).clone() for p in params]
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    out = []
    for grads in grad_steps:
        step(ps, [g.detach().cpu().to(dtype) for g in grads], ms, vs, st, **kw)
        out.append(([p.clone() for p in ps], [m.clone() for m in ms], [v.clone() for v in vs], dict(st)))
    return out
