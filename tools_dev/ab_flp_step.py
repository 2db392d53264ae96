"""A/B of the FLP training step's objective and of the step itself (waldo_amd.supervision.pose_terms,
waldo_amd.tools.flp_step.FlpStep) at the shape of scripts/cityscapes/train_flp.sh on one MI355X: 4 clips of 14 frames of
128 x 256, 4 context frames, 16 objects, the recipe's networks.  Writes profiles/flp_step.json.

    python tools_dev/ab_flp_step.py [--out profiles/flp_step.json] [--rounds 30] [--warmup 5]

Routes of the objective, the SAME inputs:
  kernel     ``pose_terms(fused=True)`` under the step's integer-built plan: one call forward, one launch backward;
  framework  ``pose_terms(fused=False)``: the masked sum in framework ops, no host read either;
  reference  the reference's spelling (models/synthesizer.py:752-754): six ``to_ctx`` calls, each an ``any()`` read on the
             host and a boolean-mask index (a second read: ``nonzero`` needs its size).
Sections: ``objective`` (the op alone on the step's own poses: forward, and forward + backward to ``pred``), ``step``
(the whole eager step -- producers, FLP, objective, backward -- per objective route under both routes of the attention's
backward), ``graph`` (the kernel-objective step eager against replayed from ONE graph).
Method: tools_dev/ab_flp.py's -- device time between events, the routes ALTERNATE inside one process, median / minimum /
quartiles per route, ``spread`` the largest interquartile range over its median.  ``fused_default`` applies the rule:
the kernel unless the framework route is faster by more than the spread BOTH at the op (forward + backward) and in the
step.  A run without a GPU fails."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ab_lvd_nets import alternate  # noqa: E402
from waldo_amd import functional as WF  # noqa: E402
from waldo_amd import supervision  # noqa: E402
from waldo_amd.tools.flp_step import FlpStep  # noqa: E402

B, T, CTX = 4, 14, 4


def _to_ctx(tensor, ctx_mask):
    """The reference's to_ctx (tools/utils.py:84-88): a host read and a boolean-mask load."""
    return tensor[ctx_mask] if bool(torch.any(~ctx_mask)) else tensor.reshape(-1, *tensor.shape[2:])


def reference_terms(real, pred, ctx_mask):
    return {name: (_to_ctx(r, ~ctx_mask) - _to_ctx(p, ~ctx_mask)).abs().mean()
            for name, r, p in zip(supervision.POSE_TERMS, real, pred)}


def faster_beyond_spread(sec, a, b):
    """Route ``a`` of section ``sec`` is faster than ``b`` by more than the section's spread."""
    return bool(sec[a]["median_ms"] < sec[b]["median_ms"] * (1.0 - sec["spread"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flp_step.json"))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    # (zero_init_dec off: with the reference's zero heads nothing upstream of them gets a gradient in the first step)
    step = FlpStep(B, dev, frames=T, ctx_len=CTX, flp_over=dict(zero_init_dec=False))
    mask = (torch.arange(T, device=dev) < CTX).expand(B, T).contiguous()
    doc = dict(shape=dict(clips=B, frames=T, ctx_len=CTX, height=step.lyt.shape[-2], width=step.lyt.shape[-1],
                          lvd=vars(step.lvd_opt), flp=vars(step.flp_opt)),
               device=torch.cuda.get_device_name(0), rounds=args.rounds, warmup=args.warmup)

    # the op alone, on the step's own poses
    inputs = step.producers()
    with torch.no_grad():
        pred = tuple(x.clone() for x in step.flp(*inputs, ctx_mask=step.plan))
    real = inputs[:3]
    leaves = tuple(x.clone().requires_grad_() for x in pred)
    routes = {"kernel": lambda r, p: supervision.pose_terms(r, p, step.plan, fused=True),
              "framework": lambda r, p: supervision.pose_terms(r, p, step.plan, fused=False),
              "reference": lambda r, p: reference_terms(r, p, mask)}

    def fwd_bwd(fn):
        for x in leaves:
            x.grad = None
        terms = fn(real, leaves)
        sum(terms.values()).backward()

    with torch.no_grad():
        got, want = routes["kernel"](real, pred), routes["reference"](real, pred)
        doc["max_abs_kernel_minus_reference"] = max(abs(float(got[k]) - float(want[k])) for k in got)
        fwd = alternate({k: (lambda fn=fn: fn(real, pred)) for k, fn in routes.items()}, args.warmup, args.rounds)
    doc["objective"] = dict(forward=fwd, forward_backward=alternate({k: (lambda fn=fn: fwd_bwd(fn))
                                                                     for k, fn in routes.items()}, args.warmup, args.rounds))

    # the whole eager step
    def run(objective, route):
        step.objective = "kernel" if objective == "kernel" else "framework"
        spelled = reference_terms if objective == "reference" else None
        saved = step.objective_terms
        if spelled is not None:
            step.objective_terms = lambda r, p, m: spelled(r, p, mask)
        try:
            with WF.token_attention_backward_route(route):
                step()
        finally:
            step.objective_terms = saved

    doc["step"] = alternate({f"{o}_bwd_{r}": (lambda o=o, r=r: run(o, r)) for r in ("kernel", "framework")
                             for o in ("kernel", "framework", "reference")}, args.warmup, args.rounds)

    # eager against one graph (the default backward route of the attention)
    step.objective = "kernel"
    eager_loss = step().clone()
    graphed = FlpStep(B, dev, frames=T, ctx_len=CTX, flp_over=dict(zero_init_dec=False), graph=True)
    doc["graph_replay_bit_equal"] = bool(torch.equal(graphed().clone(), eager_loss))
    doc["graph"] = alternate({"eager": step, "replay": graphed}, args.warmup, args.rounds)

    op, st = doc["objective"]["forward_backward"], doc["step"]
    flip = faster_beyond_spread(op, "framework", "kernel") and all(
        faster_beyond_spread(st, f"framework_bwd_{r}", f"kernel_bwd_{r}") for r in ("kernel", "framework"))
    doc["fused_default"] = not flip
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    for name, sec in (("fwd", doc["objective"]["forward"]), ("fwd+bwd", op), ("step", st), ("graph", doc["graph"])):
        for k, v in sec.items():
            if isinstance(v, dict):
                print(f"{name:8s} {k:26s} median {v['median_ms']:8.3f} ms  min {v['min_ms']:8.3f}  "
                      f"IQR [{v['q1_ms']:.3f}, {v['q3_ms']:.3f}]")
        print(f"{name:8s} spread {sec['spread']:.3f}")
    print("fused_default", doc["fused_default"], " graph bits", doc["graph_replay_bit_equal"],
          " |kernel - reference|", doc["max_abs_kernel_minus_reference"])


if __name__ == "__main__":
    main()
