"""CPU: the oracle against the REFERENCE ITSELF -- its outputs on seeded inputs, recorded by oracle/make_golden.py
(gen_live_*) from the reference's own modules into tests/golden/live_*.npz, inputs stored beside them."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_import as R
from oracle import warper_oracle as WO
from oracle import wif_oracle as O

pytestmark = pytest.mark.live_ref
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    data = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: data[k] for k in data.files}


def unflat(d, prefix):
    """What oracle/make_golden.py:flat stored under `prefix`: a tensor, None or a tuple of them."""
    if prefix + ".none" in d:
        return None
    if prefix + ".len" in d:
        return tuple(unflat(d, f"{prefix}.{i}") for i in range(int(d[prefix + ".len"])))
    return torch.from_numpy(d[prefix])


def close(a, b, tol=1e-6):
    assert (a is None) == (b is None)
    if a is None:
        return
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol


def test_buffers_bit_equal():
    ref = load("live_buffers")
    for h, w in [(4, 4), (8, 16), (128, 256), (3, 7)]:
        assert torch.equal(unflat(ref, f"grid_{h}_{w}"), O.get_grid(h, w))
    assert torch.equal(unflat(ref, "gaussian_3"), O.get_gaussian_kernel(3))
    # The TPS buffers go through `log` and `torch.inverse`, whose last bits depend on the CPU's MKL code path.  The
    # reference's calls were recorded (oracle/make_golden.py:record_primitives): the oracle must make the same calls in
    # the same order with bit-identical inputs; it is handed the recorded outputs, and everything it computes around
    # them must give the reference's buffers bit for bit.
    n_calls = sum(1 for k in ref if k.startswith("tps_call.") and k.endswith(".op"))
    calls = [(int(ref[f"tps_call.{i}.op"]), torch.from_numpy(ref[f"tps_call.{i}.in"]),
              torch.from_numpy(ref[f"tps_call.{i}.out"])) for i in range(n_calls)]
    assert [c[0] for c in calls] == [0, 1, 0]  # log (control points), inverse, log (grid)
    made = []

    def replay(op):
        def call(x, *a, **k):
            i = len(made)
            made.append(op)
            assert i < len(calls) and calls[i][0] == op, (i, op)
            assert torch.equal(x, calls[i][1]), f"primitive call {i}: input differs from the reference's"
            return calls[i][2].clone()
        return call
    orig = torch.Tensor.log, torch.log, torch.inverse
    torch.Tensor.log, torch.log, torch.inverse = replay(0), replay(0), replay(1)
    try:
        inv, rep = O.tps_init(16, 32, O.get_grid(4, 4).view(-1, 2))
    finally:
        torch.Tensor.log, torch.log, torch.inverse = orig
    assert made == [c[0] for c in calls]
    assert torch.equal(unflat(ref, "tps_inverse_kernel"), inv) and torch.equal(unflat(ref, "tps_tgt_grid_repr"), rep)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_inverse_warp_random(seed):
    ref = load(f"live_inverse_warp_{seed}")
    sg = unflat(ref, "sg")
    ht, wt = (int(x) for x in ref["target"])
    for erode in (True, False):
        assert torch.equal(unflat(ref, f"erode_{int(erode)}"), O.inverse_warp(sg, (ht, wt), erode=erode))


@pytest.mark.parametrize("over", [dict(), dict(weight_cls=True, min_cls=0.1), dict(load_dim=0),
                                  dict(allow_ghost=True, include_self=True), dict(no_filter=True)])
def test_warper_against_reference(over):
    case = [dict(), dict(weight_cls=True, min_cls=0.1), dict(load_dim=0),
            dict(allow_ghost=True, include_self=True), dict(no_filter=True)].index(over)
    ref = load(f"live_warper_{case}")
    g = lambda k: unflat(ref, k)  # noqa: E731
    size = {k[len("size."):]: int(ref[k]) for k in ref if k.startswith("size.")}  # (the recorded layer / frame size)
    opt = R.warper_opt(num_obj=3, **{**size, **over})
    cfg = WO.WarperCfg.from_opt(opt)
    obj_pose, bg_pose, grid = g("obj_pose"), g("bg_pose"), g("grid")
    for a, c in zip(grid, WO.warper_grids(cfg, obj_pose, bg_pose)):
        close(a, c)
    inp, occ, obj_alpha, bg_alpha, cls = g("inp"), g("occ"), g("obj_alpha"), g("bg_alpha"), g("cls")
    ctx_ts, pred_ts = g("ctx_ts"), g("pred_ts")
    for name in ("grid_to_flow_ctx", "grid_to_flow"):
        for i, c in enumerate((cls,) if opt.weight_cls else (cls, None)):
            r = g(f"{name}.cls{i}")
            o = getattr(WO, name)(cfg, inp, grid, occ, obj_alpha, bg_alpha, c, ctx_ts, pred_ts)
            for x, y in zip(r, o):
                close(x, y, 2e-6)
    ro = g("input_to_output")
    oo = WO.input_to_output(cfg, inp, r[3], r[0], ctx_ts)
    close(ro[0], oo[0])
    close(ro[1], oo[1])
    if cfg.include_self:  # needs Tp == T
        b, t = inp.shape[:2]
        ctx2 = torch.roll(torch.arange(t), 1).view(1, 1, t).expand(b, 1, t)
        r2 = g("self.grid_to_flow")  # LVD training path
        ro = g("self.input_to_output")
        oo = WO.input_to_output(cfg, inp, r2[3], r2[0], ctx2)
        close(ro[0], oo[0])
        close(ro[1], oo[1])
    for x, y in zip(g("alpha_to_alpha"), WO.alpha_to_alpha(cfg, obj_alpha, bg_alpha, grid, occ)):
        close(x, y)
    for x, y in zip(g("layer_from_input"), WO.layer_from_input(cfg, g("x5"), grid)):
        close(x, y)
    close(g("bg_flow_ref_to_pred"), WO.grid_to_bg_flow_from_ref_to_pred(cfg, grid, 2, 1))
    close(g("obj_flow_ref_to_pred"), WO.grid_to_obj_flow_from_ref_to_pred(cfg, grid, 2, 1, 2))
    close(g("bg_flow_ctx_to_ref"), WO.grid_to_bg_flow_from_ctx_to_ref(cfg, grid, 2, 3))


def test_wif_forward_against_reference():
    """WIF.forward with a stand-in UNet (the convolutions are out of scope): the fusion arithmetic
    around it, including the input-channel-4 blending weight (wif.py:53)."""
    ref = load("live_wif_forward")
    vid = torch.from_numpy(ref["vid"])
    b, tc, t, c, h, w = vid.shape
    lin = torch.nn.Conv2d(c, 5, 1)
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(ref["weight"]))
        lin.bias.copy_(torch.from_numpy(ref["bias"]))
    v = vid.permute(0, 2, 1, 3, 4, 5)
    out = lin(v.reshape(b * t * tc, c, h, w)).reshape(b, t, tc, 5, h, w)
    close(torch.from_numpy(ref["out"]), WO.wif_fuse(v, out), 1e-6)


def test_expand_equals_reference_bit_for_bit():
    """tools/utils.py:300-323 against the product's restatement (waldo_amd/tools/utils.py): hard and
    soft masks, every `dir`, several rounds -- and the product must leave its argument alone."""
    from waldo_amd.tools.utils import expand
    ref = load("live_expand")
    hard, soft = torch.from_numpy(ref["hard"]), torch.from_numpy(ref["soft"])
    for d in (None, "south", "north", "east", "west"):
        for num in (1, 2, 5):
            keep = hard.clone()
            assert torch.equal(expand(hard, num, dir=d), torch.from_numpy(ref[f"hard_{d}_{num}"]))
            assert torch.equal(hard, keep)
            keep = soft.clone()
            assert torch.equal(expand(soft, num, dir=d, soft=True), torch.from_numpy(ref[f"soft_{d}_{num}"]))
            assert torch.equal(soft, keep)
    b = hard.bool()
    keep = b.clone()
    expand(b, 3)
    assert torch.equal(b, keep)
