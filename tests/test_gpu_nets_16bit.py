"""GPU: ``act_dtype`` of ``nets.LVD`` and ``nets.FLP`` -- the networks under autocast with the 16-bit token attention kernel.
The networks and inputs are the smallest fixture cases of lvd_nets_ref.py / flp_nets_ref.py.  The yardstick is never the
code under test: per output tensor, the fused network's distance from the fp32 ``fused = False`` outputs is held to
TWICE the distance of ``fused = False`` under the same autocast from those same outputs, both measured here (two 16-bit
evaluations that round at different points each sit one such distance from fp32; a wrong kernel is off by orders of
magnitude).  An output whose framework distance is 0 is compared by the attention bound's TOL instead."""
import pytest
import torch

import flp_nets_ref as FR
import lvd_nets_ref as LR
from parity import TOL
from token_attention_16bit import DTYPES

pytestmark = pytest.mark.gpu


def WF():
    from waldo_amd import functional
    return functional


def launches(fn):
    from waldo_amd import _lib
    with _lib.KernelTimer() as timer:
        out = fn()
    return out, {k: len(v) for k, v in timer.pairs.items()}


def counting(monkeypatch):
    """Every call of the two attention ops the blocks make, by name."""
    seen = {}
    for name in ("token_attention", "token_attention_clips"):
        real = getattr(WF(), name)

        def op(*a, _real=real, _name=name, **kw):
            seen[_name] = seen.get(_name, 0) + 1
            return _real(*a, **kw)
        monkeypatch.setattr(WF(), name, op)
    return seen


def lvd_outputs(prefix, dev, fused, act_dtype):
    opt, _, d = LR.case(prefix)
    net = LR.build(prefix, dev, fused=fused)
    net.act_dtype = act_dtype
    with torch.no_grad():
        return LR.run(net, d["input"].to(dev), opt["ctx_len"])


def flp_outputs(prefix, dev, fused, act_dtype):
    _, _, d = FR.case(prefix)
    net = FR.build(prefix, dev, fused=fused)
    net.act_dtype = act_dtype
    with torch.no_grad():
        return FR.run(net, d, dev)


@pytest.fixture(scope="module")
def fp32_outputs(dev):
    """The fp32 ``fused = False`` outputs of the two smallest cases: the point both distances are measured from."""
    return {"lvd": lvd_outputs("a_", dev, False, None), "flp": flp_outputs("a_", dev, False, None)}


OUTPUTS = {"lvd": lvd_outputs, "flp": flp_outputs}


@pytest.mark.parametrize("which", ["lvd", "flp"])
def test_without_act_dtype_the_network_is_what_it_was(dev, which, monkeypatch):
    seen = counting(monkeypatch)
    base, calls = launches(lambda: OUTPUTS[which]("a_", dev, True, None))
    assert sum(seen.values()) > 0 and not any(k.endswith("_dt") and "token_attention" in k for k in calls), calls
    net_outputs = OUTPUTS[which]("a_", dev, True, None)
    for k, v in base.items():
        if v is not None:
            assert v.dtype == torch.float32 and torch.equal(v, net_outputs[k]), k
    assert WF().get_token_attention_16bit_route() == "framework"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["lvd", "flp"])
def test_the_fused_network_is_as_close_to_fp32_as_the_framework_under_autocast(dev, which, dtype, fp32_outputs,
                                                                              monkeypatch):
    ref = fp32_outputs[which]
    seen = counting(monkeypatch)
    fused, calls = launches(lambda: OUTPUTS[which]("a_", dev, True, dtype))
    # every attention call of the forward was served by the 16-bit kernel
    n = sum(seen.values())
    served = calls.get("waldo_token_attention_fwd_dt", 0) + calls.get("waldo_token_attention_clips_fwd_dt", 0)
    assert n > 0 and served == n, (seen, calls)
    assert "waldo_token_attention_fwd" not in calls and "waldo_token_attention_clips_fwd" not in calls, calls
    assert WF().get_token_attention_16bit_route() == "framework"   # the switch is back where it was
    plain, calls = launches(lambda: OUTPUTS[which]("a_", dev, False, dtype))
    assert not any("token_attention" in k for k in calls), calls
    failed = []
    for name, want in ref.items():
        if want is None:
            assert fused[name] is None
            continue
        assert fused[name].shape == want.shape and torch.isfinite(fused[name].float()).all(), name
        d_fused = (fused[name].float() - want).abs().max().item()
        d_plain = (plain[name].float() - want).abs().max().item()
        limit = 2.0 * d_plain if d_plain > 0 else TOL * max(1.0, want.abs().max().item())
        print(f"[nets16] {which} {dtype} {name}: fused {d_fused:.3e}  framework under autocast {d_plain:.3e}  "
              f"ratio {d_fused / max(d_plain, 1e-30):.3g}")
        if not d_fused <= limit:
            failed.append((name, d_fused, d_plain))
    assert not failed, failed


@pytest.mark.parametrize("dtype", DTYPES)
def test_what_the_warper_receives_is_fp32(dev, dtype):
    opt, _, d = LR.case("a_")
    net = LR.build("a_", dev)
    net.act_dtype = dtype
    got = []
    net.warper.register_forward_pre_hook(lambda m, args: got.extend(a.dtype for a in args if torch.is_tensor(a)))
    with torch.no_grad():
        x = net(input=d["input"].to(dev), mode="encode_input")
        x_obj, x_bg, cls = net(x=x[:, :opt["ctx_len"]], mode="estimate_layer")
        obj_pose, bg_pose, occ_score, rest, bg_rest, last_obj, last_bg = net(x=x, x_obj=x_obj, x_bg=x_bg,
                                                                            mode="estimate_pose")
        occ, obj_alpha, bg_alpha, grid = net(x_obj=x_obj, obj_pose=obj_pose, bg_pose=bg_pose, occ_score=occ_score,
                                             mode="estimate_alpha_grid_occ")
    assert got and all(t == torch.float32 for t in got), got
    flat = [cls, obj_pose, bg_pose, occ_score, rest, bg_rest, last_obj, last_bg, occ, obj_alpha, bg_alpha, *grid]
    assert all(t.dtype == torch.float32 for t in flat if torch.is_tensor(t)), [t.dtype for t in flat if torch.is_tensor(t)]
    assert all(torch.isfinite(t).all() for t in flat if torch.is_tensor(t))


def test_act_dtype_is_passed_on_and_validated():
    from waldo_amd.nets import FLP, LVD, flp_net_opt, lvd_net_opt
    opt, _, _ = LR.case("a_")
    for net in (LVD(lvd_net_opt(**opt)), FLP(flp_net_opt(**FR.case("a_")[0]))):
        assert net.act_dtype is None
        before = sorted(net.state_dict())
        net.act_dtype = torch.bfloat16
        subs = [m for m in net.modules() if hasattr(m, "_act_dtype")]
        assert len(subs) > 3 and all(m.act_dtype is torch.bfloat16 for m in subs)
        with pytest.raises(ValueError, match="act_dtype"):
            net.act_dtype = torch.float32
        net.act_dtype = None
        assert all(m.act_dtype is None for m in subs) and sorted(net.state_dict()) == before


def test_lvd_step_takes_a_step_in_bf16(dev):
    from waldo_amd.tools.lvd_step import LvdStep
    with pytest.raises(ValueError, match="act_dtype"):
        LvdStep(2, dev, act_dtype=torch.bfloat16)
    step = LvdStep(2, dev, nets="reference", act_dtype=torch.bfloat16)
    assert step.net.act_dtype is torch.bfloat16
    loss, calls = launches(step)
    assert calls.get("waldo_token_attention_fwd_dt", 0) > 0 and "waldo_token_attention_fwd" not in calls, calls
    assert "waldo_token_attention_bwd" not in calls, calls
    assert torch.isfinite(loss).all()
    grads = [p.grad for p in step.net.parameters() if p.grad is not None]
    assert len(grads) > 10 and all(g.dtype == torch.float32 and bool(torch.isfinite(g).all()) for g in grads)


@pytest.mark.parametrize("dtype", DTYPES)
def test_flp_under_a_plan_replays_from_one_graph(dev, dtype):
    prefix = "b_"
    _, _, d = FR.case(prefix)
    net = FR.build(prefix, dev, fused=True)
    net.act_dtype = dtype
    b, t = d["ctx_mask"].shape
    plan = net.plan(b, t, 2, dev)
    static = FR.inputs(d, dev)
    with torch.no_grad():
        eager, calls = launches(lambda: [x.clone() for x in net(*static, ctx_mask=plan)])
        assert calls.get("waldo_token_attention_clips_fwd_dt", 0) > 0 and "waldo_token_attention_clips_fwd" not in calls
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # (warm-up off the default stream, as capture asks for)
            net(*static, ctx_mask=plan)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = net(*static, ctx_mask=plan)
        kept = static[0].clone()
        static[0].zero_()
        graph.replay()
        zeros = [x.clone() for x in out]
        static[0].copy_(kept)
        graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(out, eager):
        assert x.dtype == torch.float32 and torch.equal(x, y)
    assert not torch.equal(zeros[0], eager[0])
