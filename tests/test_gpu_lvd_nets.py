"""GPU: the LVD networks (``waldo_amd.nets.LVD`` and its parts) with ``fused = True`` -- ``WF.token_attention`` in the
transformer blocks, ``WF.plane_norm_gelu`` in the patch projections, the warp path's kernels behind them -- against the
fixture recorded from the reference's own networks (tests/golden/lvd_nets_reference.npz) and against their own
``fused = False`` route; ``demo.reconstruct``; ``LvdStep(nets="reference")``."""
import os

import pytest
import torch

import lvd_nets_ref as R
from parity import close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP = os.path.join(ROOT, "tests", "golden", "demo_clip", "leftImg8bit_sequence_512", "val", "munster")


def kernel_calls(fn):
    """(fn(), {entry point: launches}) -- what ran natively."""
    from waldo_amd import _lib
    with _lib.KernelTimer() as timer:
        out = fn()
    torch.cuda.synchronize()
    return out, {k: len(v) for k, v in timer.pairs.items()}


@pytest.mark.parametrize("prefix", R.CASES)
def test_fixture_cases_fused_on_the_device(dev, prefix):
    opt, _, d = R.case(prefix)
    net = R.build(prefix, dev, fused=True)
    with torch.no_grad():
        got, calls = kernel_calls(lambda: R.run(net, d["input"].to(dev), opt["ctx_len"]))
    # every attention of both estimators ran in the kernel, and the patch projections' norms in theirs: with
    # s = log2(patch_size) stride-2 steps the encoder has s - 2 conv -> norm -> GELU triples, the decoder s - 1
    steps = opt["patch_size"].bit_length() - 1
    assert calls.get("waldo_token_attention_fwd") == opt["oe_depth"] + opt["pe_depth"], calls
    assert calls.get("waldo_plane_norm_gelu_fwd", 0) == 2 * steps - 3, calls
    R.check(close, got, d, f"{prefix} fused")


def functional_of(net, inp, ctx_len, weights):
    """A seeded linear functional of the 11 outputs, and the outputs."""
    out = R.run(net, inp, ctx_len)
    return sum((out[k] * weights[k].to(out[k])).sum() for k in R.OUTPUTS), out


@pytest.mark.parametrize("prefix", R.CASES)
def test_fused_and_framework_routes_agree_on_outputs_and_parameter_gradients(dev, prefix):
    opt, keys, d = R.case(prefix)
    g = torch.Generator().manual_seed(41)
    weights = {k: torch.randn(d[k + "32"].shape, generator=g) for k in R.OUTPUTS}

    def grads(net, inp):
        net.zero_grad(set_to_none=True)
        loss, out = functional_of(net, inp, opt["ctx_len"], weights)
        loss.backward()
        return {k: v.detach() for k, v in out.items()}, {k: p.grad for k, p in net.named_parameters()}

    fused = grads(R.build(prefix, dev, fused=True), d["input"].to(dev))
    plain = grads(R.build(prefix, dev, fused=False), d["input"].to(dev))
    exact = grads(R.build(prefix, "cpu", fused=False, dtype=torch.float64), d["input"].double())
    for k in R.OUTPUTS:
        close(fused[0][k], plain[0][k], exact=exact[0][k], what=f"{prefix} {k}")
    for k in keys:
        assert fused[1][k] is not None, k
        close(fused[1][k], plain[1][k], rel=True, exact=exact[1][k], what=f"{prefix} grad {k}")


def test_all_five_modes_feed_decode_output(dev):
    from waldo_amd.nets import LVD, lvd_net_opt
    opt, _, d = R.case("a_")
    # case a_'s options on a 16 x 32 raster (patch 8: the same 2 x 4 tokens), freshly seeded
    opt = {**opt, "dim": 16, "patch_size": 8, "pe_estimator_init_mode": ""}
    torch.manual_seed(53)
    net = LVD(lvd_net_opt(**opt)).to(dev).eval()
    b, t = d["input"].shape[:2]
    ctx_len, no, nl = opt["ctx_len"], opt["num_obj"], opt["num_lyt"]
    h, w = opt["dim"], int(opt["dim"] * opt["aspect_ratio"])
    g = torch.Generator().manual_seed(43)
    lyt = 2.0 * torch.randn(b, t, nl, h, w, generator=g)
    inp = torch.cat([lyt, 0.3 * torch.randn(b, t, 2, h, w, generator=g)], dim=2).to(dev)
    with torch.no_grad():
        x = net(input=inp, mode="encode_input")
        x_obj, x_bg, cls = net(x=x[:, :ctx_len], mode="estimate_layer")
        obj_pose, bg_pose, occ_score = net(x=x, x_obj=x_obj, x_bg=x_bg, mode="estimate_pose")[:3]
        occ, obj_alpha, bg_alpha, grid = net(x_obj=x_obj, obj_pose=obj_pose, bg_pose=bg_pose, occ_score=occ_score,
                                             mode="estimate_alpha_grid_occ")
        assert occ.shape == (b, t, no + 1, no + 1) and obj_alpha.shape == (b, no, 1, 16, 16)
        assert bg_alpha.shape == (b, 1, h, w)
        # the padding mask of the object alphas: one pixel of -1 all round
        assert (obj_alpha[..., 0, :] == -1).all() and (obj_alpha[..., :, -1] == -1).all()
        ctx_ts = torch.arange(ctx_len, device=dev).view(1, -1, 1).expand(b, -1, t).contiguous()
        frames = torch.cat([torch.rand(b, t, 3, h, w, generator=g) * 2 - 1, lyt], dim=2).to(dev)
        out = net(input=frames, grid=grid, occ=occ, obj_alpha=obj_alpha, bg_alpha=bg_alpha, ctx_ts=ctx_ts,
                  pred_ts=torch.arange(t, device=dev), cls=cls, mode="decode_output")
    output, flow, _, alpha, raw_alpha, raw_output, alpha_ctx = out
    assert output.shape == (b, t, 3 + nl, h, w) and flow.shape == (b, ctx_len, t, 2, h, w)
    assert raw_output.shape == (b, ctx_len, t, 3 + nl + no + 1, h, w) and alpha_ctx.shape == (b, ctx_len, t, no + 1, h, w)
    for v in (output, flow, raw_alpha, raw_output, alpha_ctx):
        assert torch.isfinite(v).all()


def test_reconstruct_on_the_demo_clip_from_a_saved_state_dict(dev, tmp_path):
    from waldo_amd.nets import LVD
    from waldo_amd.nets.wif import WIF
    from waldo_amd.tools import demo
    from waldo_amd.tools import io as wio
    opt = demo.demo_opt(ctx_len=4, latent_shape=[8, 8])   # 128 x 128 frames at scale_factor 2, patch 8: 8 x 8 tokens
    with pytest.raises(ValueError, match="latent_shape"):
        demo.lvd_demo_opt(demo.demo_opt(ctx_len=4))
    nopt = demo.lvd_demo_opt(opt, embed_dim=64, num_heads=2, oe_depth=1, pe_depth=1, input_rgb=False, input_lyt=True,
                             has_bg=True, pred_cls=True, pe_decoder_init_mode="five", pe_estimator_init_mode="")
    torch.manual_seed(47)
    src = LVD(nopt)
    torch.save({"state_dict": {"module." + k: v for k, v in src.state_dict().items()}}, tmp_path / "pe.pth")
    lvd = demo.load_lvd_checkpoint(LVD(nopt), str(tmp_path / "pe.pth")).to(dev).eval()
    for k, v in src.state_dict().items():
        assert torch.equal(lvd.state_dict()[k].cpu(), v), k
    with pytest.raises(RuntimeError):   # strictly: another width does not load
        demo.load_lvd_checkpoint(LVD(demo.lvd_demo_opt(opt, embed_dim=32, num_heads=2, oe_depth=1, pe_depth=1)),
                                 str(tmp_path / "pe.pth"))
    clip = wio.load_clip(CLIP, (128, 128), 20, max_frames=6)
    vid, lyt = clip["vid"].unsqueeze(0).to(dev), clip["lyt"].unsqueeze(0).to(dev)
    wif = WIF(opt, unet=demo.UniformFusionUNet()).to(dev)
    res = demo.reconstruct(nopt, lvd, wif, vid, lyt, None, 4)
    assert res["rec_vid"].shape == (1, 6, 3, 128, 128) and res["inp_rec_vid"].shape == (1, 6, 3, 128, 128)
    assert res["rec_disocc"].shape == (1, 6, 1, 128, 128) and res["cls"].shape == (1, 3, 20)
    for k in ("rec_vid", "inp_rec_vid", "rec_disocc", "obj_pose", "bg_pose"):
        assert torch.isfinite(res[k]).all(), k
    assert res["inp_rec_vid"].std() > 0.1   # a picture, not a blank
    nopt.input_flow = True
    with pytest.raises(ValueError, match="real_flow"):
        demo.reconstruct(nopt, lvd, wif, vid, lyt, None, 4)


def test_lvd_step_with_the_networks_gives_finite_gradients_everywhere(dev):
    from waldo_amd.tools.lvd_step import LvdStep
    step = LvdStep(1, dev, seed=1, nets="reference")
    (loss, ), calls = kernel_calls(lambda: (step(), ))
    assert torch.isfinite(loss)
    assert calls.get("waldo_token_attention_fwd") == 4, calls   # two blocks in each estimator
    missing = [k for k, p in step.net.named_parameters() if p.grad is None]
    assert not missing, missing
    assert step.grads_finite()
    assert any(float(p.grad.abs().max()) > 0 for p in step.net.layer_estimator.parameters())
