"""GPU: the FLP networks (``waldo_amd.nets.FLP``) with ``fused = True`` -- ``WF.token_attention_clips`` on the packed
tokens in the encoder's and decoder's blocks, ``WF.token_attention`` in the compressor's, ``WF.pose_affine`` behind the
heads -- against the fixture recorded from the reference's own networks (tests/golden/flp_nets_reference.npz) and against
their own ``fused = False`` route; a forward under an integer-built plan captured in one graph; ``demo.predict_future``."""
import os

import pytest
import torch

import flp_nets_ref as R
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
        got, calls = kernel_calls(lambda: R.run(net, d, dev))
    # the compressor runs twice (background, objects); every block of the encoder and, where there is a frame to
    # predict, both blocks of every decoder step ran the clips kernel on the packed tokens
    predicts = not bool(d["ctx_mask"].all())
    assert calls.get("waldo_token_attention_fwd") == 2 * opt["pg_com_depth"], calls
    assert calls.get("waldo_token_attention_clips_fwd") == opt["pg_enc_depth"] + 2 * opt["pg_dec_depth"] * predicts, calls
    assert calls.get("waldo_pose_affine_fwd") == 2, calls
    R.check(close, got, d, f"{prefix} fused")


@pytest.mark.parametrize("route", ["framework", "kernel"])
def test_fused_and_framework_routes_agree_on_parameter_gradients(dev, route):
    from waldo_amd import functional as WF
    prefix = "a_"
    _, keys, d = R.case(prefix)
    g = torch.Generator().manual_seed(41)
    weights = {k: torch.randn(d[k + "32"].shape, generator=g) for k in R.OUTPUTS}

    def grads(net, device, dtype=torch.float32):
        net.zero_grad(set_to_none=True)
        out = R.run(net, d, device, dtype)
        sum((out[k] * weights[k].to(out[k])).sum() for k in R.OUTPUTS).backward()
        return {k: p.grad for k, p in net.named_parameters()}

    with WF.token_attention_backward_route(route):
        fused, calls = kernel_calls(lambda: grads(R.build(prefix, dev, fused=True), dev))
    if route == "kernel":
        assert calls.get("waldo_token_attention_clips_bwd") == calls.get("waldo_token_attention_clips_fwd_lse") == 4, calls
    else:
        assert calls.get("waldo_token_attention_clips_fwd") == 4 and "waldo_token_attention_clips_bwd" not in calls, calls
    plain = grads(R.build(prefix, dev, fused=False), dev)
    exact = grads(R.build(prefix, "cpu", fused=False, dtype=torch.float64), "cpu", torch.float64)
    for k in keys:
        assert fused[k] is not None, k
        close(fused[k], plain[k], rel=True, exact=exact[k], what=f"{prefix} {route} grad {k}")


def test_a_forward_under_an_integer_built_plan_is_one_graph(dev):
    """Nothing between the inputs and the outputs reads the host: the capture (one stream) is the proof.  The replay
    has the bits of the eager run, and reads its inputs anew."""
    prefix = "b_"
    _, _, d = R.case(prefix)
    net = R.build(prefix, dev, fused=True)
    b, t = d["ctx_mask"].shape
    plan = net.plan(b, t, 2, dev)
    static = R.inputs(d, dev)
    with torch.no_grad():
        eager = [x.clone() for x in net(*static, ctx_mask=plan)]
        mask = (torch.arange(t, device=dev) < 2).expand(b, t)
        masked = net(*static, ctx_mask=mask)
        for x, y in zip(eager, masked):   # (the plan stands for that mask)
            assert torch.equal(x, y)
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
        assert torch.equal(x, y)
    assert not torch.equal(zeros[0], eager[0])


def test_predict_future_on_the_demo_clip(dev, tmp_path):
    """Randomly initialised small networks, FLP's through a saved state dict: finite frames of the right shapes."""
    from waldo_amd.nets import FLP, LVD
    from waldo_amd.nets.wif import WIF
    from waldo_amd.tools import demo
    from waldo_amd.tools import io as wio
    opt = demo.demo_opt(ctx_len=4, latent_shape=[8, 8])   # 128 x 128 frames at scale_factor 2, patch 8: 8 x 8 tokens
    nopt = demo.lvd_demo_opt(opt, embed_dim=64, num_heads=2, oe_depth=1, pe_depth=1, input_rgb=False, input_lyt=True,
                             has_bg=True, pred_cls=True, pe_decoder_init_mode="five", pe_estimator_init_mode="")
    fopt = demo.flp_demo_opt(nopt, pg_com_depth=1, pg_enc_depth=1, pg_dec_depth=1, pg_num_timesteps=6, zero_init_dec=False)
    assert (fopt.embed_dim, fopt.num_heads, fopt.num_obj, fopt.latent_shape) == (64, 2, nopt.num_obj, [8, 8])
    torch.manual_seed(47)
    lvd = LVD(nopt).to(dev).eval()
    src = FLP(fopt)
    torch.save({"state_dict": {"module." + k: v for k, v in src.state_dict().items()}}, tmp_path / "pg.pth")
    flp = demo.load_flp_checkpoint(FLP(fopt), str(tmp_path / "pg.pth")).to(dev).eval()
    for k, v in src.state_dict().items():
        assert torch.equal(flp.state_dict()[k].cpu(), v), k
    with pytest.raises(RuntimeError):   # strictly: another depth does not load
        demo.load_flp_checkpoint(FLP(demo.flp_demo_opt(nopt, pg_com_depth=1, pg_enc_depth=2, pg_dec_depth=1)),
                                 str(tmp_path / "pg.pth"))
    clip = wio.load_clip(CLIP, (128, 128), 20, max_frames=6)
    vid, lyt = clip["vid"].unsqueeze(0).to(dev), clip["lyt"].unsqueeze(0).to(dev)
    wif = WIF(opt, unet=demo.UniformFusionUNet()).to(dev)
    res, calls = kernel_calls(lambda: demo.predict_future(nopt, lvd, flp, wif, vid, lyt, None, 4))
    assert calls.get("waldo_token_attention_clips_fwd") == 3, calls
    assert res["pred_vid"].shape == (1, 6, 3, 128, 128) and res["fused_pred_vid"].shape == (1, 2, 3, 128, 128)
    assert res["pred_disocc"].shape == (1, 2, 1, 128, 128)
    assert torch.equal(res["pred_vid"][:, :4], vid[:, :4])
    for k in ("pred_vid", "fused_pred_vid", "pred_disocc", "obj_pose", "bg_pose", "occ_score"):
        assert torch.isfinite(res[k]).all(), k
    assert res["fused_pred_vid"].std() > 0.05   # a picture, not a blank
    # the context frames' poses are the estimator's, the others FLP's
    rec = demo.reconstruct(nopt, lvd, wif, vid, lyt, None, 4)
    assert torch.equal(res["obj_pose"][:, :4], rec["obj_pose"][:, :4])
    assert not torch.equal(res["obj_pose"][:, 4:], rec["obj_pose"][:, 4:])
    with pytest.raises(ValueError, match="ctx_len"):
        demo.predict_future(nopt, lvd, flp, wif, vid, lyt, None, 6)
