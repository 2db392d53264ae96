"""CPU: the LVD networks (``waldo_amd.nets``: ImageEncoder, LayerEstimator, PoseEstimator, ImageDecoder, LVD; the
transformer blocks of ``waldo_amd.modules.transform``; ``modules.ConvPatchProj``) with ``fused = False`` -- framework ops
only -- against the fixture recorded from the reference's own networks (tests/golden/lvd_nets_reference.npz), and what
their constructors refuse.  No GPU."""
import inspect

import pytest
import torch

import lvd_nets_ref as R
from parity import close


@pytest.mark.parametrize("prefix", R.CASES)
def test_parameter_names_order_and_shapes_are_the_references(prefix):
    from waldo_amd.nets import LVD, lvd_net_opt
    opt, keys, d = R.case(prefix)
    net = LVD(lvd_net_opt(**opt))
    named = list(net.named_parameters())
    assert [k for k, _ in named] == keys
    for k, p in named:
        assert tuple(p.shape) == tuple(d["p." + k].shape), k
    assert sum(p.numel() for _, p in named) == {"a_": 62734, "b_": 141997}[prefix]
    # the parameters come first in the state dict, in that order; what follows them is buffers
    assert [k for k in net.state_dict() if k in set(keys)] == keys
    loaded = R.build(prefix)            # (the strict load)
    for k, p in loaded.named_parameters():
        assert torch.equal(p, d["p." + k]), k
    with pytest.raises(RuntimeError, match="Missing key"):
        net.load_state_dict({k: d["p." + k] for k in keys[1:]}, strict=True)


@pytest.mark.parametrize("prefix", R.CASES)
def test_the_eleven_outputs_in_framework_ops(prefix):
    opt, _, d = R.case(prefix)
    net = R.build(prefix, fused=False)
    assert net.fused is False and not any(m.fused for m in net.modules() if hasattr(m, "fused"))
    with torch.no_grad():
        got = R.run(net, d["input"], opt["ctx_len"])
    R.check(close, got, d, prefix)


def test_the_fused_switch_reaches_every_module_that_has_one():
    net = R.build("a_")
    switches = [m for m in net.modules() if hasattr(m, "fused")]
    assert len(switches) > 10 and all(m.fused for m in switches)
    net.layer_estimator.fused = False
    assert not net.layer_estimator.blocks.multi_blocks[0].attn.attn.fused
    assert net.pose_estimator.blocks.multi_blocks[0].attn.attn.fused and net.encoder.from_img.fused


def test_attention_modules_on_the_cpu_are_the_framework_arithmetic():
    """``fused = True`` on CPU tensors is the same sequence of ops as ``fused = False``: the same bits."""
    from waldo_amd import functional as WF
    from waldo_amd.modules.transform import MultiBlocks
    torch.manual_seed(3)
    args = dict(depth=2, dim=32, num_heads=2, norm_layer="ln", spectral_norm_layer=None, noise=False, dropout=0)
    x, ctx = torch.randn(2, 12, 32), torch.randn(6, 8, 32)
    for block_type, kw in (("full", {}), ("obj", {"x_ctx": ctx})):
        blocks = MultiBlocks(block_type=block_type, **args)
        for p in blocks.parameters():
            p.data.mul_(6.0)
        with torch.no_grad():
            on = blocks(x, **kw)
            blocks.fused = False
            assert torch.equal(on, blocks(x, **kw))
    # the op itself against the spelled-out ops of the reference's ObjAttention
    q, kv1, kv2 = torch.randn(2, 7, 2, 16), torch.randn(2, 7, 2, 2, 16), torch.randn(2, 9, 2, 2, 16)
    qh = q.permute(0, 2, 1, 3)
    a1 = (qh @ kv1[:, :, 0].permute(0, 2, 1, 3).transpose(-2, -1)) * 0.25
    a2 = (qh @ kv2[:, :, 0].permute(0, 2, 1, 3).transpose(-2, -1)) * 0.25
    v = torch.cat([kv1[:, :, 1].permute(0, 2, 1, 3), kv2[:, :, 1].permute(0, 2, 1, 3)], dim=2)
    want = (torch.cat([a1, a2], dim=-1).softmax(dim=-1) @ v).transpose(1, 2).reshape(2, 7, 32)
    assert torch.equal(WF.token_attention(q, *kv1.unbind(2), *kv2.unbind(2)), want)


def test_conv_patch_proj_round_trip_shapes_and_the_served_variants():
    from waldo_amd.modules import ConvPatchProj
    torch.manual_seed(5)
    enc = ConvPatchProj(8, 32, "ln2d", 6, from_patch=True)
    dec = ConvPatchProj(8, 32, "ln2d", 4, skip_channels=3, from_patch=False)
    img = torch.randn(2, 6, 16, 32)
    tokens = enc(img)
    assert tokens.shape == (2, 8, 32)
    assert torch.equal(enc(img[:, :5]), enc(torch.cat([img[:, :5], torch.ones(2, 1, 16, 32)], 1)))   # alpha added
    assert torch.equal(enc(torch.cat([img, img[:, :1]], 1)), tokens)                                  # alpha dropped
    pyramid = enc(img, return_list=True)
    assert [tuple(t.shape[1:]) for t in pyramid] == [(32, 2, 4), (16, 4, 8), (8, 8, 16)]
    out = dec(tokens, latent_shape=(2, 4), skip=torch.randn(2, 3, 16, 32))
    assert out.shape == (2, 4, 16, 32)
    # the encoder's pyramid blended into a decoder without a skip, through a mask
    dec2 = ConvPatchProj(8, 32, "ln2d", 4, from_patch=False)
    m = torch.rand(2, 1, 16, 32)
    blended = dec2(tokens, latent_shape=(2, 4), x_list=pyramid, fuse_m=m)
    assert blended.shape == (2, 4, 16, 32) and not torch.equal(blended, dec2(tokens, latent_shape=(2, 4)))
    hr = ConvPatchProj(4, 32, "ln2d", 5, from_patch=True, hr_ratio=2, use_hr=True)
    assert hr(torch.randn(1, 5, 16, 16)).shape == (1, 4, 32)
    with pytest.raises(NotImplementedError):
        ConvPatchProj(8, 32, "ln2d", 4, skip_channels=3, from_patch=True)
    names = [k for k, _ in dec.named_parameters()]
    assert names == ["layers.0.0.weight", "layers.0.1.norm.weight", "layers.0.1.norm.bias", "layers.1.0.weight",
                     "layers.1.1.norm.weight", "layers.1.1.norm.bias", "skip_proj.weight", "proj.weight"]


def test_unsupported_options_raise():
    from waldo_amd.modules.transform import Block, CustomNorm, FullAttention, Mlp
    from waldo_amd.nets import LVD, lvd_net_opt
    opt, _, _ = R.case("a_")
    for name in ("pe_use_refiner", "pe_use_post_refiner", "pe_use_edge_filter"):
        with pytest.raises(NotImplementedError, match=name):
            LVD(lvd_net_opt(**{**opt, name: True}))
    with pytest.raises(NotImplementedError, match="time_dropout"):
        LVD(lvd_net_opt(**{**opt, "time_dropout": 0.5}))
    with pytest.raises(TypeError, match="unknown fields"):
        lvd_net_opt(no_such_field=1)
    args = dict(depth=1, dim=32, num_heads=2, norm_layer="ln", spectral_norm_layer=None, noise=False, dropout=0)
    for block_type in ("cross", "cls", "ctx", "block_causal", "skip", "skip2"):
        with pytest.raises(NotImplementedError, match=block_type):
            Block(block_type=block_type, **args)
    with pytest.raises(ValueError):
        Block(block_type="nonsense", **args)
    with pytest.raises(NotImplementedError, match="noise"):
        FullAttention(32, 2, None, True)
    with pytest.raises(NotImplementedError, match="spectral"):
        Mlp(32, "sn")
    with pytest.raises(NotImplementedError, match="ctx_mask"):
        FullAttention(32, 2, None, False)(torch.zeros(1, 4, 32), ctx_mask=torch.ones(1, 1, dtype=torch.bool))
    with pytest.raises(ValueError):
        CustomNorm("ln2d", 32)
    assert Block(block_type="full_with_cond_norm", **{**args, "norm_layer": "pn"})(
        torch.randn(2, 4, 32), z_cond=torch.randn(2, 32)).shape == (2, 4, 32)
    with pytest.raises(ValueError, match="mode"):
        R.build("a_")(mode="decode_layer")


def test_defaults_are_the_references_options():
    from waldo_amd.nets import lvd_net_opt
    o = lvd_net_opt()
    assert (o.embed_dim, o.num_heads, o.patch_size, o.latent_shape, o.obj_shape) == (512, 8, 8, [4, 8], [4, 4])
    assert (o.oe_depth, o.pe_depth, o.oe_num_timesteps, o.ctx_len, o.norm_layer, o.norm_layer_patch) == \
        (8, 8, 5, 10, "ln", "ln2d")
    assert (o.pe_pts_mode, o.pe_estimator_init_mode, o.pe_decoder_init_mode, o.occ_mode) == ("prior", "zero", "", "")
    assert (o.min_scale_bound, o.max_scale_bound, o.max_translate_bound, o.circle_translate_radius) == (-0.5, 0.5, 0.5, 0.25)
    assert not (o.has_bg or o.pred_cls or o.bound_rest or o.use_hr or o.input_lyt or o.input_flow) and o.input_rgb


def test_lvd_step_default_is_the_stand_in_step():
    from waldo_amd.tools import lvd_step
    sig = inspect.signature(lvd_step.LvdStep.__init__)
    assert sig.parameters["nets"].default == "stand-in" and sig.parameters["objective"].default == "stand-in"
    assert lvd_step.NETS == ("stand-in", "reference")
    with pytest.raises(ValueError, match="nets must be"):
        lvd_step.LvdStep(1, torch.device("cpu"), nets="real")
    o = lvd_step.recipe_net_opt()
    assert (o.embed_dim, o.num_heads, o.embed_dim // o.num_heads, o.oe_depth, o.pe_depth) == (512, 8, 64, 2, 2)
    assert (o.num_obj, o.latent_shape, o.obj_shape, o.patch_size, o.dim, o.aspect_ratio) == (16, [8, 16], [4, 4], 16, 128, 2)
    # the warp path's options are the stand-in step's own
    assert all(getattr(o, k) == v for k, v in vars(lvd_step.lvd_opt()).items())
