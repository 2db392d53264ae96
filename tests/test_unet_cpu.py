"""CPU: ``waldo_amd.modules.UNet`` and ``WIF.with_unet`` without a GPU -- the framework-op route of
``WF.plane_norm_gelu`` -- against the fixture recorded from the reference's own UNet (tests/golden/unet_reference.npz,
tools_dev/make_unet_golden.py), and, where the reference tree is present, against the reference's WIF itself."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_ref as U  # noqa: E402
from parity import close  # noqa: E402


@pytest.mark.parametrize("prefix", U.CASES)
def test_unet_equals_the_reference_fixture(prefix):
    cfg, keys, d = U.case(prefix)
    net = U.build(prefix)
    assert list(net.state_dict().keys()) == keys           # the reference's names, in its order
    assert [k for k, _ in net.named_parameters()] == keys
    U.check(close, U.run(net, d["x"], d["grad_out"]), d, keys, f"cpu {prefix}")


def test_key_names_are_the_references():
    _, keys, _ = U.case("a_")
    assert keys[:4] == ["to_emb.weight", "from_emb.weight", "conv_layers.0.0.weight", "conv_layers.0.1.norm.weight"]
    assert "conv_layers.2.1.norm.bias" in keys and "deconv_layers.2.1.norm.weight" in keys and len(keys) == 2 + 6 * 3


@pytest.mark.parametrize("prefix", U.CASES)
def test_fused_and_unfused_agree_on_the_cpu(prefix):
    _, keys, d = U.case(prefix)
    a = U.run(U.build(prefix, fused=True), d["x"], d["grad_out"])
    b = U.run(U.build(prefix, fused=False), d["x"], d["grad_out"])
    close(a[0], b[0], rel=True, what="out")
    close(a[1], b[1], rel=True, what="grad_x")
    for k in keys:
        close(a[2][k], b[2][k], rel=True, what=k)


def test_plane_norm_gelu_on_the_cpu_is_the_framework_arithmetic():
    from waldo_amd import functional as WF
    g = torch.Generator().manual_seed(1)
    x, skip = torch.randn(2, 3, 5, 7, generator=g), torch.randn(2, 2, 5, 7, generator=g)
    w, b = torch.randn(3, generator=g), torch.randn(3, generator=g)
    want = torch.cat([torch.nn.functional.gelu(torch.nn.functional.group_norm(x, 3, w, b, 1e-5)), skip], dim=1)
    assert torch.equal(WF.plane_norm_gelu(x, w, b, skip), want)
    assert torch.equal(WF.plane_norm_gelu(x, w, b), want[:, :3])
    one = WF.plane_norm_gelu(torch.zeros(2, 3, 1, 1), w, b)   # H W = 1: z = beta
    assert torch.allclose(one, torch.nn.functional.gelu(b).view(1, 3, 1, 1).expand(2, 3, 1, 1))


def test_indivisible_sizes_raise_a_value_error_that_names_the_requirement():
    net = U.build("a_")  # depth 3
    for shape in ((1, 8, 12, 16), (1, 8, 16, 20), (1, 8, 7, 8)):
        with pytest.raises(ValueError, match=r"multiples of 2\*\*depth = 8"):
            net(torch.zeros(shape))
    assert net(torch.zeros(1, 8, 8, 16)).shape == (1, 5, 8, 16)


def test_bn2d_builds_the_framework_route_and_other_norms_are_refused():
    from waldo_amd.modules import UNet
    net = UNet(4, 3, 8, "bn2d", 2, 1, False, "bilinear")
    assert isinstance(net.conv_layers[0][1].norm, torch.nn.SyncBatchNorm)
    assert "conv_layers.0.1.norm.running_mean" in net.state_dict()
    with pytest.raises(ValueError, match="norm_layer"):
        UNet(4, 3, 8, "ln", 2, 1, False, "bilinear")


def test_zero_init_zeroes_the_last_convolution_only():
    from waldo_amd.modules import UNet
    net = UNet(4, 3, 8, "ln2d", 2, 1, True, "bilinear")
    assert not net.from_emb.weight.any() and net.to_emb.weight.any() and net.deconv_layers[0][0].weight.any()
    bound = (6.0 / (4 * 9 + 4 * 9)) ** 0.5     # Xavier-uniform, gain 1, of to_emb (4 -> 4 channels, 3 x 3)
    assert net.to_emb.weight.abs().max() <= bound
    norm = net.conv_layers[0][1].norm
    assert torch.equal(norm.weight, torch.ones(8)) and not norm.bias.any()


def _opt(**over):
    from waldo_amd.tools import demo
    return demo.demo_opt(dim=16, aspect_ratio=2.0, num_obj=2, num_lyt=5, ii_embed_dim=16, ii_depth=2, **over)


@pytest.mark.parametrize("over,cin,cout,zero", [
    (dict(ii_score=True, ii_ab=True), 11, 5, True),
    (dict(ii_score=True, ii_ab=False), 11, 4, False),
    (dict(ii_score=True, ii_ab=True, use_disocc=True), 12, 5, True),
    (dict(ii_score=False, ii_ab=True, ctx_len=3), 33, 3, False),
    (dict(ii_score=False, ii_ab=False, ctx_len=4, use_disocc=True), 48, 3, False),
])
def test_with_unet_derives_the_channel_counts_as_the_reference(over, cin, cout, zero):
    from waldo_amd.nets import WIF
    opt = _opt(**over)
    wif = WIF.with_unet(opt)
    assert wif.unet.to_emb.in_channels == cin and wif.unet.from_emb.out_channels == cout
    assert wif.unet.depth == 2 and wif.unet.to_emb.out_channels == 16 // 2
    assert bool(wif.unet.from_emb.weight.any()) != zero
    assert all(k.startswith("unet.") for k in wif.state_dict())
    args = WIF.unet_arguments(opt)
    assert args["scale_hd"] == 1 and args["upmode"] == "bilinear" and args["norm_layer"] == "ln2d"
    assert WIF.unet_arguments(_opt(load_dim=64, ii_ft_hd=True))["scale_hd"] == 4.0
    assert WIF(opt).unet is None                       # the plain constructor keeps its meaning


def test_wif_step_takes_the_stand_in_by_default():
    import inspect
    from waldo_amd.tools.wif_step import WifStep, wif_opt
    assert inspect.signature(WifStep.__init__).parameters["unet"].default == "stand-in"
    o = wif_opt()
    assert (o.ii_depth, o.ii_embed_dim, o.norm_layer_patch) == (6, 512, "ln2d")
    with pytest.raises(ValueError, match="unet"):
        WifStep(1, torch.device("cpu"), unet="other")


def test_load_wif_checkpoint_strips_the_module_prefix(tmp_path):
    from waldo_amd.nets import WIF
    from waldo_amd.tools import demo
    opt = _opt()
    src = WIF.with_unet(opt)
    with torch.no_grad():
        src.unet.from_emb.weight.normal_()
    path = str(tmp_path / "ii.pth")
    torch.save({"module." + k: v for k, v in src.state_dict().items()}, path)
    dst = demo.load_wif_checkpoint(WIF.with_unet(opt), path)
    for k, v in src.state_dict().items():
        assert torch.equal(dst.state_dict()[k], v), k
    torch.save({"unet.to_emb.weight": src.unet.to_emb.weight}, path)
    with pytest.raises(RuntimeError, match="Missing key"):
        demo.load_wif_checkpoint(WIF.with_unet(opt), path)


def test_reference_wif_state_dict_loads_strictly_and_forwards_equal():
    """Live: the reference's WIF built on the CPU, its state dict loaded into ``WIF.with_unet`` strictly, equal forward
    results on one tiny clip.  Skipped where the reference tree is absent."""
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("the reference tree is not on this machine")
    from waldo_amd.nets import WIF
    ns = ref_import.load()
    for over in (dict(ii_ab=True), dict(ii_ab=False, use_disocc=True)):
        opt = _opt(**over)
        torch.manual_seed(3)
        with ref_import.cuda_is_noop():
            ref = ns.WIF(types.SimpleNamespace(**vars(opt)))
        with torch.no_grad():
            ref.unet.from_emb.weight.normal_(std=0.1)      # (zero_init would make every output the same)
        ours = WIF.with_unet(opt)
        ours.load_state_dict(ref.state_dict(), strict=True)
        c = ours.unet.to_emb.in_channels
        vid = torch.randn(1, 3, 2, c, 16, 32, generator=torch.Generator().manual_seed(4))
        with torch.no_grad():
            want = ref(vid)
            net_out = ours.unet(vid.permute(0, 2, 1, 3, 4, 5).reshape(-1, c, 16, 32))
            ref_net = ref.unet(vid.permute(0, 2, 1, 3, 4, 5).reshape(-1, c, 16, 32))
        close(net_out, ref_net, what="unet")
        if torch.cuda.is_available():  # (the fusion around the network is a kernel: there is no CPU route for it)
            with torch.no_grad():
                got = ours.cuda()(vid.cuda())
            close(got, want, what="WIF.forward")
