"""CPU: ``WF.lpips_level`` off the kernel route, the ``LPIPS`` module's layout, loading and forward against the plain
restatement (tests/lpips_ref.py), and the argument checks of the metric and of ``WifStep`` that come before the device."""
import pytest
import torch

import lpips_ref as R
from parity import close


@pytest.fixture(scope="module")
def modules():
    from waldo_amd.nets import LPIPS
    torch.manual_seed(5)
    return {net: LPIPS(net) for net in ("vgg", "alex")}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_lpips_level_on_the_cpu_is_the_chain(dtype):
    from waldo_amd import functional as WF
    f0, f1, w = R.features((3, 5, 7, 9), 1, dtype=dtype)
    f0.requires_grad_()
    f1.requires_grad_()
    w4 = w.view(1, -1, 1, 1).clone().requires_grad_()       # the lin weight as the module holds it; trainable here
    got = WF.lpips_level(f0, f1, w4)
    assert got.shape == (3,) and got.dtype == dtype
    grads = torch.autograd.grad(got.sum(), (f0, f1, w4))

    def chain(dt):
        x0, x1, xw = (t.detach().to(dt).requires_grad_() for t in (f0, f1, w))
        out = R.level(x0, x1, xw)
        return (out.detach(),) + torch.autograd.grad(out.sum(), (x0, x1, xw))

    same, exact = chain(dtype), chain(torch.float64)
    for i, name in enumerate(("out", "grad_f0", "grad_f1", "grad_w")):
        g = got.detach() if i == 0 else grads[i - 1].reshape(same[i].shape)
        close(g, same[i], rel=True, exact=exact[i], what=f"cpu {dtype} {name}")
    assert torch.equal(WF.lpips_level(f0, f0.clone(), w), torch.zeros(3, dtype=dtype))


def test_lpips_level_argument_errors_before_the_device():
    from waldo_amd import functional as WF
    f = torch.rand(2, 5, 3, 4)
    w = torch.rand(5)
    for bad in (torch.rand(2, 5, 12), torch.rand(5, 3, 4), torch.rand(2, 5, 3, 4, 1)):
        with pytest.raises(ValueError, match=r"\(N, C, H, W\)"):
            WF.lpips_level(bad, bad, w)
    with pytest.raises(ValueError, match=r"\(N, C, H, W\)"):
        WF.lpips_level(f, f.long(), w)
    with pytest.raises(ValueError, match="disagree"):
        WF.lpips_level(f, torch.rand(2, 5, 4, 3), w)
    with pytest.raises(ValueError, match="disagree"):
        WF.lpips_level(f, f.double(), w)
    for bad_w in (torch.rand(4), torch.rand(1, 6, 1, 1), torch.rand(5).double(), [0.1] * 5):
        with pytest.raises(ValueError, match="C = 5"):
            WF.lpips_level(f, f, bad_w)
    with pytest.raises(ValueError, match="empty"):
        WF.lpips_level(f[:0], f[:0], w)


@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_state_dict_is_the_packages_layout(modules, net):
    state = modules[net].state_dict()
    want = R.expected_shapes(net)
    assert set(state) == set(want), set(state) ^ set(want)
    for name, shape in want.items():
        assert tuple(state[name].shape) == shape, name
    assert torch.equal(state["scaling_layer.shift"].flatten(), torch.tensor(R.SHIFT))
    assert torch.equal(state["scaling_layer.scale"].flatten(), torch.tensor(R.SCALE))
    for k in range(5):
        assert (state[f"lin{k}.model.1.weight"] >= 0).all()
    m = modules[net]
    assert not m.training and not any(p.requires_grad for p in m.parameters())
    assert m.train() is m and not m.training and not any(s.training for s in m.modules())


@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_strict_loading_of_both_file_forms(modules, net, tmp_path):
    from waldo_amd.nets import LPIPS
    src = modules[net]
    state = {k: v.clone() for k, v in src.state_dict().items()}
    full = dict(state, **{f"lins.{k}.model.1.weight": state[f"lin{k}.model.1.weight"] for k in range(5)})
    path = tmp_path / "full.pth"
    torch.save(full, path)
    for given in (state, full, str(path)):
        loaded = LPIPS.load(net, state=given)
        for k, v in loaded.state_dict().items():
            assert torch.equal(v, state[k]), k
    # the two-file form: torchvision's backbone (with its classifier) and the package's lin file
    backbone = {"classifier.1.weight": torch.zeros(3, 3), "classifier.1.bias": torch.zeros(3)}
    for name, v in state.items():
        if name.startswith("net."):
            _, _, idx, leaf = name.split(".")
            backbone[f"features.{idx}.{leaf}"] = v
    lin = {k: v for k, v in state.items() if k.startswith("lin")}
    torch.save(backbone, tmp_path / "backbone.pth")
    torch.save(lin, tmp_path / "lin.pth")
    for b, l in ((backbone, lin), (str(tmp_path / "backbone.pth"), str(tmp_path / "lin.pth"))):
        loaded = LPIPS.load(net, backbone=b, lin=l)
        for k, v in loaded.state_dict().items():
            assert torch.equal(v, state[k]), k
    # unknown and missing keys are named
    with pytest.raises(KeyError, match="net.slice9.0.weight"):
        LPIPS.load(net, state=dict(state, **{"net.slice9.0.weight": torch.zeros(1)}))
    with pytest.raises(KeyError, match="missing key 'lin3.model.1.weight'"):
        LPIPS.load(net, state={k: v for k, v in state.items() if k != "lin3.model.1.weight"})
    with pytest.raises(KeyError, match="lins.2.model.1.weight"):
        LPIPS.load(net, state=dict(full, **{"lins.2.model.1.weight": full["lins.2.model.1.weight"] + 1}))
    with pytest.raises(KeyError, match="features.1.weight"):
        LPIPS.load(net, backbone=dict(backbone, **{"features.1.weight": torch.zeros(1)}), lin=lin)
    with pytest.raises(KeyError, match="avgpool.weight"):
        LPIPS.load(net, backbone=dict(backbone, **{"avgpool.weight": torch.zeros(1)}), lin=lin)
    with pytest.raises(KeyError, match="missing key 'net.slice1.0.bias'"):
        LPIPS.load(net, backbone={k: v for k, v in backbone.items() if k != "features.0.bias"}, lin=lin)
    with pytest.raises(KeyError, match="lin7.model.1.weight"):
        LPIPS.load(net, backbone=backbone, lin=dict(lin, **{"lin7.model.1.weight": torch.zeros(1)}))
    with pytest.raises(KeyError, match="missing key 'lin0.model.1.weight'"):
        LPIPS.load(net, backbone=backbone, lin={k: v for k, v in lin.items() if k != "lin0.model.1.weight"})
    with pytest.raises(KeyError, match="shape"):
        LPIPS.load(net, state=dict(state, **{"lin0.model.1.weight": torch.zeros(1, 3, 1, 1)}))
    with pytest.raises(ValueError, match="either"):
        LPIPS.load(net)
    with pytest.raises(ValueError, match="either"):
        LPIPS.load(net, backbone=backbone)
    with pytest.raises(ValueError, match="either"):
        LPIPS.load(net, state=state, lin=lin)


@pytest.mark.parametrize("net,shape", [("vgg", (2, 3, 32, 48)), ("alex", (2, 3, 64, 64))])
def test_forward_on_the_cpu_is_the_restatement(modules, net, shape):
    m = modules[net]
    g = torch.Generator().manual_seed(11)
    in0 = torch.rand(*shape, generator=g) * 2 - 1
    in1 = (in0 + 0.3 * torch.randn(*shape, generator=g)).clamp(-1, 1)
    state = m.state_dict()
    got = m(in0, in1)
    assert got.shape == (2, 1, 1, 1) and got.dtype == torch.float32
    want = R.lpips(net, state, in0.double(), in1.double())
    assert (want > 0).all()
    close(got, R.lpips(net, state, in0, in1), rel=True, exact=want, what=f"cpu {net}")
    u0, u1 = (in0 + 1) / 2, (in1 + 1) / 2
    close(m(u0, u1, normalize=True), R.lpips(net, state, u0, u1, True), rel=True,
          exact=R.lpips(net, state, u0.double(), u1.double(), True), what=f"cpu {net} normalize")
    assert torch.equal(m(in0, in0.clone()), torch.zeros(2, 1, 1, 1))


def test_chunking_does_not_change_an_image(modules):
    from waldo_amd.nets import LPIPS
    g = torch.Generator().manual_seed(3)
    in0 = torch.rand(3, 3, 64, 64, generator=g) * 2 - 1
    in1 = torch.rand(3, 3, 64, 64, generator=g) * 2 - 1
    state = modules["alex"].state_dict()
    # the framework's own convolution works image by image: chunking leaves every bit where it was
    with torch.backends.mkldnn.flags(enabled=False):
        whole = LPIPS.load("alex", state=state, chunk=8)(in0, in1)
        for chunk in (1, 2):
            pieces = LPIPS.load("alex", state=state, chunk=chunk)(in0, in1)
            assert pieces.shape == (3, 1, 1, 1) and torch.equal(pieces, whole), chunk
    # oneDNN picks its blocking by the batch size, so its sums are taken in another order (2e-9 of a value of 1e-5
    # when this was written): equal within the fp32 chain's own distance from the fp64 restatement
    want = R.lpips("alex", state, in0.double(), in1.double())
    whole = LPIPS.load("alex", state=state, chunk=8)(in0, in1)
    for chunk in (1, 2):
        pieces = LPIPS.load("alex", state=state, chunk=chunk)(in0, in1)
        close(pieces, whole, rel=True, exact=want, what=f"chunk {chunk} against 8")
    single = LPIPS.load("alex", state=state, chunk=1)
    for i in range(3):  # an image alone is what it is in a chunk of one
        assert torch.equal(single(in0, in1)[i], single(in0[i:i + 1], in1[i:i + 1])[0])


def test_module_argument_errors():
    from waldo_amd.nets import LPIPS
    with pytest.raises(ValueError, match="squeeze"):
        LPIPS("squeeze")
    with pytest.raises(ValueError, match="spatial"):
        LPIPS("alex", spatial=True)
    with pytest.raises(ValueError, match="chunk"):
        LPIPS("alex", chunk=0)
    m = LPIPS("alex")
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match=r"\(N, 3, H, W\)"):
        m(torch.zeros(1, 4, 64, 64), torch.zeros(1, 4, 64, 64))
    with pytest.raises(ValueError, match=r"\(N, 3, H, W\)"):
        m(x[0], x[0])
    with pytest.raises(ValueError, match="differ in shape"):
        m(x, torch.zeros(2, 3, 64, 64))


def test_the_metric_is_refused_without_a_module_and_checked_with_one(modules):
    from waldo_amd import functional as WF
    from waldo_amd._lib import WaldoHipError
    from waldo_amd.metrics import check_metrics, frame_metrics
    x = torch.zeros(1, 2, 3, 64, 64)
    with pytest.raises(ValueError, match="not available: it needs the pretrained AlexNet and LPIPS linear-layer weights"):
        frame_metrics(x, x, metrics=("lpips",))
    with pytest.raises(ValueError, match="weights"):
        check_metrics(("psnr", "lpips"))
    assert check_metrics(("psnr", "lpips"), modules["alex"]) == ("psnr", "lpips")
    with pytest.raises(ValueError, match="LPIPS module"):
        check_metrics(("lpips",), "alex")
    with pytest.raises(WaldoHipError, match="GPU"):                      # what the other metrics raise on the CPU
        frame_metrics(x, x, metrics=("lpips",), lpips=modules["alex"])
    with pytest.raises(WaldoHipError, match="GPU"):
        frame_metrics(x.to(torch.uint8), x.to(torch.uint8), metrics=("psnr", "lpips"), lpips=modules["alex"])
    packed = WF.PackedClip(torch.zeros(1, 2, 64, 64, 4, dtype=torch.uint8), 5)
    with pytest.raises(ValueError, match="PackedClip"):
        frame_metrics(x, packed, metrics=("lpips",), lpips=modules["alex"])
    with pytest.raises(ValueError, match="unknown metric"):
        frame_metrics(x, x, metrics=("lpips", "fid"), lpips=modules["alex"])
    with pytest.raises(ValueError, match="differ in shape"):
        frame_metrics(x, torch.zeros(1, 2, 3, 64, 65), metrics=("lpips",), lpips=modules["alex"])


def test_wif_step_argument_checks():
    from waldo_amd.tools.wif_step import WifStep
    dev = torch.device("cpu")
    with pytest.raises(ValueError, match="objective must be 'sharp' or 'recipe'"):
        WifStep(1, dev, objective="lpips")
    with pytest.raises(ValueError, match="needs objective='recipe'"):
        WifStep(1, dev, lpips=torch.nn.Identity())
    with pytest.raises(ValueError, match="LPIPS module"):
        WifStep(1, dev, objective="recipe", lpips=torch.nn.Identity())
    with pytest.raises(ValueError, match="unet must be"):               # the earlier checks still stand
        WifStep(1, dev, unet="big", objective="recipe")
