"""Shared by tests/test_unet_cpu.py and tests/test_gpu_unet.py: the cases of tests/golden/unet_reference.npz (recorded from
the reference's UNet by tools_dev/make_unet_golden.py) and how a ``waldo_amd.modules.UNet`` is run on them."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_reference.npz")
CASES = ("a_", "b_")
_data = None


def case(prefix):
    """cfg (cin, cout, embed, depth, N, H, W), the key list, and a dict of tensors: x, grad_out, out32/64, gx32/64,
    sd.<key>, g32.<key>, g64.<key>."""
    global _data
    if _data is None:
        _data = np.load(GOLDEN)
    d = {k[len(prefix):]: torch.from_numpy(_data[k]) for k in _data.files
         if k.startswith(prefix) and k not in (prefix + "keys", prefix + "cfg")}
    return [int(v) for v in _data[prefix + "cfg"]], [str(k) for k in _data[prefix + "keys"]], d


def build(prefix, device="cpu", fused=True):
    """The package's UNet at the case's widths with the recorded state dict loaded strictly."""
    from waldo_amd.modules import UNet
    (cin, cout, embed, depth, _, _, _), keys, d = case(prefix)
    net = UNet(cin, cout, embed, "ln2d", depth, 1, False, "bilinear")
    net.load_state_dict({k: d["sd." + k] for k in keys}, strict=True)
    net.fused = fused
    return net.to(device)


def run(net, x, grad_out):
    """(out, grad_x, {key: parameter gradient}) of one forward + backward."""
    net.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_()
    out = net(x)
    out.backward(grad_out)
    return out.detach(), x.grad, {k: p.grad for k, p in net.named_parameters()}


def check(close, got, d, keys, what):
    """Output, input gradient and every parameter gradient against the recorded fp32 results, the fp64 ones as exact."""
    out, gx, gp = got
    close(out, d["out32"], rel=True, exact=d["out64"], what=f"{what} out")
    close(gx, d["gx32"], rel=True, exact=d["gx64"], what=f"{what} grad_x")
    assert sorted(gp) == sorted(keys)
    for k in keys:
        close(gp[k], d["g32." + k], rel=True, exact=d["g64." + k], what=f"{what} grad {k}")
