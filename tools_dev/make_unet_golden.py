"""Writes tests/golden/unet_reference.npz: what the reference's own ``UNet`` (models/modules/conv.py) computes on small
seeded inputs -- the fixture of tests/test_unet_cpu.py and tests/test_gpu_unet.py.  Data only.

    python tools_dev/make_unet_golden.py [REFERENCE_ROOT]

Needs the reference tree (default /root/reference, or $WALDO_REFERENCE_ROOT); no test runs it.  The reference's files
are executed from where they lie, under stub parents ``models`` / ``models.modules`` and a stub ``tools.utils`` (the
norm file imports two helpers from it that a UNet never calls; the real file would pull in torchvision).  (The loading
is done here and not through the test suite's reference-import harness: development scripts stay clear of that
package -- tests/test_abi.py.)

Per case (prefix ``a_``, ``b_``): ``cfg`` = (cin, cout, embed, depth, N, H, W); ``keys`` = the state dict's keys in
order; ``sd.<key>`` the state dict, with the norm affines moved away from 1 / 0 so that they matter; ``x`` and a seeded
``grad_out``; ``out32``, ``gx32``, ``g32.<key>`` = the output, the input gradient and every parameter gradient of the
fp32 network, ``out64``, ``gx64``, ``g64.<key>`` = the same network run in fp64 on the same values.  No case has a bottom
plane of fewer than 8 values: below that the reference's own fp32 gradients are 1e-4 of their scale from fp64."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "unet_reference.npz")
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("WALDO_REFERENCE_ROOT", "/root/reference")
SEED = 20261018
# (cin, cout, embed, depth, N, H, W)
CASES = {"a_": (8, 5, 16, 3, 2, 16, 32), "b_": (6, 4, 8, 2, 3, 8, 12)}


def load_unet(ref=REF):
    """The reference's UNet class, with the stand-ins of the module docstring in place while its files execute."""
    sys.dont_write_bytecode = True
    names = ("tools", "tools.utils", "models", "models.modules", "models.modules.spectral",
             "models.modules.weight_init", "models.modules.transform", "models.modules.conv")
    saved = {k: sys.modules.get(k) for k in names}
    try:
        tools, utils = types.ModuleType("tools"), types.ModuleType("tools.utils")
        utils.from_ctx = utils.to_ctx = None
        tools.utils = utils
        models, modules = types.ModuleType("models"), types.ModuleType("models.modules")
        models.__path__ = [os.path.join(ref, "models")]
        modules.__path__ = [os.path.join(ref, "models", "modules")]
        sys.modules.update({"tools": tools, "tools.utils": utils, "models": models, "models.modules": modules})
        for name in ("spectral", "weight_init", "transform", "conv"):
            spec = importlib.util.spec_from_file_location(f"models.modules.{name}",
                                                          os.path.join(ref, "models", "modules", name + ".py"))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[spec.name] = mod
            spec.loader.exec_module(mod)
        return mod.UNet
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def run(net, x, grad_out):
    x = x.clone().requires_grad_()
    out = net(x)
    out.backward(grad_out)
    return out.detach(), x.grad, {k: p.grad for k, p in net.named_parameters()}


def main():
    UNet = load_unet()
    res = {}
    for prefix, (cin, cout, embed, depth, n, h, w) in CASES.items():
        torch.manual_seed(SEED + len(res))
        net = UNet(cin, cout, embed, "ln2d", depth, 1, False, "bilinear")
        g = torch.Generator().manual_seed(SEED + 1 + len(res))
        with torch.no_grad():
            for k, p in net.named_parameters():
                if k.endswith(".norm.weight"):
                    p.copy_(1 + 0.3 * torch.randn(p.shape, generator=g))
                elif k.endswith(".norm.bias"):
                    p.copy_(0.2 * torch.randn(p.shape, generator=g))
        x = torch.randn(n, cin, h, w, generator=g)
        grad_out = torch.randn(n, cout, h, w, generator=g)
        sd = net.state_dict()
        assert set(sd) == {k for k, _ in net.named_parameters()}, "the state dict holds parameters only"
        net64 = UNet(cin, cout, embed, "ln2d", depth, 1, False, "bilinear").double()
        net64.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
        out32, gx32, g32 = run(net, x, grad_out)
        out64, gx64, g64 = run(net64, x.double(), grad_out.double())
        res[prefix + "cfg"] = np.array([cin, cout, embed, depth, n, h, w], np.int64)
        res[prefix + "keys"] = np.array(list(sd.keys()))
        res[prefix + "x"], res[prefix + "grad_out"] = x.numpy(), grad_out.numpy()
        res[prefix + "out32"], res[prefix + "out64"] = out32.numpy(), out64.numpy()
        res[prefix + "gx32"], res[prefix + "gx64"] = gx32.numpy(), gx64.numpy()
        for k, v in sd.items():
            res[f"{prefix}sd.{k}"] = v.numpy()
            res[f"{prefix}g32.{k}"], res[f"{prefix}g64.{k}"] = g32[k].numpy(), g64[k].numpy()
        print(f"{prefix}: |out| {out32.abs().max():.3g}  |out32 - out64| {(out32 - out64).abs().max():.2e}   "
              f"|gx| {gx32.abs().max():.3g}  |gx32 - gx64| {(gx32 - gx64).abs().max():.2e}")
        for k in sd:
            rel = (g32[k] - g64[k]).abs().max() / g64[k].abs().max()
            print(f"    {k}: |g| {g64[k].abs().max():.3g}  rel fp32 error {rel:.2e}")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **res)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
