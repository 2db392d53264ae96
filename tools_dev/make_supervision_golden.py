"""Writes tests/golden/flow_edges_reference.npz: what the reference's own ``EdgeExtractor`` (models/modules/edge.py)
returns for small seeded flows at kernel sizes 3, 7 and 15 and, at 15 (the recipe's ``--s_edge_size``), for the committed
real flow tests/golden/demo_flow.flo -- the fixture of tests/test_supervision_cpu.py and tests/test_gpu_supervision.py.
Data only.

    python tools_dev/make_supervision_golden.py [REFERENCE_ROOT]

Needs the reference tree (default /root/reference, or $WALDO_REFERENCE_ROOT); no test runs it.  The reference's file is
executed from where it lies, with two things put in place first:
  * ``tools.utils`` as a module that holds the reference's own ``flatten`` / ``unflatten`` (tools/utils.py:54-68, compiled
    from that file's text on the fly): importing the whole file would pull in torchvision, scipy and matplotlib, none of
    which those two functions use;
  * the module's name ``F``: edge.py calls ``F.conv2d`` without importing ``F``; it is set to ``torch.nn.functional``,
    which is what the name means everywhere else in the reference.
(The loading is done here and not through the test suite's reference-import harness: development scripts stay clear of
that package -- tests/test_abi.py.)"""
import ast
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "flow_edges_reference.npz")
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("WALDO_REFERENCE_ROOT", "/root/reference")
KERNELS = (3, 7, 15)
SEED = 20261018


def load_edge_extractor(ref=REF):
    """The reference's EdgeExtractor class, with the stand-ins of the module docstring in place."""
    sys.dont_write_bytecode = True
    path = os.path.join(ref, "tools", "utils.py")
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("flatten", "unflatten")]
    assert len(keep) == 2, [n.name for n in keep]
    utils = types.ModuleType("tools.utils")
    utils.__dict__.update(torch=torch, mul=__import__("operator").mul, reduce=__import__("functools").reduce)
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), utils.__dict__)
    tools = types.ModuleType("tools")
    tools.utils = utils
    saved = {k: sys.modules.get(k) for k in ("tools", "tools.utils")}
    sys.modules["tools"], sys.modules["tools.utils"] = tools, utils
    try:
        spec = importlib.util.spec_from_file_location("_reference_edge", os.path.join(ref, "models", "modules", "edge.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    mod.F = torch.nn.functional
    return mod.EdgeExtractor


def seeded_flow():
    """(2, 3, 2, 24, 40): a smooth field plus noise, in the normalised units of a real flow."""
    rng = np.random.default_rng(SEED)
    ys, xs = np.meshgrid(np.linspace(-1, 1, 24), np.linspace(-1, 1, 40), indexing="ij")
    base = np.stack([0.03 * np.sin(3 * xs + ys), 0.02 * np.cos(2 * ys - xs)])
    return (base[None, None] * rng.uniform(0.5, 1.5, (2, 3, 1, 1, 1)) + 0.004 * rng.standard_normal((2, 3, 2, 24, 40))
            ).astype(np.float32)


def read_flo(path):
    """A Middlebury .flo file as (2, H, W) in normalised units (the reference's data/base_dataset.py:185-203)."""
    with open(path, "rb") as fh:
        assert fh.read(4) == b"PIEH"
        w, h = (int(v) for v in np.frombuffer(fh.read(8), np.int32))
        flow = np.frombuffer(fh.read(w * h * 8), np.float32).reshape(h, w, 2).transpose(2, 0, 1).copy()
    flow[0] = 2.0 * flow[0] / w
    flow[1] = 2.0 * flow[1] / h
    return flow


def main():
    Edge = load_edge_extractor()
    out = {"flow": seeded_flow()}
    with torch.no_grad():
        for k in KERNELS:
            edge, dominant = Edge(k)(torch.from_numpy(out["flow"]))
            out[f"edge_k{k}"], out[f"dominant_k{k}"] = edge.numpy(), dominant.numpy().astype(np.uint8)
        real = read_flo(os.path.join(ROOT, "tests", "golden", "demo_flow.flo"))[None]
        edge, dominant = Edge(15)(torch.from_numpy(real))
        out["real_edge_k15"], out["real_dominant_k15"] = edge.numpy(), dominant.numpy().astype(np.uint8)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    for name, v in out.items():
        print(f"  {name}: {v.dtype} {v.shape}")


if __name__ == "__main__":
    main()
