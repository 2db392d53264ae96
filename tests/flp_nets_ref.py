"""Shared by tests/test_flp_nets_cpu.py and tests/test_gpu_flp_nets.py: the cases of tests/golden/flp_nets_reference.npz
(recorded from the reference's FLP networks by tools_dev/make_flp_nets_golden.py) and how a ``waldo_amd.nets.FLP`` is built
for them and run."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flp_nets_reference.npz")
CASES = ("a_", "b_", "all_", "nocatz_", "last_", "free_")
NOISE = ("embed", "inject", "modulate")
INPUTS = ("obj_pose", "bg_pose", "occ_score", "x_obj", "x_bg", "last_obj", "last_bg")
OUTPUTS = ("obj_pose", "bg_pose", "occ_score")
_data = None


def data():
    global _data
    if _data is None:
        _data = np.load(GOLDEN)
    return _data


def case(prefix):
    """(the option values, the parameter names in order, a dict of tensors: in.<input>, ctx_mask, p.<key>,
    <output>32, <output>64); the parameters of a case that shares another's are that case's."""
    f = data()
    d = {k[len(prefix):]: torch.from_numpy(f[k]) for k in f.files
         if k.startswith(prefix) and k[len(prefix):] not in ("keys", "state_keys", "opt", "params_of")}
    if prefix + "params_of" in f.files:
        owner = str(f[prefix + "params_of"])
        d.update({k[len(owner):]: torch.from_numpy(f[k]) for k in f.files if k.startswith(owner + "p.")})
    for k in list(d):
        if k.startswith(("in.", "p.")):
            d[k] = d[k].float()   # (stored in 16 bits, exactly)
    return json.loads(str(f[prefix + "opt"])), [str(k) for k in f[prefix + "keys"]], d


def build(prefix, device="cpu", fused=True, dtype=torch.float32):
    """The package's FLP for the case's options with the recorded parameters loaded STRICTLY, next to the buffers the
    module built for itself (the fixture holds none; their names are checked against the recorded state keys)."""
    from waldo_amd.nets import FLP, flp_net_opt
    opt, keys, d = case(prefix)
    net = FLP(flp_net_opt(**opt))
    state = net.state_dict()
    assert list(state) == [str(k) for k in data()[prefix + "state_keys"]]
    assert [k for k, _ in net.named_parameters()] == keys
    state.update({k: d["p." + k] for k in keys})
    net.load_state_dict(state, strict=True)
    net.fused = fused
    return net.to(device=device, dtype=dtype).eval()


def inputs(d, device="cpu", dtype=torch.float32):
    return [d["in." + k].to(device=device, dtype=dtype) for k in INPUTS]


def run(net, d, device="cpu", dtype=torch.float32, ctx_mask=None):
    """The three outputs, by name, under the recorded mask (or ``ctx_mask``: a plan)."""
    mask = d["ctx_mask"].to(device) if ctx_mask is None else ctx_mask
    return dict(zip(OUTPUTS, net(*inputs(d, device, dtype), ctx_mask=mask)))


def check(close, got, d, what):
    for name in OUTPUTS:
        close(got[name], d[name + "32"], exact=d[name + "64"], what=f"{what} {name}")
