"""Shared by tests/test_lvd_nets_cpu.py and tests/test_gpu_lvd_nets.py: the cases of tests/golden/lvd_nets_reference.npz
(recorded from the reference's LVD networks by tools_dev/make_lvd_nets_golden.py) and how a ``waldo_amd.nets.LVD`` is
built for them and run."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lvd_nets_reference.npz")
CASES = ("a_", "b_")
OUTPUTS = ("x", "x_obj", "x_bg", "cls", "obj_pose", "bg_pose", "occ_score", "pts_rest_obj", "pts_rest_bg", "obj_alpha",
           "occ")
_data = None


def case(prefix):
    """(the option values, the parameter names in order, a dict of tensors: input, p.<key>, <output>32, <output>64)."""
    global _data
    if _data is None:
        _data = np.load(GOLDEN)
    d = {k[len(prefix):]: torch.from_numpy(_data[k]) for k in _data.files
         if k.startswith(prefix) and k not in (prefix + "keys", prefix + "opt")}
    d["input"] = d["input"].float()   # (stored in 16 bits, exactly)
    return json.loads(str(_data[prefix + "opt"])), [str(k) for k in _data[prefix + "keys"]], d


def build(prefix, device="cpu", fused=True, dtype=torch.float32):
    """The package's LVD for the case's options with the recorded parameters loaded STRICTLY, next to the buffers the
    module built for itself (the fixture holds none)."""
    from waldo_amd.nets import LVD, lvd_net_opt
    opt, keys, d = case(prefix)
    net = LVD(lvd_net_opt(**opt))
    state = net.state_dict()
    assert not set(keys) - set(state), sorted(set(keys) - set(state))
    state.update({k: d["p." + k] for k in keys})
    net.load_state_dict(state, strict=True)
    net.fused = fused
    return net.to(device=device, dtype=dtype).eval()


def run(net, inp, ctx_len):
    """The 11 recorded outputs, by name: the modes in front of the Warper, ``decoder(x_obj)`` and ``compute_occ``."""
    x = net(input=inp, mode="encode_input")
    x_obj, x_bg, cls = net(x=x[:, :ctx_len], mode="estimate_layer")
    obj_pose, bg_pose, occ_score, rest_obj, rest_bg, _, _ = net(x=x, x_obj=x_obj, x_bg=x_bg, mode="estimate_pose")
    vals = (x, x_obj, x_bg, cls, obj_pose, bg_pose, occ_score, rest_obj, rest_bg, net.decoder(x_obj),
            net.compute_occ(occ_score))
    return dict(zip(OUTPUTS, vals))


def check(close, got, d, what):
    for name in OUTPUTS:
        close(got[name], d[name + "32"], exact=d[name + "64"], what=f"{what} {name}")
