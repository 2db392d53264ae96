"""CPU: the option switches of the LVD estimators (models/nets/lvd.py:346-460, 920-950), one at a time on a 16-wide
network with ``fused = False``, against what the reference's own module computes with each
(tests/golden/lvd_nets_variants.npz, recorded by tools_dev/make_lvd_nets_golden.py); and the settings the reference
itself cannot run (``has_bg`` off, ``pe_pts_mode "head"``), for shapes.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

import lvd_nets_ref as R
from parity import close

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lvd_nets_variants.npz")
DATA = np.load(GOLDEN)
NAMES = [str(n) for n in DATA["names"]]
EXTRA = ("last_obj", "last_bg")


def field(name, key):
    """A variant's own array ``<name>.<key>``, or None where the file holds none: an output that is None in the
    reference, or one left out because the variant shares it (``build`` resolves ``params_of`` / ``input_of``)."""
    own = f"{name}.{key}"
    return DATA[own] if own in DATA.files else None


def build(name):
    from waldo_amd.nets import LVD, lvd_net_opt
    opt = json.loads(str(DATA[name + ".opt"]))
    keys = [str(k) for k in DATA[name + ".keys"]]
    src = str(DATA[name + ".params_of"])[:-1] if name + ".params_of" in DATA.files else name
    net = LVD(lvd_net_opt(**opt))
    assert [k for k, _ in net.named_parameters()] == keys
    state = net.state_dict()
    state.update({k: torch.from_numpy(DATA[f"{src}.p.{k}"]) for k in keys})
    net.load_state_dict(state, strict=True)
    net.fused = False
    isrc = str(DATA[name + ".input_of"])[:-1] if name + ".input_of" in DATA.files else name
    return opt, net.eval(), torch.from_numpy(DATA[isrc + ".input"]).float(), src != name


def run(net, inp, ctx_len):
    x = net(input=inp, mode="encode_input")
    x_obj, x_bg, cls = net(x=x[:, :ctx_len], mode="estimate_layer")
    pose = net(x=x, x_obj=x_obj, x_bg=x_bg, mode="estimate_pose")
    vals = (x, x_obj, x_bg, cls, *pose[:5], net.decoder(x_obj), net.compute_occ(pose[2]), *pose[5:])
    return dict(zip(R.OUTPUTS + EXTRA, vals))


def test_the_recorded_variants_cover_the_switches():
    assert {"occ_bias", "occ_normalize", "occ_freeze", "fix_bg", "fix_bg1", "hard_bound", "soft_bound", "norm_scale",
            "bound_scale", "decompose_embed", "no_cls", "no_delta", "use_last", "decoder_prior", "circle_bias",
            "pixel_norm", "ln_not_affine", "decoder_zero", "patch8", "patch16", "use_hr"} <= set(NAMES)


def test_patch_projection_stacks_at_the_recorded_patch_sizes():
    """patch_size 8 and 16 and the high-resolution stack: the norm -> GELU steps the patch-4 cases do not have (their
    names are compared with the reference's in ``build``, their values in the test below)."""
    for name, enc_steps, dec_steps in (("patch8", 1, 2), ("patch16", 2, 3)):
        keys = [str(k) for k in DATA[name + ".keys"]]
        assert sum(k.startswith("encoder.from_img.layers.") and k.endswith(".1.norm.weight") for k in keys) == enc_steps
        assert sum(k.startswith("decoder.to_img.layers.") and k.endswith(".1.norm.weight") for k in keys) == dec_steps
    keys = [str(k) for k in DATA["use_hr.keys"]]
    assert "encoder.from_img.hr_proj.weight" in keys and "decoder.to_img.hr_proj.weight" in keys
    assert any(k.startswith("decoder.to_img.hr_layers.0.1.norm") for k in keys)


@pytest.mark.parametrize("name", NAMES)
def test_variant_against_the_reference(name):
    opt, net, inp, shares_base = build(name)
    with torch.no_grad():
        got = run(net, inp, opt["ctx_len"])
    for out in R.OUTPUTS + EXTRA:
        ref32, ref64 = field(name, out + "32"), field(name, out + "64")
        if ref32 is None:
            # None in the reference -- or the encoder's output of a variant that shares the base's parameters and input
            if out == "x" and shares_base:
                close(got[out], torch.from_numpy(DATA["base.x32"]), exact=torch.from_numpy(DATA["base.x64"]), what="x")
            else:
                assert got[out] is None, out
            continue
        close(got[out], torch.from_numpy(ref32), exact=torch.from_numpy(ref64), what=f"{name} {out}")
    if name != "base":   # the switch does something: an output appears, vanishes or differs from the base's
        def differs(k):
            a, b = field(name, k + "32"), field("base", k + "32")
            if k == "x" and shares_base:
                return False
            return (a is None) != (b is None) or a is not None and (a.shape != b.shape or not np.array_equal(a, b))
        assert any(differs(k) for k in R.OUTPUTS + EXTRA), name


def test_settings_the_reference_cannot_run():
    """``has_bg`` off (its LayerEstimator reshapes a None) and ``pe_pts_mode "head"`` (its PoseEstimator registers an
    unset ``mul``): served here, checked for shapes and finiteness."""
    from waldo_amd.nets import LVD, lvd_net_opt
    base = json.loads(str(DATA["base.opt"]))
    inp = torch.from_numpy(DATA["base.input"]).float()
    for over in (dict(has_bg=False), dict(has_bg=False, pe_pts_mode="head")):
        torch.manual_seed(7)
        net = LVD(lvd_net_opt(**{**base, **over})).eval()
        net.fused = False
        with torch.no_grad():
            got = run(net, inp, base["ctx_len"])
        assert got["x_bg"] is None and got["bg_pose"] is None and got["pts_rest_bg"] is None
        assert got["obj_pose"].shape == (1, 5, 2, 4, 2) and torch.isfinite(got["obj_pose"]).all()
        assert got["occ_score"].shape == (1, 5, 2) and got["cls"].shape == (1, 2, 3)
    with pytest.raises(ValueError, match="has_bg"):
        LVD(lvd_net_opt(**{**base, "pe_pts_mode": "head"}))
