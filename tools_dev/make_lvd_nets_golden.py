"""Writes tests/golden/lvd_nets_reference.npz: what the reference's own ``LVD`` networks (models/nets/lvd.py: ImageEncoder,
LayerEstimator, PoseEstimator, ImageDecoder and the transformer blocks of models/modules/transform.py) compute on small
seeded inputs -- the fixture of tests/test_lvd_nets_cpu.py and tests/test_gpu_lvd_nets.py.  Data only.

    python tools_dev/make_lvd_nets_golden.py [REFERENCE_ROOT]

Needs the reference tree (default /root/reference, or $WALDO_REFERENCE_ROOT); no test runs it.  The reference's files are
executed from where they lie, under stub parents ``models`` / ``models.modules`` / ``models.nets`` / ``tools`` and an
empty stand-in for torchvision, which its tools/utils.py imports and these networks never call.  (The loading is done
here and not through the test suite's reference-import harness: development scripts stay clear of that package --
tests/test_abi.py.)

Per case (prefix ``a_``, ``b_``): ``opt`` = the option values as JSON; ``keys`` = the parameter names in order;
``p.<key>`` the parameters (buffers are not stored: a drop-in builds its own); ``input`` (B, T, C, H, W), values that
16 bits hold exactly, stored so; and for each of the 11 outputs ``<name>32`` / ``<name>64``, the fp32 network's value
and that of the same network in fp64 on the same values: x, x_obj, x_bg, cls, obj_pose, bg_pose, occ_score,
pts_rest_obj, pts_rest_bg, obj_alpha (= decoder(x_obj)),
occ (= compute_occ(occ_score)).  The fp64 run stops in front of Warper.forward (its InverseWarp mixes an fp32 mask into
an fp64 kernel and raises).

A second file, tests/golden/lvd_nets_variants.npz, holds the same record for ``VARIANTS``: the option switches of the
estimators one at a time on a 16-wide base (prefix ``<name>.``; ``names`` lists them; a variant whose parameters are the
base's stores ``params_of`` instead of them; ``last_obj`` / ``last_bg`` where ``use_last_pose_decoder`` makes them; an
output that is None in the reference is absent).

Freshly initialised weights give nearly uniform attention, which would test nothing: the q / kv / qkv weights are
scaled by 12 and the embeddings by 25, the norm affines and the zero-initialised heads are moved off 1 / 0, and the
script asserts that the logits of EVERY attention of the two full cases have a standard deviation in [1.5, 6]."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "lvd_nets_reference.npz")
OUT_VARIANTS = os.path.join(ROOT, "tests", "golden", "lvd_nets_variants.npz")
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("WALDO_REFERENCE_ROOT", "/root/reference")
SEED = 20261019
B, T = 2, 5
COMMON = dict(dim=8, aspect_ratio=2, patch_size=4, latent_shape=[2, 4], obj_shape=[2, 2], input_rgb=False,
              input_lyt=True, input_flow=True, ctx_len=4, has_bg=True, bound_rest=True, soft_bound_rest=True,
              circle_translate_bias=True, pred_cls=True, pe_decoder_init_mode="five", pad_obj_alpha=1)
CASES = {"a_": dict(embed_dim=32, num_heads=2, num_obj=3, num_lyt=5, oe_depth=2, pe_depth=2),
         "b_": dict(embed_dim=64, num_heads=1, num_obj=2, num_lyt=4, oe_depth=1, pe_depth=1)}
OUTPUTS = ("x", "x_obj", "x_bg", "cls", "obj_pose", "bg_pose", "occ_score", "pts_rest_obj", "pts_rest_bg", "obj_alpha",
           "occ")
QKV_GAIN, EMBED_GAIN = 12.0, 25.0
LOGIT_STD = (1.5, 6.0)


def load_lvd(ref=REF):
    """The reference's LVD class (and its transform module), with the stand-ins of the module docstring in place while
    its files execute."""
    sys.dont_write_bytecode = True
    names = ("torchvision", "torchvision.transforms", "tools", "tools.utils", "models", "models.modules", "models.nets")
    saved = {k: sys.modules.get(k) for k in names}
    loaded = []

    def run_file(modname, *rel):
        spec = importlib.util.spec_from_file_location(modname, os.path.join(ref, *rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[modname] = mod
        loaded.append(modname)
        spec.loader.exec_module(mod)
        return mod

    try:
        tv = types.ModuleType("torchvision")
        tv.transforms = types.ModuleType("torchvision.transforms")
        tools, models = types.ModuleType("tools"), types.ModuleType("models")
        modules, nets = types.ModuleType("models.modules"), types.ModuleType("models.nets")
        tools.__path__ = [os.path.join(ref, "tools")]
        models.__path__ = [os.path.join(ref, "models")]
        modules.__path__ = [os.path.join(ref, "models", "modules")]
        nets.__path__ = [os.path.join(ref, "models", "nets")]
        sys.modules.update({"torchvision": tv, "torchvision.transforms": tv.transforms, "tools": tools, "models": models,
                            "models.modules": modules, "models.nets": nets})
        tools.utils = run_file("tools.utils", "tools", "utils.py")
        parts = {name: run_file(f"models.modules.{name}", "models", "modules", name + ".py")
                 for name in ("spectral", "weight_init", "transform", "warp", "conv")}
        for name, src in (("TPSWarp", "warp"), ("InverseWarp", "warp"), ("CustomNorm", "transform"),
                          ("MultiBlocks", "transform"), ("Block", "transform"), ("trunc_normal_", "weight_init"),
                          ("init_weights", "weight_init"), ("ConvPatchProj", "conv"), ("UNet", "conv")):
            setattr(modules, name, getattr(parts[src], name))
        lvd = run_file("models.nets.lvd", "models", "nets", "lvd.py")
        return lvd.LVD, parts["transform"]
    finally:
        for k in loaded:
            sys.modules.pop(k, None)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def condition(net, g):
    """Move the parameters to where they matter (module docstring)."""
    with torch.no_grad():
        for k, p in net.named_parameters():
            leaf = k.rsplit(".", 2)[-2:]
            if k.endswith("_embed"):
                p.mul_(EMBED_GAIN)
            elif leaf[0] in ("q", "kv", "qkv") and leaf[1] == "weight":
                p.mul_(QKV_GAIN)
            elif leaf[0] == "norm" and leaf[1] == "weight":
                p.copy_(1 + 0.3 * torch.randn(p.shape, generator=g))
            elif leaf[0] == "norm" and leaf[1] == "bias":
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
            elif k == "pose_estimator.head.weight":      # zero-initialised
                p.copy_(0.15 * torch.randn(p.shape, generator=g))
            elif k == "decoder.to_img.proj.weight":      # zero-initialised; large, against the + 5 in front of the tanh
                p.copy_(1.5 * torch.randn(p.shape, generator=g))
            elif k == "pose_estimator.head.bias":
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            elif k == "layer_estimator.cls_head.weight":
                p.mul_(20.0)


def watch_logits(net, transform):
    """Forward pre-hooks that record, for every attention module, the standard deviation of its logits."""
    stds, handles = {}, []

    def logits_of(m, q_in, kv_ins):
        h = m.num_heads
        d = (m.qkv.out_features // 3 if hasattr(m, "qkv") else m.q.out_features) // h
        b = q_in.shape[0]
        if hasattr(m, "qkv"):
            qkv = m.qkv(q_in).reshape(b, -1, 3, h, d)
            q, ks = qkv[:, :, 0], [qkv[:, :, 1]]
        else:
            q = m.q(q_in).reshape(b, -1, h, d)
            ks = [m.kv(t).reshape(b, -1, 2, h, d)[:, :, 0] for t in kv_ins]
        k = torch.cat(ks, dim=1)
        return torch.einsum("bihd,bjhd->bhij", q, k) * m.scale

    for name, m in net.named_modules():
        if isinstance(m, transform.FullAttention):
            def hook(mod, args, kwargs, name=name):
                stds[name] = logits_of(mod, args[0], None).std().item()
        elif isinstance(m, transform.ObjAttention):
            def hook(mod, args, kwargs, name=name):
                stds[name] = logits_of(mod, args[0], [args[0], kwargs["x_ctx"]]).std().item()
        else:
            continue
        handles.append(m.register_forward_pre_hook(hook, with_kwargs=True))
    return stds, handles


def run(net, inp, ctx_len):
    with torch.no_grad():
        x = net(input=inp, mode="encode_input")
        x_obj, x_bg, cls = net(x=x[:, :ctx_len], mode="estimate_layer")
        obj_pose, bg_pose, occ_score, rest_obj, rest_bg, last_obj, last_bg = net(x=x, x_obj=x_obj, x_bg=x_bg,
                                                                                 mode="estimate_pose")
        obj_alpha = net.decoder(x_obj)
        occ = net.compute_occ(occ_score)
    out = dict(zip(OUTPUTS, (x, x_obj, x_bg, cls, obj_pose, bg_pose, occ_score, rest_obj, rest_bg, obj_alpha, occ)))
    out.update(last_obj=last_obj, last_bg=last_bg)
    return out


def record(res, prefix, opt, LVD, transform, seed, check_logits, base=None, batch=B):
    """One case into ``res``; returns (its parameters, its input, its ``x``).  ``base``: another case's -- when this
    case's parameters are the same tensors (same shapes, same seed), ``<prefix>params_of`` names that case instead of
    storing them again, and the encoder's output ``x``, which is then that case's too, is left out; likewise
    ``<prefix>input_of``."""
    torch.manual_seed(seed)
    net = LVD(opt).eval()
    g = torch.Generator().manual_seed(seed + 100)
    condition(net, g)
    params = {k: p.detach() for k, p in net.named_parameters()}
    h, w = opt.dim, int(opt.dim * opt.aspect_ratio)
    inp = torch.cat([2.0 * torch.randn(batch, T, opt.num_lyt, h, w, generator=g),
                     0.3 * torch.randn(batch, T, 2, h, w, generator=g)], dim=2)
    inp = inp.half().float()   # (stored in 16 bits, exactly)
    net64 = LVD(opt).double().eval()
    net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()}, strict=True)
    stds, handles = watch_logits(net, transform)
    out32 = run(net, inp, opt.ctx_len)
    for hd in handles:
        hd.remove()
    out64 = run(net64, inp.double(), opt.ctx_len)
    print(f"{prefix}: {sum(p.numel() for p in params.values())} parameters")
    for name, s in stds.items():
        print(f"    logit std {s:6.3f}  {name}")
        assert not check_logits or LOGIT_STD[0] <= s <= LOGIT_STD[1], (name, s)
    res[prefix + "opt"] = np.array(json.dumps(vars(opt), sort_keys=True))
    res[prefix + "keys"] = np.array(list(params))
    shared = (base is not None and list(base[1]) == list(params)
              and all(torch.equal(base[1][k], v) for k, v in params.items()))
    if base is not None and torch.equal(base[2], inp):
        res[prefix + "input_of"] = np.array(base[0])
    else:
        res[prefix + "input"] = inp.half().numpy()
    if shared:
        res[prefix + "params_of"] = np.array(base[0])
    else:
        for k, p in params.items():
            res[f"{prefix}p.{k}"] = p.numpy()
    for name in OUTPUTS + ("last_obj", "last_bg"):
        a, e = out32[name], out64[name]
        if shared and name == "x" and prefix + "input_of" in res:
            assert torch.equal(a, base[3])
            continue
        if a is None:
            assert e is None
            continue
        res[f"{prefix}{name}32"], res[f"{prefix}{name}64"] = a.numpy(), e.numpy()
        print(f"    {name:13s} {tuple(a.shape)!s:18s} |v| {a.abs().max():8.3g}  std {a.std():8.3g}  "
              f"|v32 - v64| {(a.double() - e).abs().max():.2e}")
    return params, inp, out32["x"]


# the option switches of lvd.py:346-460, 920-950, one at a time on a narrow base (16 wide, one head, one block each):
# what the two full cases leave at one setting.  (``rd_translate_bias`` draws from numpy's global generator, ``has_bg``
# off and ``pe_pts_mode "head"`` do not run in the reference: not recorded.)
VARIANT_BASE = dict(COMMON, bound_rest=False, soft_bound_rest=False, circle_translate_bias=False, pad_obj_alpha=0,
                    pe_estimator_init_mode="", embed_dim=16, num_heads=1, num_obj=2, num_lyt=3, oe_depth=1, pe_depth=1)
VARIANTS = {
    "base": {}, "occ_bias": dict(occ_mode="bias"), "occ_normalize": dict(occ_mode="normalize"),
    "occ_freeze": dict(occ_mode="freeze"), "fix_bg": dict(fix_bg=True), "fix_bg1": dict(fix_bg1=True),
    "hard_bound": dict(bound_rest=True), "soft_bound": dict(bound_rest=True, soft_bound_rest=True),
    "norm_scale": dict(norm_scale=True, tgt_scale=0.7), "bound_scale": dict(bound_scale=True, min_scale=0.2, max_scale=1.5),
    "decompose_embed": dict(decompose_embed_oe=True), "no_cls": dict(pred_cls=False), "no_delta": dict(use_delta=False),
    "use_last": dict(use_last_pose_decoder=True), "decoder_prior": dict(pe_decoder_use_prior=True),
    "circle_bias": dict(circle_translate_bias=True, circle_translate_radius=0.3, init_scale_obj=0.5, mul_scale_obj=0.5,
                        mul_delta_obj=0.2, bg_mul=1.2),
    "pixel_norm": dict(norm_layer="pn"), "ln_not_affine": dict(norm_layer="ln_not_affine"),
    "decoder_zero": dict(pe_decoder_init_mode="zero", pad_obj_alpha=1, pad_bg_alpha=1),
    # the patch projections' stacks: the two full cases and every variant above have patch_size 4 -- no
    # conv -> norm -> GELU step in the encoder, one in the decoder.  The default (8) and the recipe's (16) on larger
    # rasters with the same 2 x 4 tokens, and the high-resolution stacks
    "patch8": dict(dim=16, patch_size=8), "patch16": dict(dim=32, patch_size=16),
    "use_hr": dict(dim=16, use_hr=True, hr_ratio=2),
}


def save(path, res):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


def main():
    from waldo_amd.nets.lvd import lvd_net_opt   # (the defaults of every option field, as tools/options.py has them)
    LVD, transform = load_lvd()
    res = {}
    for i, (prefix, over) in enumerate(CASES.items()):
        record(res, prefix, lvd_net_opt(**COMMON, **over), LVD, transform, SEED + i, check_logits=True)
    save(OUT, res)
    res, base = {}, None
    for name, over in VARIANTS.items():
        got = record(res, name + ".", lvd_net_opt(**dict(VARIANT_BASE, **over)), LVD, transform, SEED + 50,
                     check_logits=False, base=base, batch=1)
        base = base or (name + ".", *got)
    res["names"] = np.array(list(VARIANTS))
    save(OUT_VARIANTS, res)


if __name__ == "__main__":
    main()
