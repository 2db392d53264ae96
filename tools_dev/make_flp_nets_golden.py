"""Writes tests/golden/flp_nets_reference.npz: what the reference's own future layer predictor (models/nets/flp.py: FLP =
LatentCompressor + PoseEncoder + PoseDecoder over the blocks of models/modules/transform.py) computes on small seeded
inputs -- the fixture of tests/test_flp_nets_cpu.py and tests/test_gpu_flp_nets.py.  Data only.

    python tools_dev/make_flp_nets_golden.py [REFERENCE_ROOT]

Needs the reference tree (default /root/reference, or $WALDO_REFERENCE_ROOT); no test runs it.  The reference's files are
executed from where they lie, under the stub parents of tools_dev/make_lvd_nets_golden.py.

Per case (``names`` lists the prefixes): ``opt`` = the option values as JSON; ``keys`` = the parameter names in order and
``state_keys`` = the state dict's (parameters and buffers); ``p.<key>`` the parameters, values that 16 bits hold exactly,
stored so (buffers are not stored: a drop-in builds its own) -- or ``params_of``, the case whose parameters these are;
the seeded inputs ``obj_pose`` (B, T, No, Lo, 2), ``bg_pose`` (B, T, 1, L, 2), ``occ_score`` (B, T, No), ``x_obj``
(B, No, Nt, C), ``x_bg`` (B, Nt, C), ``last_obj``, ``last_bg``, in 16 bits too, and ``ctx_mask`` (B, T) bool; and the three
outputs ``<name>32`` / ``<name>64``: the fp32 network's and those of the same network in fp64 on the same values.  The
fp64 run is made under ``torch.set_default_dtype(torch.float64)``: the reference's ``from_ctx`` allocates its dense
tensor without a dtype, and would round an fp64 run through fp32.

The cases: ``a_`` (embed_dim 32, 2 heads: D = 16) and ``b_`` (embed_dim 64, 1 head: D = 64) with a DIFFERENT number of
context frames per clip, not all of them leading ones; ``all_`` = a_ under an all-true mask; ``nocatz_``, ``last_`` and
``free_`` = a_'s parameters with ``cat_z=False``, ``use_last_pose_decoder`` and ``unconstrained_pose_decoder``.  The noise
options draw from the framework's generator, whose stream a drop-in does not share: for ``pg_embed_noise``,
``pg_inject_noise`` and ``pg_modulate_noise`` only ``noise.<name>.keys`` / ``.state_keys`` / ``.opt`` are recorded.

Conditioning as in the LVD script (gains 12 on q / kv / qkv, 25 on the embeddings, norm affines and the zero-initialised
heads moved off 1 / 0); the script asserts that the LIVE logits of every attention -- the query / key pairs the masks
leave -- have a standard deviation in that script's LOGIT_STD range."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_lvd_nets_golden import EMBED_GAIN, LOGIT_STD, QKV_GAIN, ROOT, save  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "flp_nets_reference.npz")
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("WALDO_REFERENCE_ROOT", "/root/reference")
SEED = 20261020
NT = 3   # tokens per layer handed to the compressor
COMMON = dict(latent_shape=[2, 4], obj_shape=[2, 2], aspect_ratio=2, init_scale_obj=0.5, mul_scale_obj=0.5,
              mul_delta_obj=0.2, bg_mul_pose_decoder=1.2, zero_init_dec=True, pg_num_timesteps=5)
A = dict(COMMON, embed_dim=32, num_heads=2, num_obj=3, pg_com_depth=1, pg_enc_depth=2, pg_dec_depth=1)
B_ = dict(COMMON, embed_dim=64, num_heads=1, num_obj=2, pg_com_depth=1, pg_enc_depth=1, pg_dec_depth=1)
MASK_A = [[1, 1, 0, 1, 0], [1, 0, 0, 0, 0], [0, 1, 1, 1, 1]]
MASK_B = [[1, 1, 0, 0], [1, 0, 1, 1]]
CASES = {"a_": (A, MASK_A, None), "b_": (B_, MASK_B, None), "all_": (A, [[1] * 5] * 3, "a_"),
         "nocatz_": (dict(A, cat_z=False), MASK_A, "a_"), "last_": (dict(A, use_last_pose_decoder=True), MASK_A, "a_"),
         "free_": (dict(A, unconstrained_pose_decoder=True), MASK_A, "a_")}
NOISE = {"embed": dict(pg_embed_noise=True), "inject": dict(pg_inject_noise=True), "modulate": dict(pg_modulate_noise=True)}
OUTPUTS = ("obj_pose", "bg_pose", "occ_score")
INPUTS = ("obj_pose", "bg_pose", "occ_score", "x_obj", "x_bg", "last_obj", "last_bg")


def load_flp(ref=REF):
    """The reference's FLP class and its transform module, with stand-ins for their package parents in place while the
    files execute."""
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
        for mod, path in ((tools, ("tools",)), (models, ("models",)), (modules, ("models", "modules")),
                          (nets, ("models", "nets"))):
            mod.__path__ = [os.path.join(ref, *path)]
        sys.modules.update({"torchvision": tv, "torchvision.transforms": tv.transforms, "tools": tools, "models": models,
                            "models.modules": modules, "models.nets": nets})
        tools.utils = run_file("tools.utils", "tools", "utils.py")
        parts = {name: run_file(f"models.modules.{name}", "models", "modules", name + ".py")
                 for name in ("spectral", "weight_init", "transform")}
        for name, src in (("CustomNorm", "transform"), ("MultiBlocks", "transform"), ("Block", "transform"),
                          ("trunc_normal_", "weight_init"), ("init_weights", "weight_init")):
            setattr(modules, name, getattr(parts[src], name))
        flp = run_file("models.nets.flp", "models", "nets", "flp.py")
        return flp.FLP, parts["transform"]
    finally:
        for k in loaded:
            sys.modules.pop(k, None)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def condition(net, g):
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
            elif leaf[0] in ("obj_head", "bg_head"):      # zero-initialised
                p.copy_((0.15 if leaf[1] == "weight" else 0.3) * torch.randn(p.shape, generator=g))
            p.copy_(p.half().float())   # (stored in 16 bits, exactly)


def watch_logits(net, transform):
    """Forward pre-hooks that record, for every attention module, the standard deviation of its LIVE logits: the pairs
    of a query and a key of the same clip, among the frames the masks select on either side."""
    stds, handles = {}, []

    def clips(mask):   # the clip of every packed frame, repeated for its tokens later
        return torch.nonzero(mask)[:, 0]

    def live(m, q_in, k_ins, q_clip, k_clip):
        h = m.num_heads
        d = (m.qkv.out_features // 3 if hasattr(m, "qkv") else m.q.out_features) // h
        if hasattr(m, "qkv"):
            qkv = m.qkv(q_in).reshape(-1, 3, h, d)
            q, k = qkv[:, 0], qkv[:, 1]
        else:
            q = m.q(q_in).reshape(-1, h, d)
            k = torch.cat([m.kv(t).reshape(t.shape[0], -1, 2, h, d)[:, :, 0] for t in k_ins], dim=1).reshape(-1, h, d)
        s = torch.einsum("ihd,jhd->hij", q, k) * m.scale
        same = q_clip[:, None] == k_clip[None, :]
        return s[:, same].std().item()

    def rows(ids, n):
        return ids.repeat_interleave(n)

    for name, m in net.named_modules():
        if isinstance(m, transform.FullAttention):
            def hook(mod, args, kwargs, name=name):
                x, c = args[0], clips(kwargs["ctx_mask"])
                stds[name] = live(mod, x, None, rows(c, x.shape[1]), rows(c, x.shape[1]))
        elif isinstance(m, transform.CrossAttention):
            def hook(mod, args, kwargs, name=name):
                x, x_ctx, mask = args[0], kwargs["x_ctx"], kwargs["ctx_mask"]
                stds[name] = live(mod, x, [x_ctx], rows(clips(~mask), x.shape[1]), rows(clips(mask), x_ctx.shape[1]))
        elif isinstance(m, transform.ClsAttention):
            def hook(mod, args, kwargs, name=name):
                z, x_ctx = args[0], kwargs["x_ctx"]
                seq = torch.arange(z.shape[0])
                stds[name] = live(mod, z, [z, x_ctx], seq, rows(seq, 1 + x_ctx.shape[1]))
        else:
            continue
        handles.append(m.register_forward_pre_hook(hook, with_kwargs=True))
    return stds, handles


def inputs_of(opt, mask, g):
    b, t = mask.shape
    no, lo, l, c = opt.num_obj, opt.obj_shape[0] * opt.obj_shape[1], opt.latent_shape[0] * opt.latent_shape[1], opt.embed_dim
    shapes = dict(obj_pose=(b, t, no, lo, 2), bg_pose=(b, t, 1, l, 2), occ_score=(b, t, no), x_obj=(b, no, NT, c),
                  x_bg=(b, NT, c), last_obj=(b, no, 6 + 2 * lo), last_bg=(b, 1, 6 + 2 * l))
    gains = dict(obj_pose=0.6, bg_pose=0.6, occ_score=1.0, x_obj=1.0, x_bg=1.0, last_obj=0.3, last_bg=0.3)
    return {k: (gains[k] * torch.randn(s, generator=g)).half().float() for k, s in shapes.items()}


def run(net, inp, mask, dtype):
    with torch.no_grad():
        out = net(*[inp[k].to(dtype) for k in INPUTS], ctx_mask=mask)
    return dict(zip(OUTPUTS, out))


def record(res, prefix, opt, mask, FLP, transform, seed, base):
    torch.manual_seed(seed)
    net = FLP(opt).eval()
    g = torch.Generator().manual_seed(seed + 100)
    condition(net, g)
    params = {k: p.detach() for k, p in net.named_parameters()}
    mask = torch.tensor(mask, dtype=torch.bool)
    inp = inputs_of(opt, mask, g)
    stds, handles = watch_logits(net, transform)
    out32 = run(net, inp, mask, torch.float32)
    for hd in handles:
        hd.remove()
    torch.set_default_dtype(torch.float64)
    try:
        net64 = FLP(opt).eval()
        net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()}, strict=True)
        assert all(p.dtype == torch.float64 for p in net64.parameters())
        out64 = run(net64, inp, mask, torch.float64)
    finally:
        torch.set_default_dtype(torch.float32)
    print(f"{prefix}: {sum(p.numel() for p in params.values())} parameters, mask {mask.int().tolist()}")
    for name, s in stds.items():
        print(f"    live logit std {s:6.3f}  {name}")
        assert s != s or LOGIT_STD[0] <= s <= LOGIT_STD[1], (name, s)   # (NaN: an attention without a live pair)
    res[prefix + "opt"] = np.array(json.dumps(vars(opt), sort_keys=True))
    res[prefix + "keys"] = np.array(list(params))
    res[prefix + "state_keys"] = np.array(list(net.state_dict()))
    res[prefix + "ctx_mask"] = mask.numpy()
    for k, v in inp.items():
        res[f"{prefix}in.{k}"] = v.half().numpy()
    if base is not None:
        assert list(base[1]) == list(params) and all(torch.equal(base[1][k], v) for k, v in params.items())
        res[prefix + "params_of"] = np.array(base[0])
    else:
        for k, p in params.items():
            assert torch.equal(p.half().float(), p)
            res[f"{prefix}p.{k}"] = p.half().numpy()
    for name in OUTPUTS:
        a, e = out32[name], out64[name]
        assert e.dtype == torch.float64
        res[f"{prefix}{name}32"], res[f"{prefix}{name}64"] = a.numpy(), e.numpy()
        moved = (a - inp[name]).abs().max().item()
        print(f"    {name:10s} {tuple(a.shape)!s:18s} |v| {a.abs().max():8.3g}  moved {moved:8.3g}  "
              f"|v32 - v64| {(a.double() - e).abs().max():.2e}")
    return params


def main():
    from waldo_amd.nets.flp import flp_net_opt   # (the defaults of every option field, as tools/options.py has them)
    FLP, transform = load_flp()
    res, recorded = {}, {}
    for prefix, (over, mask, params_of) in CASES.items():
        base = None if params_of is None else (params_of, recorded[params_of])
        # (a case that shares a_'s parameters is built from a_'s seed)
        seed = SEED + list(CASES).index(params_of or prefix)
        recorded[prefix] = record(res, prefix, flp_net_opt(**over), mask, FLP, transform, seed, base)
    for name, over in NOISE.items():
        opt = flp_net_opt(**dict(A, **over))
        net = FLP(opt)
        res[f"noise.{name}.opt"] = np.array(json.dumps(vars(opt), sort_keys=True))
        res[f"noise.{name}.keys"] = np.array([k for k, _ in net.named_parameters()])
        res[f"noise.{name}.state_keys"] = np.array(list(net.state_dict()))
    res["names"] = np.array(list(CASES))
    save(OUT, res)
    assert os.path.getsize(OUT) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "lvd_nets_reference.npz"))


if __name__ == "__main__":
    main()
