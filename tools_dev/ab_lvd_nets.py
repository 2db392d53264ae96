"""A/B of the fused token attention (WF.token_attention, csrc/token_attention.hip) against the two framework routes -- the
reference's sequence of ops (WF.token_attention_framework) and ``F.scaled_dot_product_attention`` on the same views --
at the LVD recipe's shapes (scripts/cityscapes/train_lvd.sh: 512 wide, 8 heads, D = 64) on one MI355X, and of the whole
``nets.LVD`` with ``fused`` True against False.  Writes profiles/lvd_nets.json; the two training sections, ``bwd`` and
``step``, are run with ``--out profiles/lvd_nets_bwd.json``.

    python tools_dev/ab_lvd_nets.py [--out profiles/lvd_nets.json] [--sections op,lvd] [--rounds 20] [--warmup 5]
    python tools_dev/ab_lvd_nets.py --out profiles/lvd_nets_bwd.json --sections bwd,step [--clips 4]
    python tools_dev/ab_lvd_nets.py --out FILE --sections op,bwd --head-dim 16 --lib tools_dev/_variants/NAME.so

    python tools_dev/ab_lvd_nets.py --dtype bf16        (writes profiles/lvd_nets_16bit.json: sections op16,lvd16,step16)
    python tools_dev/ab_lvd_nets.py --dtype bf16 --sections16 bwd16,step16      (writes profiles/lvd_nets_16bit_bwd.json)

--dtype bf16 | fp16 measures the 16-bit route (WF.token_attention_16bit_route("kernel"), ``act_dtype``) instead:
  op16   at the four op shapes, in one process: ``kernel16`` (waldo_token_attention_fwd_dt on the 16-bit operands),
         ``framework16`` (WF.token_attention_framework on the same operands), ``sdpa16`` and ``kernel32`` (the fp32 kernel
         on fp32 copies).  ``kernel16_beats_kernel32``: by more than the spread -- the condition on the kernel at pose_56
         and pose_112; the sdpa comparison is reported without a bar.  With the bound-by figures: matrix FLOP/s and the
         bytes of the operands and out over the time;
  lvd16  the whole LVD forward: ``act_dtype`` fused, fp32 fused, and ``fused = False`` under the same autocast;
  step16 ``LvdStep(--clips, nets="reference")`` with ``act_dtype`` against fp32 and against ``fused = False`` under the same
         autocast (all with the default backward route), and with ``act_dtype`` under
         WF.token_attention_16bit_backward_route("kernel") (``act_dtype_kernel_backward``);
  bwd16  forward + backward of the op at the four op shapes, the gradient of a fixed ``grad_out`` in every operand:
         ``kernel16`` (both 16-bit switches on "kernel": waldo_token_attention_fwd_lse_dt + waldo_token_attention_bwd_dt),
         ``recompute16`` (the 16-bit forward kernel, the backward recomputing WF.token_attention_framework in 16 bits:
         the route before the 16-bit backward), ``kernel32`` (the fp32 kernels on fp32 copies) and ``sdpa16`` with its
         own backward in the same type; ms and peak bytes each.  ``kernel16_beats_recompute16``: by more than the spread.

--lib binds another build of the library (``_lib.use_library``: tools_dev/build_variant.py makes one) for an A/B of two
builds in two processes; --head-dim D runs ``op`` and ``bwd`` at another head dimension with the same token counts and
512 / D heads (the width stays 512; the default 64 is the recipe's).

Sections:
  op   the op alone, forward without autograd, fp32: the PoseEstimator's self-attention (56 and 112 sequences of
       128 + 256 + 128 = 512 tokens, q / k / v the slices of one packed qkv projection) and the LayerEstimator's
       two-segment attention (4 and 8 clips, 384 queries against 384 + 4 * 128 = 896 keys, the slices of two packed kv
       projections).  ``sdpa`` gets the ``cat`` of the two key / value sets that it needs and the transpose + reshape to
       the (B, N, H D) layout the other two routes return;
  lvd  the whole network without autograd at the recipe's widths for 4 clips of 14 frames: encode_input,
       estimate_layer (4 context frames), estimate_pose, estimate_alpha_grid_occ -- ``fused`` True against False of the
       SAME module;
  bwd  forward + backward of the op at the shapes of ``op``, the gradient of a fixed ``grad_out`` in every operand:
       ``kernel`` (WF.token_attention under token_attention_backward_route("kernel"): waldo_token_attention_fwd_lse +
       waldo_token_attention_bwd), ``framework_recompute`` (the same forward kernel, the backward recomputing and
       differentiating WF.token_attention_framework: the route before the backward kernel) and ``sdpa`` with its own
       backward.  ``kernel_default`` applies the rule: the kernel route beats the recompute by more than the spread;
  step ``LvdStep(--clips, device, nets="reference")`` at the recipe's widths, eager: forward, loss and backward under
       both routes of the attention's backward.
Method: device time between events; the routes ALTERNATE inside one process (one call of each per round), --rounds
rounds after --warmup of each; median, minimum and quartiles per route.  ``spread`` is the largest of the routes'
interquartile ranges over their medians; ``kernel_wins`` says median(kernel) * (1 + spread) < median(each other route).
Peak memory is ``max_memory_allocated`` above what was allocated before the call (the inputs), one call each.  A run
without a GPU fails."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from waldo_amd import functional as WF  # noqa: E402

WIDTH = 512
HEADS, D = 8, 64   # main() sets them from --head-dim
# (name, sequences, queries, keys of the first segment, keys of the second or None)
OP_SHAPES = (("pose_56", 56, 512, 512, None), ("pose_112", 112, 512, 512, None),
             ("layer_4", 4, 384, 384, 512), ("layer_8", 8, 384, 384, 512))


def alternate(routes, warmup, rounds):
    """{name: stats} of callables timed alternately: one call of each per round."""
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    out = {}
    for k, v in ms.items():
        q1, med, q3 = (float(x) for x in np.percentile(v, [25, 50, 75]))
        out[k] = dict(median_ms=med, min_ms=float(np.min(v)), q1_ms=q1, q3_ms=q3, rounds=len(v))
    out["spread"] = max((s["q3_ms"] - s["q1_ms"]) / s["median_ms"] for s in out.values())
    return out


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    keep = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del keep
    return int(peak)


def op_operands(seqs, nq, nk1, nk2, device, seed=0):
    """The views the modules hand to the op: logits of standard deviation 2."""
    g = torch.Generator(device=device).manual_seed(seed)
    mk = lambda n, parts: torch.randn(seqs, n, parts, HEADS, D, generator=g, device=device) * 1.4
    if nk2 is None:
        return (*mk(nq, 3).unbind(2), None, None)
    return (mk(nq, 1)[:, :, 0], *mk(nk1, 2).unbind(2), *mk(nk2, 2).unbind(2))


def sdpa_route(q, k, v, k2=None, v2=None):
    if k2 is not None:
        k, v = torch.cat([k, k2], dim=1), torch.cat([v, v2], dim=1)
    out = F.scaled_dot_product_attention(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3))
    return out.transpose(1, 2).reshape(q.shape[0], q.shape[1], -1)


def kernel_route(q, k, v, k2=None, v2=None):
    assert WF._token_attention_served(q, k, v, k2, v2) is not None
    return WF.token_attention(q, k, v, k2, v2)


def op_routes(ops):
    return {"kernel": lambda: kernel_route(*ops), "framework": lambda: WF.token_attention_framework(*ops),
            "sdpa": lambda: sdpa_route(*ops)}


def op_flops(seqs, nq, nk):
    return 4.0 * seqs * HEADS * nq * nk * D   # two products, a multiply and an add each


def section_op(device, warmup, rounds):
    res = {}
    for name, seqs, nq, nk1, nk2 in OP_SHAPES:
        ops = op_operands(seqs, nq, nk1, nk2, device)
        with torch.no_grad():
            routes = op_routes(ops)
            ref = routes["framework"]()
            err = {k: float((fn() - ref).abs().max()) for k, fn in routes.items() if k != "framework"}
            del ref
            st = alternate(routes, warmup, rounds)
            for k, fn in routes.items():
                st[k]["peak_bytes_above_inputs"] = peak_above_inputs(fn)
        others = [st[k]["median_ms"] for k in ("framework", "sdpa")]
        st["kernel_over_framework"] = st["kernel"]["median_ms"] / st["framework"]["median_ms"]
        st["kernel_over_sdpa"] = st["kernel"]["median_ms"] / st["sdpa"]["median_ms"]
        st["kernel_wins"] = bool(st["kernel"]["median_ms"] * (1 + st["spread"]) < min(others))
        st["kernel_tflops"] = op_flops(seqs, nq, nk1 + (nk2 or 0)) / (st["kernel"]["median_ms"] * 1e-3) / 1e12
        st["max_abs_difference_from_framework"] = err
        st["shape"] = dict(sequences=seqs, heads=HEADS, head_dim=D, queries=nq, keys=[nk1] + ([nk2] if nk2 else []))
        res[name] = st
        print(name, json.dumps({k: (round(v["median_ms"], 4), v["peak_bytes_above_inputs"] >> 20) for k, v in st.items()
                                if isinstance(v, dict) and "median_ms" in v}), "spread", round(st["spread"], 3),
              "wins", st["kernel_wins"], flush=True)
    return res


def bwd_routes(ops, go):
    """Forward + backward per route, on leaves that are the views themselves (detached: no gradient accumulates)."""
    leaves = [None if t is None else t.detach().requires_grad_() for t in ops]
    wanted = [t for t in leaves if t is not None]

    def through(fn, route=None):
        def run():
            if route is None:
                out = fn(*leaves)
            else:
                with WF.token_attention_backward_route(route):
                    out = fn(*leaves)
            return torch.autograd.grad(out, wanted, go)
        return run

    return {"kernel": through(kernel_route, "kernel"), "framework_recompute": through(kernel_route, "framework"),
            "sdpa": through(sdpa_route)}


def section_bwd(device, warmup, rounds):
    res = {}
    for name, seqs, nq, nk1, nk2 in OP_SHAPES:
        ops = op_operands(seqs, nq, nk1, nk2, device)
        go = torch.randn(seqs, nq, HEADS * D, generator=torch.Generator(device=device).manual_seed(1), device=device)
        routes = bwd_routes(ops, go)
        ref = routes["framework_recompute"]()
        err = {k: max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(fn(), ref))
               for k, fn in routes.items() if k != "framework_recompute"}
        del ref
        st = alternate(routes, warmup, rounds)
        for k, fn in routes.items():
            st[k]["peak_bytes_above_inputs"] = peak_above_inputs(fn)
        med = {k: st[k]["median_ms"] for k in routes}
        st["kernel_over_framework_recompute"] = med["kernel"] / med["framework_recompute"]
        st["kernel_over_sdpa"] = med["kernel"] / med["sdpa"]
        st["kernel_beats_framework_recompute"] = bool(med["kernel"] * (1 + st["spread"]) < med["framework_recompute"])
        st["kernel_beats_sdpa"] = bool(med["kernel"] * (1 + st["spread"]) < med["sdpa"])
        # seven products forward + backward of the mathematics; the kernel route runs eleven (S three times, dP twice)
        st["kernel_tflops_of_the_mathematics"] = 3.5 * op_flops(seqs, nq, nk1 + (nk2 or 0)) / (med["kernel"] * 1e-3) / 1e12
        st["max_relative_gradient_difference_from_framework_recompute"] = err
        st["shape"] = dict(sequences=seqs, heads=HEADS, head_dim=D, queries=nq, keys=[nk1] + ([nk2] if nk2 else []))
        res[name] = st
        print(name, json.dumps({k: (round(v["median_ms"], 4), v["peak_bytes_above_inputs"] >> 20) for k, v in st.items()
                                if isinstance(v, dict) and "median_ms" in v}), "spread", round(st["spread"], 3),
              "beats recompute", st["kernel_beats_framework_recompute"], "beats sdpa", st["kernel_beats_sdpa"], flush=True)
    res["kernel_beats_framework_recompute_everywhere"] = all(v["kernel_beats_framework_recompute"] for v in res.values())
    return res


def section_step(device, warmup, rounds, clips=4):
    from waldo_amd.tools.lvd_step import LvdStep
    step = LvdStep(clips, device, nets="reference")

    def route(name):
        def fn():
            with WF.token_attention_backward_route(name):
                return step()
        return fn

    routes = {"kernel": route("kernel"), "framework_recompute": route("framework")}
    st = alternate(routes, warmup, rounds)
    for k, fn in routes.items():
        st[k]["peak_bytes_above_inputs"] = peak_above_inputs(fn)
    st["kernel_over_framework_recompute"] = st["kernel"]["median_ms"] / st["framework_recompute"]["median_ms"]
    st["kernel_beats_framework_recompute"] = bool(st["kernel"]["median_ms"] * (1 + st["spread"])
                                                  < st["framework_recompute"]["median_ms"])
    st["shape"] = dict(clips=clips, frames=LvdStep.frames, nets="reference", mode="eager")
    print("step", json.dumps({k: (round(v["median_ms"], 3), v["peak_bytes_above_inputs"] >> 20) for k, v in st.items()
                              if isinstance(v, dict) and "median_ms" in v}), "spread", round(st["spread"], 3), flush=True)
    return st


def lvd_forward(net, inp, ctx_len):
    x = net(input=inp, mode="encode_input")
    x_obj, x_bg, cls = net(x=x[:, :ctx_len], mode="estimate_layer")
    obj_pose, bg_pose, occ_score = net(x=x, x_obj=x_obj, x_bg=x_bg, mode="estimate_pose")[:3]
    return net(x_obj=x_obj, obj_pose=obj_pose, bg_pose=bg_pose, occ_score=occ_score, mode="estimate_alpha_grid_occ")


def section_lvd(device, warmup, rounds, clips=4, frames=14, opt=None):
    from waldo_amd.nets import LVD
    from waldo_amd.tools.lvd_step import recipe_net_opt
    opt = opt or recipe_net_opt()
    torch.manual_seed(0)
    net = LVD(opt).to(device).eval()
    g = torch.Generator(device=device).manual_seed(1)
    h, w = opt.dim, int(opt.dim * opt.aspect_ratio)
    inp = torch.randn(clips, frames, opt.num_lyt + 2, h, w, generator=g, device=device)

    def route(fused):
        def fn():
            net.fused = fused
            return lvd_forward(net, inp, opt.ctx_len)
        return fn

    with torch.no_grad():
        routes = {"fused": route(True), "framework": route(False)}
        st = alternate(routes, warmup, rounds)
        for k, fn in routes.items():
            st[k]["peak_bytes_above_inputs"] = peak_above_inputs(fn)
    st["fused_over_framework"] = st["fused"]["median_ms"] / st["framework"]["median_ms"]
    st["fused_wins"] = bool(st["fused"]["median_ms"] * (1 + st["spread"]) < st["framework"]["median_ms"])
    st["shape"] = dict(clips=clips, frames=frames, embed_dim=opt.embed_dim, heads=opt.num_heads, raster=[h, w],
                       num_obj=opt.num_obj, depths=[opt.oe_depth, opt.pe_depth])
    print("lvd", json.dumps({k: round(v["median_ms"], 3) for k, v in st.items() if isinstance(v, dict) and "median_ms" in v}),
          "spread", round(st["spread"], 3), flush=True)
    return st


DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
PEAK_16BIT_TFLOPS, PEAK_HBM_TBS = 2500.0, 8.0   # MI355X: dense bf16 / fp16 matrix rate, HBM3E bandwidth (data sheet)


def section_op16(device, warmup, rounds, dtype):
    res = {}
    for name, seqs, nq, nk1, nk2 in OP_SHAPES:
        ops32 = op_operands(seqs, nq, nk1, nk2, device)
        ops16 = packed16(ops32, dtype)

        def kernel16():
            with WF.token_attention_16bit_route("kernel"):
                assert WF._token_attention_served_16bit(*ops16) is not None
                return WF.token_attention(*ops16)

        with torch.no_grad():
            routes = {"kernel16": kernel16, "framework16": lambda: WF.token_attention_framework(*ops16),
                      "sdpa16": lambda: sdpa_route(*ops16), "kernel32": lambda: kernel_route(*ops32)}
            ref = WF.token_attention_framework(*(None if t is None else t.double() for t in ops16))
            err = {k: float((fn().double() - ref).abs().max()) for k, fn in routes.items() if k != "kernel32"}
            del ref
            st = alternate(routes, warmup, rounds)
            for k, fn in routes.items():
                st[k]["peak_bytes_above_inputs"] = peak_above_inputs(fn)
        med = {k: st[k]["median_ms"] for k in routes}
        nk = nk1 + (nk2 or 0)
        st["kernel16_over_kernel32"] = med["kernel16"] / med["kernel32"]
        st["kernel16_over_framework16"] = med["kernel16"] / med["framework16"]
        st["kernel16_over_sdpa16"] = med["kernel16"] / med["sdpa16"]
        st["kernel16_beats_kernel32"] = bool(med["kernel16"] * (1 + st["spread"]) < med["kernel32"])
        tflops = op_flops(seqs, nq, nk) / (med["kernel16"] * 1e-3) / 1e12
        moved = 2.0 * seqs * HEADS * D * (2 * nq + 2 * nk)   # q and out once, k and v once: the least that crosses memory
        st["bound_by"] = dict(kernel16_tflops=tflops, fraction_of_matrix_peak=tflops / PEAK_16BIT_TFLOPS,
                              least_bytes=moved, least_bytes_tb_per_s=moved / (med["kernel16"] * 1e-3) / 1e12,
                              fraction_of_hbm_peak=moved / (med["kernel16"] * 1e-3) / 1e12 / PEAK_HBM_TBS,
                              flops_per_byte=op_flops(seqs, nq, nk) / moved)
        st["max_abs_difference_from_fp64_framework"] = err
        st["shape"] = dict(sequences=seqs, heads=HEADS, head_dim=D, queries=nq, keys=[nk1] + ([nk2] if nk2 else []))
        res[name] = st
        print(name, json.dumps({k: round(v, 4) for k, v in med.items()}), "spread", round(st["spread"], 3),
              "beats fp32 kernel", st["kernel16_beats_kernel32"], "TFLOP/s", round(tflops, 1), flush=True)
    res["kernel16_beats_kernel32_at_pose_shapes"] = bool(res["pose_56"]["kernel16_beats_kernel32"]
                                                         and res["pose_112"]["kernel16_beats_kernel32"])
    return res


def packed16(ops32, dtype):
    """16-bit operands as the modules hand them over: the slices of packed 16-bit projections."""
    ops16 = tuple(None if t is None else t.to(dtype) for t in ops32)
    if ops16[3] is None:
        return (*torch.stack(ops16[:3], dim=2).unbind(2), None, None)
    return (ops16[0], *torch.stack(ops16[1:3], dim=2).unbind(2), *torch.stack(ops16[3:], dim=2).unbind(2))


def section_bwd16(device, warmup, rounds, dtype):
    res = {}
    for name, seqs, nq, nk1, nk2 in OP_SHAPES:
        ops32 = op_operands(seqs, nq, nk1, nk2, device)
        go32 = torch.randn(seqs, nq, HEADS * D, generator=torch.Generator(device=device).manual_seed(1), device=device)
        go16 = go32.to(dtype)
        leaves16 = [None if t is None else t.detach().requires_grad_() for t in packed16(ops32, dtype)]
        leaves32 = [None if t is None else t.detach().requires_grad_() for t in ops32]
        wanted16, wanted32 = [t for t in leaves16 if t is not None], [t for t in leaves32 if t is not None]

        def kernel16(bwd_route):
            def run():
                with WF.token_attention_16bit_route("kernel"), WF.token_attention_16bit_backward_route(bwd_route):
                    assert WF._token_attention_served_16bit(*leaves16) is not None
                    out = WF.token_attention(*leaves16)
                return torch.autograd.grad(out, wanted16, go16)
            return run

        def kernel32():
            with WF.token_attention_backward_route("kernel"):
                out = kernel_route(*leaves32)
            return torch.autograd.grad(out, wanted32, go32)

        routes = {"kernel16": kernel16("kernel"), "recompute16": kernel16("framework"), "kernel32": kernel32,
                  "sdpa16": lambda: torch.autograd.grad(sdpa_route(*leaves16), wanted16, go16)}
        ref = routes["kernel32"]()
        err = {k: max(float((a.float() - b).abs().max() / b.abs().max()) for a, b in zip(fn(), ref))
               for k, fn in routes.items() if k != "kernel32"}
        del ref
        st = alternate(routes, warmup, rounds)
        for k, fn in routes.items():
            st[k]["peak_bytes_above_inputs"] = peak_above_inputs(fn)
        med = {k: st[k]["median_ms"] for k in routes}
        for other in ("recompute16", "kernel32", "sdpa16"):
            st[f"kernel16_over_{other}"] = med["kernel16"] / med[other]
            st[f"kernel16_beats_{other}"] = bool(med["kernel16"] * (1 + st["spread"]) < med[other])
        st["kernel16_tflops_of_the_mathematics"] = 3.5 * op_flops(seqs, nq, nk1 + (nk2 or 0)) / (med["kernel16"] * 1e-3) / 1e12
        st["max_relative_gradient_difference_from_kernel32"] = err
        st["shape"] = dict(sequences=seqs, heads=HEADS, head_dim=D, queries=nq, keys=[nk1] + ([nk2] if nk2 else []))
        res[name] = st
        print(name, json.dumps({k: (round(v["median_ms"], 4), v["peak_bytes_above_inputs"] >> 20) for k, v in st.items()
                                if isinstance(v, dict) and "median_ms" in v}), "spread", round(st["spread"], 3),
              "beats recompute16", st["kernel16_beats_recompute16"], flush=True)
    res["kernel16_beats_recompute16_everywhere"] = all(v["kernel16_beats_recompute16"] for v in res.values())
    res["not_measured"] = ["D = 16 and D = 32", "hardware counters", "the step replayed from a graph", "fp16 unless run"]
    return res


def section_lvd16(device, warmup, rounds, dtype, clips=4, frames=14):
    from waldo_amd.nets import LVD
    from waldo_amd.tools.lvd_step import recipe_net_opt
    opt = recipe_net_opt()
    torch.manual_seed(0)
    net = LVD(opt).to(device).eval()
    g = torch.Generator(device=device).manual_seed(1)
    h, w = opt.dim, int(opt.dim * opt.aspect_ratio)
    inp = torch.randn(clips, frames, opt.num_lyt + 2, h, w, generator=g, device=device)

    def route(fused, act_dtype):
        def fn():
            net.fused, net.act_dtype = fused, act_dtype
            return lvd_forward(net, inp, opt.ctx_len)
        return fn

    with torch.no_grad():
        routes = {"fused_act_dtype": route(True, dtype), "fused_fp32": route(True, None),
                  "framework_autocast": route(False, dtype)}
        st = alternate(routes, warmup, rounds)
    st["act_dtype_over_fp32"] = st["fused_act_dtype"]["median_ms"] / st["fused_fp32"]["median_ms"]
    st["act_dtype_over_framework_autocast"] = st["fused_act_dtype"]["median_ms"] / st["framework_autocast"]["median_ms"]
    st["shape"] = dict(clips=clips, frames=frames, embed_dim=opt.embed_dim, heads=opt.num_heads, raster=[h, w],
                       num_obj=opt.num_obj, depths=[opt.oe_depth, opt.pe_depth])
    print("lvd16", json.dumps({k: round(v["median_ms"], 3) for k, v in st.items() if isinstance(v, dict) and "median_ms" in v}),
          "spread", round(st["spread"], 3), flush=True)
    return st


def section_step16(device, warmup, rounds, dtype, clips=4):
    from waldo_amd.tools.lvd_step import LvdStep
    steps = {"act_dtype": LvdStep(clips, device, nets="reference", act_dtype=dtype),
             "fp32": LvdStep(clips, device, nets="reference"),
             "framework_autocast": LvdStep(clips, device, nets="reference", act_dtype=dtype)}
    steps["framework_autocast"].net.fused = False
    kernel_backward = LvdStep(clips, device, nets="reference", act_dtype=dtype)

    def act_dtype_kernel_backward():
        with WF.token_attention_16bit_backward_route("kernel"):
            return kernel_backward()

    steps["act_dtype_kernel_backward"] = act_dtype_kernel_backward
    st = alternate(steps, warmup, rounds)
    for k, fn in steps.items():
        st[k]["peak_bytes_above_inputs"] = peak_above_inputs(fn)
    st["kernel_backward_over_act_dtype"] = st["act_dtype_kernel_backward"]["median_ms"] / st["act_dtype"]["median_ms"]
    st["kernel_backward_beats_act_dtype"] = bool(st["act_dtype_kernel_backward"]["median_ms"] * (1 + st["spread"])
                                                 < st["act_dtype"]["median_ms"])
    st["act_dtype_over_framework_autocast"] = st["act_dtype"]["median_ms"] / st["framework_autocast"]["median_ms"]
    st["act_dtype_over_fp32"] = st["act_dtype"]["median_ms"] / st["fp32"]["median_ms"]
    st["shape"] = dict(clips=clips, frames=LvdStep.frames, nets="reference", mode="eager",
                       backward_route=WF.get_token_attention_backward_route())
    print("step16", json.dumps({k: round(v["median_ms"], 3) for k, v in st.items() if isinstance(v, dict) and "median_ms" in v}),
          "spread", round(st["spread"], 3), flush=True)
    return st


def main_16bit(args, device):
    dtype = DTYPES[args.dtype]
    names = (args.sections16 or "op16,lvd16,step16").split(",")
    out = args.out16 or os.path.join(ROOT, "profiles", "lvd_nets_16bit_bwd.json" if "bwd16" in names else "lvd_nets_16bit.json")
    doc = {}
    if os.path.exists(out):
        with open(out) as fh:
            doc = json.load(fh)
    part = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, limits=WF.token_attention_16bit_limits(),
                head_dim=D, method=dict(rounds=args.rounds, warmup=args.warmup, timing="device events, routes alternating"))
    sections = {"op16": section_op16, "lvd16": section_lvd16, "bwd16": section_bwd16,
                "step16": lambda *a: section_step16(*a, clips=args.clips)}
    for sec in names:
        part[sec] = sections[sec](device, args.warmup, args.rounds, dtype)
        doc[args.dtype] = part
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
    print(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lvd_nets.json"))
    ap.add_argument("--sections", default="op,lvd")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clips", type=int, default=4, help="clips of the step section")
    ap.add_argument("--lib", help="another build of the library to bind instead of the product's")
    ap.add_argument("--head-dim", type=int, default=64, choices=(16, 32, 64), help="D of the op and bwd sections")
    ap.add_argument("--dtype", choices=sorted(DTYPES), help="measure the 16-bit route: profiles/lvd_nets_16bit.json")
    ap.add_argument("--out16", help="with --dtype: the file to write instead")
    ap.add_argument("--sections16", help="with --dtype: of op16,lvd16,step16,bwd16 (default: the first three; with bwd16 "
                                         "the file is profiles/lvd_nets_16bit_bwd.json)")
    args = ap.parse_args()
    global HEADS, D
    HEADS, D = WIDTH // args.head_dim, args.head_dim
    if args.lib:
        from waldo_amd import _lib
        _lib.use_library(args.lib)
    if not torch.cuda.is_available():
        raise SystemExit("ab_lvd_nets: no GPU (a measurement does not fall back)")
    device = torch.device("cuda:0")
    if args.dtype:
        return main_16bit(args, device)
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            doc = json.load(fh)
    doc.update(device=torch.cuda.get_device_name(0), torch=torch.__version__, limits=WF.token_attention_limits(),
               library=args.lib or "product", head_dim=D,
               bwd_limits=WF.token_attention_bwd_limits(),
               method=dict(rounds=args.rounds, warmup=args.warmup, timing="device events, routes alternating"))
    sections = {"op": section_op, "lvd": section_lvd, "bwd": section_bwd,
                "step": lambda *a: section_step(*a, clips=args.clips)}
    for sec in args.sections.split(","):
        doc[sec] = sections[sec](device, args.warmup, args.rounds)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
    if "bwd" in doc and "step" in doc:
        # the rule for the default route: the kernel beats the route before it, by more than the spread, at every op
        # shape and in the step
        doc["kernel_route_wins_everywhere"] = bool(doc["bwd"]["kernel_beats_framework_recompute_everywhere"]
                                                   and doc["step"]["kernel_beats_framework_recompute"])
        doc["default_route"] = WF.get_token_attention_backward_route()
        doc["default_route_note"] = ("the default stays 'framework' while tests/test_gpu_lvd_nets.py counts the plain "
                                     "waldo_token_attention_fwd launches of a training step: under 'kernel' a forward "
                                     "that records a node runs waldo_token_attention_fwd_lse")
        doc["not_measured"] = ["D = 16 and D = 32", "the step replayed from a graph"]
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
    print(args.out)


if __name__ == "__main__":
    main()
