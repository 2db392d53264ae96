"""dev: is a rebuilt frame warp (csrc/flow_ctx_kernels.hip.h: frame_warp_fuse_kernel, frame_warp_fuse_lds_kernel) the
parent's, bit for bit and in time?

    python tools_dev/fwf_refactor_check.py dump --lib PARENT.so --out DIR_A     # one process per library
    python tools_dev/fwf_refactor_check.py dump --out DIR_B                     # the product library
    python tools_dev/fwf_refactor_check.py compare DIR_A DIR_B --out bits.json
    python tools_dev/fwf_refactor_check.py speed --runs RUNS.json --out speed.json

dump    writes `out` and `raw` of a fixed, seeded case list as raw bytes in one file with an index: the shape grid of
        tests/test_gpu_warper.py::test_frame_warp_fuse_staged_boxes_same_bits plus Tc = 6 at 24 x 48 (the gather kernel's
        <8> instance), every case with 16-byte aligned frames (the LDS kernel) and with the same frames one float into a
        buffer (the gather kernel), through WF.frame_warp_fuse (the alpha path), WF.frame_warp_fuse_raw with `raw` in
        fp32 / bf16 / fp16 on the fp32 clip, and with `raw` in fp32 / bf16 on a PackedClip (aligned only).
compare counts the differing bytes of two dumps (required: 0).
speed   RUNS.json: {setting: {"parent": [[ms of a run's rounds], ...], "new": [[...], ...]}} -- one run per library for
        ab_hd.py (its rounds interleave the libraries), two for the pipeline tools (ab_raw_dtype.py, ab_packed_clip.py:
        ms_rounds, taken in the order parent, new, parent, new).  Per setting the new median against the parent's median
        x (1 + margin), margin = the larger of the spread of the parent's own rounds and of the relative difference
        between the parent's two runs.  With one run per library (the ab_hd.py settings) there is no second run to
        differ from: the margin is then the spread of the parent's rounds alone."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refactor_check  # noqa: E402  (dump writer, compare, the no-slower rule, the command line; puts the repository on the path)

GRID = [(tc, inc, hw, amp) for tc, inc in ((4, False), (2, False), (3, True), (4, True), (1, False), (1, True))
        for hw in ((64, 128), (37, 100), (8, 36), (128, 256)) for amp in (3.0, 40.0)]
GRID += [(6, False, (24, 48), amp) for amp in (3.0, 40.0)]


def dump(d):
    import torch
    from waldo_amd import functional as WF
    dev = torch.device("cuda:0")
    b, t, c, nl = 2, 5, 6, 3
    put = d.put
    with torch.no_grad():
        for tc, inc, (hd, wd), amp in GRID:
            tp = t if inc else 3
            tcx = tc + (1 if inc else 0)
            g = torch.Generator(device=dev).manual_seed(hd + tc)
            buf = torch.randn(b * t * c * hd * wd + 1, generator=g, device=dev)
            off = buf[1:].view(b, t, c, hd, wd)
            fl = (amp * 2 / wd) * torch.randn(b * tc * tp, 2, max(hd // 16, 1), max(wd // 16, 1), generator=g, device=dev)
            flow = torch.nn.functional.interpolate(fl, size=(hd, wd), mode="bilinear").view(b, tc, tp, 2, hd, wd).contiguous()
            flow[0, 0, 0, :, : hd // 2] += 2.5                          # a block of samples outside the frame
            alpha = torch.rand(b, tc, tp, nl, hd, wd, generator=g, device=dev) * 2 - 1
            ctx_ts = torch.randint(0, t, (b, tc, tp), generator=g, device=dev)
            raw0 = torch.rand(b, tp, tcx, c + nl, hd, wd, generator=g, device=dev) * 2 - 1
            score = torch.rand(b, tc, tp, hd, wd, generator=g, device=dev) * nl + 0.05
            rgb = torch.randint(0, 256, (b, t, 3, hd, wd), generator=g, device=dev, dtype=torch.uint8)
            cls = torch.randint(0, c - 3 + 1, (b, t, hd, wd), generator=g, device=dev)  # (one id past the classes, too)
            packed = WF.pack_clip(rgb, cls, c - 3)
            for where, frames in (("aligned", off.clone()), ("misaligned", off)):
                assert frames.data_ptr() % 16 == (0 if where == "aligned" else 4)
                name = f"tc={tc} self={inc} {hd}x{wd} amp={amp} {where}"
                out, raw = WF.frame_warp_fuse(frames, flow, alpha, ctx_ts, include_self=inc)
                put(name, "alpha out", out), put(name, "alpha raw", raw)
                for clip, dtypes in ((frames, (torch.float32, torch.bfloat16, torch.float16)),
                                     (packed if where == "aligned" else None, (torch.float32, torch.bfloat16))):
                    for dt in dtypes if clip is not None else ():
                        slots = WF.RawSlots(raw0.to(dt), score, c, inc)
                        out, _ = WF.frame_warp_fuse_raw(clip, flow, slots, ctx_ts)
                        kind = f"{'packed' if clip is packed else 'fp32'} clip, {str(dt)[6:]} raw"
                        put(name, kind + ": out", out), put(name, kind + ": raw", slots.raw)
    return 2 * len(GRID)


if __name__ == "__main__":
    refactor_check.main(__doc__, dump)
