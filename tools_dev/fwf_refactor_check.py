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
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID = [(tc, inc, hw, amp) for tc, inc in ((4, False), (2, False), (3, True), (4, True), (1, False), (1, True))
        for hw in ((64, 128), (37, 100), (8, 36), (128, 256)) for amp in (3.0, 40.0)]
GRID += [(6, False, (24, 48), amp) for amp in (3.0, 40.0)]


def dump(args):
    import torch
    from waldo_amd import _lib, functional as WF
    if args.lib:
        _lib.use_library(args.lib)
    dev = torch.device("cuda:0")
    b, t, c, nl = 2, 5, 6, 3
    os.makedirs(args.out, exist_ok=True)
    index = []
    with open(os.path.join(args.out, "dump.bin"), "wb") as fh, torch.no_grad():
        def put(name, what, x):
            raw = x.contiguous().view(torch.uint8).cpu().numpy().tobytes()
            fh.write(raw)
            index.append([name, what, len(raw)])

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
    torch.cuda.synchronize()
    with open(os.path.join(args.out, "index.json"), "w") as fh:
        json.dump(dict(library=args.lib or "product", cases=2 * len(GRID), tensors=index), fh)
    print("dumped", 2 * len(GRID), "cases,", sum(n for *_, n in index), "bytes to", args.out)


def compare(args):
    import numpy as np
    docs = [json.load(open(os.path.join(d, "index.json"))) for d in args.dirs]
    assert docs[0]["tensors"] == docs[1]["tensors"], "the dumps are of other cases"
    files = [open(os.path.join(d, "dump.bin"), "rb") for d in args.dirs]
    differing = total = 0
    for _, _, n in docs[0]["tensors"]:  # (tensor by tensor: the dumps are gigabytes)
        x, y = (np.frombuffer(f.read(n), dtype=np.uint8) for f in files)
        assert x.size == n and y.size == n, "a dump is shorter than its index"
        differing += int(np.count_nonzero(x != y))
        total += n
    res = dict(cases=docs[0]["cases"], tensors=len(docs[0]["tensors"]), bytes=total,
               libraries=[d["library"] for d in docs], differing_bytes=differing, same_bits=differing == 0)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res))
    return 0 if differing == 0 else 1


def speed(args):
    runs = json.load(open(args.runs))
    res, ok = {}, True
    for setting, side in runs.items():
        assert len(side["parent"]) in (1, 2) and side["new"], f"{setting}: one (interleaved rounds) or two runs per library"
        pm = [statistics.median(r) for r in side["parent"]]
        spread = max((max(r) - min(r)) / statistics.median(r) for r in side["parent"])
        rerun = abs(pm[0] - pm[-1]) / min(pm)
        margin = max(spread, rerun)
        parent = statistics.median([x for r in side["parent"] for x in r])
        new = statistics.median([x for r in side["new"] for x in r])
        verdict = bool(new <= parent * (1 + margin))
        ok = ok and verdict
        res[setting] = dict(parent_median_ms=parent, new_median_ms=new, parent_run_medians_ms=pm, spread=spread,
                            rerun_difference=rerun, margin=margin, new_over_parent=new / parent, no_slower=verdict)
    doc = dict(compared="the median over a library's rounds of both runs", settings=res, no_slower_everywhere=ok)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    for k, v in res.items():
        print(f"{k}: parent {v['parent_median_ms']:.4f} new {v['new_median_ms']:.4f} ms, margin {v['margin']:.3f}",
              "ok" if v["no_slower"] else "SLOWER")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("dump")
    p.add_argument("--lib")
    p.add_argument("--out", required=True)
    p = sub.add_parser("compare")
    p.add_argument("dirs", nargs=2)
    p.add_argument("--out", required=True)
    p = sub.add_parser("speed")
    p.add_argument("--runs", required=True)
    p.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.exit({"dump": dump, "compare": compare, "speed": speed}[args.cmd](args) or 0)


if __name__ == "__main__":
    main()
