"""dev: is a rebuilt kernel family the parent's, bit for bit and in time?  The parts every such check shares -- the dump
writer, the streaming comparison and the no-slower rule -- and the suite of the flow-context backward
(csrc/flow_ctx_bwd.hip, csrc/occ_composite.hip).  tools_dev/ta_refactor_check.py (token attention) and
tools_dev/fwf_refactor_check.py (frame warp) are further case lists on top of this module.

    python tools_dev/refactor_check.py dump --lib PARENT.so --out DIR_A     # one process per library
    python tools_dev/refactor_check.py dump --out DIR_B                     # the product library
    python tools_dev/refactor_check.py compare DIR_A DIR_B --out bits.json
    python tools_dev/refactor_check.py speed --runs RUNS.json --out speed.json

dump    writes, for a fixed, seeded case list, tensors as raw bytes in one file (dump.bin) with an index (index.json).
        The flow-context suite: the gradients of flow_ctx_alpha, flow_ctx_warp and occ_composite (and the forward outputs
        they come from) over every padded layer instance (L = 2, 5, 8, 12, 13, 17, 24, 32), no filter and 20 / 21 / 32
        classes, scale 1 / 2 / 3, a 9 x 20 (last tile partly live) and a 16 x 32 low-resolution raster with Tw < T, the
        ghost mask present and absent, every subset of incoming gradients and of gradients required, and one case whose
        workgroups walk more than one tile (8 units of 128 x 256, L = 4); and flow_ctx_alpha's forward with want_bits on
        an fp32 clip and on the same clip packed, every layer instance at 20 and 32 classes.  In the default mode only what is written
        once per element is dumped (grad_alpha_lr, grad_flow_lr, occ_composite's grad_alpha: grad_occ, grad_dist and
        grad_a01 are summed with float atomics); under deterministic() every gradient.
compare counts the differing bytes of two dumps, tensor by tensor (the dumps may be gigabytes).  Required: 0.
speed   RUNS.json: {setting: {"parent": [[ms of a run's rounds], ...], "new": [[...], ...]}}, the runs taken in the order
        parent, new, parent, new, one process each.  Per setting the new median against the parent's median x (1 +
        margin), margin = the larger of the spread of the parent's own rounds and of the relative difference between
        the parent's two runs (one run: the spread alone)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Dump:
    """dump.bin + index.json under `out`: put(case, what, tensor) appends the tensor's bytes."""

    def __init__(self, out, lib):
        os.makedirs(out, exist_ok=True)
        self.out, self.lib, self.index, self.cases = out, lib, [], set()
        self.fh = open(os.path.join(out, "dump.bin"), "wb")

    def put(self, case, what, x):
        import torch
        raw = x.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()
        self.fh.write(raw)
        self.index.append([case, what, len(raw)])
        self.cases.add(case)

    def close(self, cases=None):
        self.fh.close()
        with open(os.path.join(self.out, "index.json"), "w") as fh:
            json.dump(dict(library=self.lib or "product", cases=cases or len(self.cases), tensors=self.index), fh)
        print("dumped", cases or len(self.cases), "cases,", sum(n for *_, n in self.index), "bytes to", self.out)


def compare(dirs, out):
    import numpy as np
    docs = [json.load(open(os.path.join(d, "index.json"))) for d in dirs]
    assert docs[0]["tensors"] == docs[1]["tensors"], "the dumps are of other cases"
    files = [open(os.path.join(d, "dump.bin"), "rb") for d in dirs]
    differing = total = 0
    where = []
    for case, what, n in docs[0]["tensors"]:  # (tensor by tensor: the dumps are gigabytes)
        x, y = (np.frombuffer(f.read(n), dtype=np.uint8) for f in files)
        assert x.size == n and y.size == n, "a dump is shorter than its index"
        d = int(np.count_nonzero(x != y))
        if d and len(where) < 20:
            where.append([case, what, d])
        differing += d
        total += n
    for f in files:
        f.close()
    res = dict(cases=docs[0]["cases"], tensors=len(docs[0]["tensors"]), bytes=total,
               libraries=[d["library"] for d in docs], differing_bytes=differing, same_bits=differing == 0)
    if where:
        res["first_differing_tensors"] = where
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res))
    return 0 if differing == 0 else 1


def no_slower(runs, spreads=None):
    """The rule over {setting: {"parent": [[ms...], ...], "new": [[...], ...]}}; spreads: {setting: spread} where a run
    is a tool's median and the tool reports the spread of its rounds itself.  Returns (document, ok)."""
    res, ok = {}, True
    for setting, side in runs.items():
        assert len(side["parent"]) in (1, 2) and side["new"], f"{setting}: one or two runs per library"
        pm = [statistics.median(r) for r in side["parent"]]
        spread = (spreads[setting] if spreads else
                  max((max(r) - min(r)) / statistics.median(r) for r in side["parent"]))
        rerun = abs(pm[0] - pm[-1]) / min(pm)
        margin = max(spread, rerun)
        parent = statistics.median([x for r in side["parent"] for x in r])
        new = statistics.median([x for r in side["new"] for x in r])
        verdict = bool(new <= parent * (1 + margin))
        ok = ok and verdict
        res[setting] = dict(parent_median_ms=parent, new_median_ms=new, parent_run_medians_ms=pm, spread=spread,
                            rerun_difference=rerun, margin=margin, new_over_parent=new / parent, no_slower=verdict)
    doc = dict(order="parent, new, parent, new: one process each", compared="the median over a library's rounds of its runs",
               settings=res, no_slower_everywhere=ok)
    return doc, ok


def speed(runs, out, spreads=None):
    doc, ok = no_slower(runs, spreads)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    for k, v in doc["settings"].items():
        print(f"{k}: parent {v['parent_median_ms']:.4f} new {v['new_median_ms']:.4f} ms, margin {v['margin']:.3f}",
              "ok" if v["no_slower"] else "SLOWER")
    return 0 if ok else 1


def main(doc, dump, speed_args=None, speed_runs=None):
    """The command line of a suite: dump(Dump) writes its cases; speed_args(parser) / speed_runs(args) -> (runs, spreads)
    where the suite reads its timings from another tool's documents (default: --runs RUNS.json)."""
    ap = argparse.ArgumentParser(description=doc.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("dump")
    p.add_argument("--lib")
    p.add_argument("--out", required=True)
    p = sub.add_parser("compare")
    p.add_argument("dirs", nargs=2)
    p.add_argument("--out", required=True)
    p = sub.add_parser("speed")
    if speed_args is None:
        p.add_argument("--runs", required=True)
    else:
        speed_args(p)
    p.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.cmd == "dump":
        import torch
        from waldo_amd import _lib
        if args.lib:
            _lib.use_library(args.lib)
        d = Dump(args.out, args.lib)
        cases = dump(d)
        torch.cuda.synchronize()
        d.close(cases)
        sys.exit(0)
    if args.cmd == "compare":
        sys.exit(compare(args.dirs, args.out))
    runs, spreads = speed_runs(args) if speed_runs else (json.load(open(args.runs)), None)
    sys.exit(speed(runs, args.out, spreads))


# ---- the flow-context backward suite ---------------------------------------------------------------------------------
LAYERS = (2, 5, 8, 12, 13, 17, 24, 32)


def alpha_cases():
    """(L, classes or None, scale, (h, w), outputs in the loss, inputs that require a gradient, B)"""
    both, every = ("a01", "alpha"), ("alpha_lr", "dist", "occ")
    cases = [(nl, 20, 1, (9, 20), both, every, 2) for nl in LAYERS]
    cases += [(nl, 20, s, hw, both, every, 2) for nl in (5, 17) for s, hw in ((2, (16, 32)), (3, (9, 20)))]
    cases += [(5, ncls, 1, (9, 20), both, every, 2) for ncls in (None, 21, 32)] + [(17, 32, 2, (9, 20), both, every, 2)]
    cases += [(8, 20, 1, (9, 20), outs, every, 2) for outs in (("a01",), ("alpha",))]
    cases += [(8, 20, 2, (9, 20), both, need, 2) for need in (("alpha_lr", "dist"), ("alpha_lr", "occ"), ("alpha_lr",))]
    return cases


def warp_cases():
    """(L, scale, (h, w), ghost mask, outputs in the loss, inputs that require a gradient)"""
    outs, every = ("flow", "alpha_ctx", "disocc"), ("flow_lr", "a01", "occ")
    cases = [(nl, 1, (9, 20), True, outs, every) for nl in LAYERS]
    cases += [(nl, s, hw, ghost, outs, every) for nl in (5, 17) for s, hw, ghost in ((2, (16, 32), False), (3, (9, 20), True))]
    cases += [(8, 2, (9, 20), True, tuple(o for o in outs if o != drop), every) for drop in outs]
    cases += [(8, 1, (9, 20), False, outs, need) for need in (("flow_lr", "a01"), ("flow_lr", "occ"))]
    return cases


def flow_ctx_dump(d):
    import torch
    from waldo_amd import functional as WF
    dev = torch.device("cuda:0")
    t, tw, tc, tp = 3, 2, 2, 2

    def run_alpha(name, nl, ncls, s, hw, outs, need, b, modes):
        h, w = hw
        g = torch.Generator(device=dev).manual_seed(1000 + nl)
        x = dict(alpha_lr=torch.rand(b * tw, nl, h, w, generator=g, device=dev),
                 dist=None if ncls is None else torch.rand(b, nl - 1, ncls, generator=g, device=dev).softmax(dim=2),
                 occ=torch.rand(b, t, nl, nl, generator=g, device=dev) * 0.5)
        inp = torch.randn(b, t, 3 + (ncls or 1), h * s, w * s, generator=g, device=dev) * 2
        wts = {o: torch.randn(b * tw, nl, h * s, w * s, generator=g, device=dev) for o in ("a01", "alpha")}
        for det in modes:
            lv = {k: (v.clone().requires_grad_(k in need) if v is not None else None) for k, v in x.items()}
            with WF.deterministic(det):
                res = dict(zip(("a01", "alpha"), WF.flow_ctx_alpha(lv["alpha_lr"], inp, lv["dist"], lv["occ"], tw, 3, s)))
                sum((res[o] * wts[o]).sum() for o in outs).backward()
            mode = "det" if det else "default"
            for o, v in res.items():
                d.put(name, f"{mode}: {o}", v)
            for k in need:
                if lv[k] is not None and (det or k == "alpha_lr"):
                    d.put(name, f"{mode}: grad_{k}", lv[k].grad)

    def run_warp(name, nl, s, hw, ghost, outs, need, b, modes):
        h, w = hw
        hd, wd, m = h * s, w * s, b * tc * tp
        g = torch.Generator(device=dev).manual_seed(2000 + nl)
        x = dict(flow_lr=torch.randn(m, nl, 2, h, w, generator=g, device=dev) * (4.0 / wd),
                 a01=torch.rand(b * tw, nl, hd, wd, generator=g, device=dev),
                 occ=torch.rand(b, t, nl, nl, generator=g, device=dev) * 0.5)
        isobj = torch.rand(m, nl - 1, h, w, generator=g, device=dev) * 0.2 + 0.85 if ghost and nl > 1 else None
        ctx_ts = torch.randint(0, tw, (b, tc, tp), generator=g, device=dev)
        pred_ts = torch.randint(0, t, (tp,), generator=g, device=dev)
        shapes = dict(flow=(m, 2, hd, wd), alpha_ctx=(m, nl, hd, wd), disocc=(m, hd, wd))
        wts = {o: torch.randn(*sh, generator=g, device=dev) for o, sh in shapes.items()}
        for det in modes:
            lv = {k: v.clone().requires_grad_(k in need) for k, v in x.items()}
            with WF.deterministic(det):
                res = dict(zip(shapes, WF.flow_ctx_warp(lv["flow_lr"], isobj, lv["a01"], ctx_ts, pred_ts, lv["occ"], tw, s)))
                sum((res[o] * wts[o]).sum() for o in outs).backward()
            mode = "det" if det else "default"
            for o, v in res.items():
                d.put(name, f"{mode}: {o}", v)
            for k in need:
                if det or k == "flow_lr":
                    d.put(name, f"{mode}: grad_{k}", lv[k].grad)

    def run_alpha_fwd(name, nl, ncls, s, hw, b):
        """the forward alone, with want_bits: on an fp32 clip of +-5 layout logits and on the same clip packed"""
        h, w = hw
        hd, wd = h * s, w * s
        g = torch.Generator(device=dev).manual_seed(4000 + nl)
        alpha_lr = torch.rand(b * tw, nl, h, w, generator=g, device=dev)
        alpha_lr[:, 1::2, : h // 2] = 0.0  # layers absent from half of the raster: the active-layer short cuts
        dist = torch.rand(b, nl - 1, ncls, generator=g, device=dev).softmax(dim=2)
        occ = torch.rand(b, t, nl, nl, generator=g, device=dev) * 0.5
        rgb = torch.randint(0, 256, (b, t, 3, hd, wd), generator=g, device=dev, dtype=torch.uint8)
        cls = torch.randint(0, ncls + 1, (b, t, hd, wd), generator=g, device=dev)  # (one id past the classes, too)
        packed = WF.pack_clip(rgb, cls, ncls)
        with torch.no_grad():
            for kind, clip in (("fp32 clip", packed.unpack()), ("packed clip", packed)):
                res = WF.flow_ctx_alpha(alpha_lr, clip, dist, occ, tw, 3, s, want_bits=True)
                for o, v in zip(("a01", "alpha", "layer_bits"), res):
                    d.put(name, f"{kind}: {o}", v)

    n = 0
    for nl in LAYERS:  # (flow_ctx_warp_into_raw is not dumped: flow_ctx_warp_kernel's text is the parent's but for a typedef)
        for ncls, s, hw in ((20, 1, (9, 20)), (32, 2, (16, 32))):
            run_alpha_fwd(f"alpha forward L={nl} Nl={ncls} x{s} {hw}, want_bits", nl, ncls, s, hw, 2)
            n += 1
    for c in alpha_cases():
        run_alpha(f"alpha L={c[0]} Nl={c[1]} x{c[2]} {c[3]} loss={c[4]} grads={c[5]}", *c, modes=(False, True))
        n += 1
    for c in warp_cases():
        run_warp(f"warp L={c[0]} x{c[1]} {c[2]} ghost={c[3]} loss={c[4]} grads={c[5]}", *c, b=2, modes=(False, True))
        n += 1
    # more than one tile per workgroup (units * tiles / 512 >= 2), default mode: 8 units of a 128 x 256 raster
    run_alpha("alpha L=4 128x256, 8 units", 4, 20, 1, (128, 256), ("a01", "alpha"), ("alpha_lr", "dist", "occ"), 4, (False,))
    run_warp("warp L=4 128x256, 8 units", 4, 1, (128, 256), True, ("flow", "alpha_ctx", "disocc"), ("flow_lr", "a01", "occ"),
             2, (False,))
    n += 2
    for nl in (5, 9, 17, 32):
        for div in (1, 3):
            g = torch.Generator(device=dev).manual_seed(3000 + nl)
            alpha = torch.rand(6, nl, 9, 20, generator=g, device=dev)
            occ = torch.rand(6 // div, nl, nl, generator=g, device=dev) * 0.5
            go = torch.randn(6, nl, 9, 20, generator=g, device=dev)
            for det in (False, True):
                a, o = alpha.clone().requires_grad_(), occ.clone().requires_grad_()
                with WF.deterministic(det):
                    (WF.occ_composite(a, o, div) * go).sum().backward()
                name, mode = f"occ_composite L={nl} occ_div={div}", "det" if det else "default"
                d.put(name, f"{mode}: grad_alpha", a.grad)
                if det:
                    d.put(name, f"{mode}: grad_occ", o.grad)
            n += 1
    return n


if __name__ == "__main__":
    main(__doc__, flow_ctx_dump)
