"""dev: is a rebuilt token attention (csrc/token_attention*.hip) the parent's, bit for bit and in time?

    python tools_dev/ta_refactor_check.py dump --lib PARENT.so --out DIR_A     # one process per library
    python tools_dev/ta_refactor_check.py dump --out DIR_B                     # the product library
    python tools_dev/ta_refactor_check.py compare DIR_A DIR_B --out bits.json
    python tools_dev/ta_refactor_check.py speed --parent P1.json P2.json --new N1.json N2.json --out speed.json

dump   writes out (with and without autograd: both forward instances), lse and the five gradients under the kernel route
       of every case of tests/test_gpu_token_attention.py's tile_edge_cases at D = 16, 32, 64, of its two large-score
       cases and of tests/test_gpu_token_attention_bwd.py's one-key cases, as raw bytes in one file with an index.
compare counts the differing bytes of two dumps (required: 0) .
speed  reads tools_dev/ab_lvd_nets.py documents (sections op,bwd; any number of head dimensions per side, two runs
       each, taken in the order parent, new, parent, new): per shape and D the new medians of the kernel's forward and
       of its forward + backward against the parent's medians x (1 + margin), margin = the larger of the tool's
       ``spread`` and of the relative difference between the two runs of one library."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def dump(args):
    import torch
    from waldo_amd import _lib, functional as WF
    if args.lib:
        _lib.use_library(args.lib)
    from test_gpu_token_attention import LARGE_SCORE_CASES, large_score_operands, operands, tile_edge_cases
    from test_gpu_token_attention_bwd import one_key_cases
    dev = torch.device("cuda:0")
    lim = WF.token_attention_limits()
    qt, kt = lim["q_tile"], lim["k_tile"]
    cases = [(f"edge {c}", operands(dev, *c[:6], seed=c[6]), None) for d in (16, 32, 64) for c in tile_edge_cases(qt, kt, d)]
    cases += [(f"large low_rows={low}", large_score_operands(dev, kt, low), None) for low in LARGE_SCORE_CASES]
    cases += [(f"one key {c} scale={s}", operands(dev, *c[:6], seed=c[6]), s) for c, s in one_key_cases(qt)]
    os.makedirs(args.out, exist_ok=True)
    index = []
    with open(os.path.join(args.out, "dump.bin"), "wb") as fh:
        for i, (name, ops, scale) in enumerate(cases):
            assert WF._token_attention_served(*ops) is not None, name
            with torch.no_grad():
                plain = WF.token_attention(*ops, scale)
            leaves = [None if t is None else t.detach().clone().requires_grad_() for t in ops]
            b, nq, h, d = ops[0].shape
            go = torch.randn(b, nq, h * d, generator=torch.Generator().manual_seed(3000 + i)).to(dev)
            with WF.token_attention_backward_route("kernel"):
                out = WF.token_attention(*leaves, scale)
                lse = out.grad_fn.saved_tensors[-1]
                grads = torch.autograd.grad(out, [t for t in leaves if t is not None], go)
            for what, t in (("out_plain", plain), ("out", out.detach()), ("lse", lse), *zip("q k v k2 v2".split(), grads)):
                raw = t.contiguous().cpu().numpy().tobytes()
                fh.write(raw)
                index.append([name, what, len(raw)])
    torch.cuda.synchronize()
    with open(os.path.join(args.out, "index.json"), "w") as fh:
        json.dump(dict(library=args.lib or "product", cases=len(cases), tensors=index), fh)
    print("dumped", len(cases), "cases,", sum(n for *_, n in index), "bytes to", args.out)


def compare(args):
    import numpy as np
    docs = [json.load(open(os.path.join(d, "index.json"))) for d in args.dirs]
    raws = [np.fromfile(os.path.join(d, "dump.bin"), dtype=np.uint8) for d in args.dirs]
    assert docs[0]["tensors"] == docs[1]["tensors"] and raws[0].size == raws[1].size, "the dumps are of other cases"
    differing = int(np.count_nonzero(raws[0] != raws[1]))
    res = dict(cases=docs[0]["cases"], tensors=len(docs[0]["tensors"]), bytes=int(raws[0].size),
               libraries=[d["library"] for d in docs], differing_bytes=differing, same_bits=differing == 0)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res))
    return 0 if differing == 0 else 1


def speed(args):
    runs = {side: [json.load(open(p)) for p in paths] for side, paths in (("parent", args.parent), ("new", args.new))}
    med = lambda doc, sec, shape: doc[sec][shape]["kernel"]["median_ms"]
    res, ok = {}, True
    for d in sorted({doc["head_dim"] for doc in runs["parent"]}):
        side = {s: [doc for doc in docs if doc["head_dim"] == d] for s, docs in runs.items()}
        assert len(side["parent"]) == 2 and len(side["new"]) == 2, f"two runs per library at D={d}"
        for sec, what in (("op", "forward"), ("bwd", "forward+backward")):
            for shape in (k for k, v in side["parent"][0][sec].items() if isinstance(v, dict) and "kernel" in v):
                ms = {s: [med(doc, sec, shape) for doc in docs] for s, docs in side.items()}
                spread = max(doc[sec][shape]["spread"] for docs in side.values() for doc in docs)
                rerun = max(abs(a - b) / min(a, b) for a, b in ms.values())
                margin = max(spread, rerun)
                parent, new = sorted(ms["parent"])[0] / 2 + sorted(ms["parent"])[1] / 2, sum(ms["new"]) / 2
                verdict = bool(new <= parent * (1 + margin))
                ok = ok and verdict
                res[f"D={d} {what} {shape}"] = dict(parent_median_ms=ms["parent"], new_median_ms=ms["new"], spread=spread,
                                                    rerun_difference=rerun, margin=margin, new_over_parent=new / parent,
                                                    no_slower=verdict)
    doc = dict(order="parent, new, parent, new: one process each", compared="the mean of a library's two medians",
               shapes=res, no_slower_everywhere=ok)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    for k, v in res.items():
        print(k, "parent", [round(x, 4) for x in v["parent_median_ms"]], "new", [round(x, 4) for x in v["new_median_ms"]],
              "margin", round(v["margin"], 3), "ok" if v["no_slower"] else "SLOWER")
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
    p.add_argument("--parent", nargs="+", required=True)
    p.add_argument("--new", nargs="+", required=True)
    p.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.exit({"dump": dump, "compare": compare, "speed": speed}[args.cmd](args) or 0)


if __name__ == "__main__":
    main()
