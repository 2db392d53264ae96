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
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refactor_check  # noqa: E402  (dump writer, compare, the no-slower rule, the command line; puts the repository on the path)

sys.path.insert(0, os.path.join(refactor_check.ROOT, "tests"))


def dump(dumped):
    import torch
    from waldo_amd import functional as WF
    from test_gpu_token_attention import LARGE_SCORE_CASES, large_score_operands, operands, tile_edge_cases
    from test_gpu_token_attention_bwd import one_key_cases
    dev = torch.device("cuda:0")
    lim = WF.token_attention_limits()
    qt, kt = lim["q_tile"], lim["k_tile"]
    cases = [(f"edge {c}", operands(dev, *c[:6], seed=c[6]), None) for d in (16, 32, 64) for c in tile_edge_cases(qt, kt, d)]
    cases += [(f"large low_rows={low}", large_score_operands(dev, kt, low), None) for low in LARGE_SCORE_CASES]
    cases += [(f"one key {c} scale={s}", operands(dev, *c[:6], seed=c[6]), s) for c, s in one_key_cases(qt)]
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
            dumped.put(name, what, t)
    return len(cases)


def speed_args(p):
    p.add_argument("--parent", nargs="+", required=True)
    p.add_argument("--new", nargs="+", required=True)


def speed_runs(args):
    """tools_dev/ab_lvd_nets.py documents -> the rule's runs: per shape, D and section a run is the tool's median (one
    round), its spread the largest ``spread`` the tool reports for the parent's runs."""
    docs = {side: [json.load(open(p)) for p in paths] for side, paths in (("parent", args.parent), ("new", args.new))}
    runs, spreads = {}, {}
    for d in sorted({doc["head_dim"] for doc in docs["parent"]}):
        side = {s: [doc for doc in ds if doc["head_dim"] == d] for s, ds in docs.items()}
        assert len(side["parent"]) == 2 and len(side["new"]) == 2, f"two runs per library at D={d}"
        for sec, what in (("op", "forward"), ("bwd", "forward+backward")):
            for shape in (k for k, v in side["parent"][0][sec].items() if isinstance(v, dict) and "kernel" in v):
                key = f"D={d} {what} {shape}"
                runs[key] = {s: [[doc[sec][shape]["kernel"]["median_ms"]] for doc in ds] for s, ds in side.items()}
                spreads[key] = max(doc[sec][shape]["spread"] for doc in side["parent"])
    return runs, spreads


if __name__ == "__main__":
    refactor_check.main(__doc__, dump, speed_args, speed_runs)
