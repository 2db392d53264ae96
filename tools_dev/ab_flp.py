"""A/B of the FLP networks' routes (nets/flp.py) at the shape of scripts/cityscapes/train_flp.sh on one MI355X: 4 clips of
14 frames, 4 context frames, 16 objects (17 tokens per frame), 512 wide, 8 heads (D = 64), depths 2 / 4 / 4.  Writes
profiles/flp_nets.json.

    python tools_dev/ab_flp.py [--out profiles/flp_nets.json] [--rounds 30] [--warmup 5]

Routes, the SAME module and inputs:
  kernel     ``fused = True`` under an integer-built plan (``FLP.plan``): WF.token_attention_clips on the packed tokens,
             no host read anywhere;
  framework  ``fused = False`` under the same plan: WF.token_attention_clips_framework (all Rq x Rk scores under a block
             mask), no host read either;
  reference  the attention as the reference runs it (models/modules/transform.py:100-158), spelled in framework ops on
             the module's own parameters: the packed projection scattered into a dense (B, T N) tensor, all T N keys
             under a -inf mask, the result gathered back -- with the ``any(~mask)`` host read each of the three steps
             makes and boolean-mask indexing.  What surrounds the attention is this package's in all three routes.
Sections: ``forward`` (no autograd), ``step`` (forward, a sum loss, backward to the parameters; the kernel route under
both routes of the attention's backward), ``graph`` (the kernel route's forward eager against replayed from ONE graph).
Method: tools_dev/ab_lvd_nets.py's -- device time between events, the routes ALTERNATE inside one process, median /
minimum / quartiles per route, ``spread`` the largest interquartile range over its median.  ``fused_default`` applies
the rule: the faster of kernel and framework by the forward's medians.  A run without a GPU fails."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ab_lvd_nets import alternate  # noqa: E402
from waldo_amd import functional as WF  # noqa: E402
from waldo_amd.modules import transform  # noqa: E402
from waldo_amd.nets import FLP, flp_net_opt  # noqa: E402

B, T, CTX, NO, NT = 4, 14, 4, 16, 16
OPT = dict(embed_dim=512, num_heads=8, num_obj=NO, latent_shape=[4, 8], obj_shape=[4, 4], pg_com_depth=2, pg_enc_depth=4,
           pg_dec_depth=4, pg_num_timesteps=T, zero_init_dec=False)


def _scatter(packed, mask):
    """The reference's from_ctx: a host read, a dense tensor, a boolean-mask store."""
    if not bool(torch.any(~mask)):
        return packed.reshape(*mask.shape, *packed.shape[1:])
    dense = packed.new_zeros(*mask.shape, *packed.shape[1:])
    dense[mask] = packed
    return dense


def _gather(dense, mask):
    """The reference's to_ctx: a host read and a boolean-mask load."""
    return dense[mask] if bool(torch.any(~mask)) else dense.reshape(-1, *dense.shape[2:])


def _dense_attention(self, q, k, v, masked):
    attn = (q @ k.transpose(-2, -1)) * self.scale
    attn = attn.masked_fill(masked.expand(-1, self.num_heads, -1, -1), float("-inf")).softmax(dim=-1)
    return (attn @ v).transpose(1, 2)


def reference_full(self, x, ctx_mask=None, **kwargs):
    mask = ctx_mask.mask
    (b, t), (_, n, c) = mask.shape, x.shape
    qkv = _scatter(self.qkv(self._noisy(x)), mask).reshape(b, -1, 3, self.num_heads, c // self.num_heads)
    q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
    off = (~mask).view(b, t, 1).expand(-1, -1, n).contiguous()
    masked = off.view(b, 1, 1, t * n) * (~off).view(b, 1, t * n, 1)
    out = _dense_attention(self, q, k, v, masked).reshape(b, t, n, c)
    return self.proj(_gather(out, mask))


def reference_cross(self, x_pred, x_ctx, ctx_mask=None, **kwargs):
    mask = ctx_mask.mask
    (b, t), (_, n, c) = mask.shape, x_pred.shape
    h = self.num_heads
    q = _scatter(self.q(self._noisy(x_pred)), ~mask).reshape(b, -1, h, c // h).permute(0, 2, 1, 3)
    k, v = _scatter(self.kv(x_ctx), mask).reshape(b, -1, 2, h, c // h).permute(2, 0, 3, 1, 4).unbind(0)
    off = (~mask).view(b, t, 1).expand(-1, -1, n).contiguous()
    masked = off.view(b, 1, 1, t * n) * off.view(b, 1, t * n, 1)
    out = _dense_attention(self, q, k, v, masked).reshape(b, t, n, c)
    return self.proj(_gather(out, ~mask))


class reference_attention:
    """``with reference_attention():`` the two masked attentions run the reference's sequence."""

    def __enter__(self):
        self.saved = (transform.FullAttention.forward, transform.CrossAttention.forward)
        transform.FullAttention.forward, transform.CrossAttention.forward = reference_full, reference_cross

    def __exit__(self, *exc):
        transform.FullAttention.forward, transform.CrossAttention.forward = self.saved
        return False


def main_16bit(args, net, forward):
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]
    out = args.out if os.path.basename(args.out) != "flp_nets.json" else os.path.join(ROOT, "profiles", "flp_nets_16bit.json")

    def route(fused, act_dtype):
        def fn():
            net.act_dtype = act_dtype
            return forward(fused)
        return fn

    doc = {}
    if os.path.exists(out):
        with open(out) as fh:
            doc = json.load(fh)
    with torch.no_grad():
        ref, got = route(True, None)(), route(True, dtype)()
        part = dict(shape=dict(clips=B, frames=T, ctx_len=CTX, tokens_per_frame=NO + 1, **OPT),
                    device=torch.cuda.get_device_name(0), rounds=args.rounds, warmup=args.warmup,
                    max_abs_act_dtype_minus_fp32=max((a - b).abs().max().item() for a, b in zip(got, ref)))
        part["forward"] = f = alternate({"fused_act_dtype": route(True, dtype), "fused_fp32": route(True, None),
                                         "framework_autocast": route(False, dtype)}, args.warmup, args.rounds)
    part["act_dtype_over_fp32"] = f["fused_act_dtype"]["median_ms"] / f["fused_fp32"]["median_ms"]
    part["act_dtype_over_framework_autocast"] = f["fused_act_dtype"]["median_ms"] / f["framework_autocast"]["median_ms"]
    doc[args.dtype] = part
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print(json.dumps({k: round(v["median_ms"], 3) for k, v in f.items() if isinstance(v, dict)}), "spread", f["spread"])
    print(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flp_nets.json"))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", choices=("bf16", "fp16"),
                    help="measure act_dtype instead: the forward with act_dtype fused, in fp32 fused and fused = False "
                         "under the same autocast; writes profiles/flp_nets_16bit.json")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    opt = flp_net_opt(**OPT)
    net = FLP(opt).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
    lo, l, c = 16, 32, opt.embed_dim
    inputs = [0.5 * rnd(B, T, NO, lo, 2), 0.5 * rnd(B, T, 1, l, 2), rnd(B, T, NO), rnd(B, NO, NT, c), rnd(B, NT * 2, c),
              None, None]
    plan = net.plan(B, T, CTX, dev)

    def forward(fused, reference=False):
        net.fused = fused
        if reference:
            with reference_attention():
                return net(*inputs, ctx_mask=plan)
        return net(*inputs, ctx_mask=plan)

    if args.dtype:
        return main_16bit(args, net, forward)

    def step(fused, route="framework", reference=False):
        net.zero_grad(set_to_none=True)
        with WF.token_attention_backward_route(route):
            out = forward(fused, reference)
            sum(o.sum() for o in out).backward()

    doc = dict(shape=dict(clips=B, frames=T, ctx_len=CTX, tokens_per_frame=NO + 1, **OPT),
               device=torch.cuda.get_device_name(0), rounds=args.rounds, warmup=args.warmup)
    with torch.no_grad():
        ref, out = forward(False, True), forward(True)
        doc["max_abs_kernel_minus_reference"] = max((a - b).abs().max().item() for a, b in zip(out, ref))
        doc["forward"] = alternate({"kernel": lambda: forward(True), "framework": lambda: forward(False),
                                    "reference": lambda: forward(False, True)}, args.warmup, args.rounds)
    doc["step"] = alternate({"kernel_bwd_kernel": lambda: step(True, "kernel"),
                             "kernel_bwd_framework": lambda: step(True, "framework"),
                             "framework": lambda: step(False), "reference": lambda: step(False, reference=True)},
                            args.warmup, args.rounds)
    # the kernel route's forward from one graph
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            forward(True)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = forward(True)
        graph.replay()
        torch.cuda.synchronize()
        doc["graph_replay_bit_equal"] = all(torch.equal(a, b) for a, b in zip(static, out))
        doc["graph"] = alternate({"eager": lambda: forward(True), "replay": graph.replay}, args.warmup, args.rounds)
    f = doc["forward"]
    doc["fused_default"] = bool(f["kernel"]["median_ms"] <= f["framework"]["median_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    for sec in ("forward", "step", "graph"):
        for k, v in doc[sec].items():
            if isinstance(v, dict):
                print(f"{sec:8s} {k:22s} median {v['median_ms']:8.3f} ms  min {v['min_ms']:8.3f}  "
                      f"IQR [{v['q1_ms']:.3f}, {v['q3_ms']:.3f}]")
        print(f"{sec:8s} spread {doc[sec]['spread']:.3f}")
    print("fused_default", doc["fused_default"], " graph bits", doc["graph_replay_bit_equal"],
          " |kernel - reference|", doc["max_abs_kernel_minus_reference"])


if __name__ == "__main__":
    main()
