"""CPU: the C ABI of the token attention over clips (include/waldo_hip.h "Token attention over clips":
waldo_token_attention_clips_fwd, _fwd_lse, _bwd) and the CPU route of ``WF.token_attention_clips``.  No kernel is launched
and no GPU is touched: every case is refused, or returns, on the host before a launch; the pointers are small integers
that are never dereferenced."""
import ctypes
import itertools
import os

import pytest
import torch

from parity import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("waldo_token_attention_clips_fwd", "waldo_token_attention_clips_fwd_lse", "waldo_token_attention_clips_bwd")


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def views(q=64, qs=384, k=128, ks=384, v=192, vs=384, q_off=4, k_off=8):
    return (q, qs, k, ks, v, vs, q_off, k_off)


SHAPE = dict(scale=0.125, b=2, h=2, d=64, rq=8, rk=10, max_q_len=8, max_k_len=10)
VIEW_KEYS = ("q", "qs", "k", "ks", "v", "vs", "q_off", "k_off")


def split(kw):
    shape = dict(SHAPE)
    shape.update({k: v for k, v in kw.items() if k in shape})
    return views(**{k: v for k, v in kw.items() if k in VIEW_KEYS}), list(shape.values())


def fwd(lib, out=512, **kw):
    vw, shape = split(kw)
    return lib.waldo_token_attention_clips_fwd(*vw, out, *shape, None)


def fwd_lse(lib, out=512, lse=1536, **kw):
    vw, shape = split(kw)
    return lib.waldo_token_attention_clips_fwd_lse(*vw, out, lse, *shape, None)


def bwd(lib, out=512, grad_out=1024, lse=1536, delta=2048, grad_q=4096, grad_k=8192, grad_v=12288, **kw):
    vw, shape = split(kw)
    return lib.waldo_token_attention_clips_bwd(*vw, out, grad_out, lse, delta, grad_q, grad_k, grad_v, *shape, None)


def kinds_of(section, name):
    proto = section[section.index(f"int {name}("):]
    proto = proto[proto.index("(") + 1:proto.index(");")]
    kinds = []
    for arg in proto.split(","):
        arg = " ".join(arg.split())
        kinds.append(ctypes.c_void_p if "*" in arg or arg.startswith("waldo_stream_t") else
                     ctypes.c_int64 if arg.startswith("int64_t") else ctypes.c_float if arg.startswith("float") else
                     ctypes.c_int)
    return kinds


def test_symbols_are_exported_and_match_the_header(lib):
    from waldo_amd import _lib
    header = open(os.path.join(ROOT, "include", "waldo_hip.h")).read()
    sec = header[header.index(" * Token attention over clips:"):]
    for name in NAMES:
        assert hasattr(lib, name), name
        sig = _lib.SIGNATURES[name]
        assert sig[-1] is ctypes.c_void_p
        assert kinds_of(sec, name) == sig, name
    for needle in NAMES + ("IN DEVICE MEMORY", "NO SYNCHRONISATION", "NO ATOMICS", "NO TABLE CONTENT", "NaN",
                           "exact zeros", "not wanted", "OVERWRITTEN", "max_q_len", "max_k_len"):
        assert needle in sec, needle
    # lse follows out in the forward's argument list and nothing else moves
    f, l = kinds_of(sec, NAMES[0]), kinds_of(sec, NAMES[1])
    assert l == f[:9] + [ctypes.c_void_p] + f[9:]
    # the dense section comes first and is what it was: the older tests parse it from its title on
    assert header.index(" * Token attention:") < header.index(" * Token attention over clips:")
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION  # the symbols are additions: the version is unchanged
    # the tiles are the dense section's: no limits call of its own
    assert not hasattr(lib, "waldo_token_attention_clips_limits")


REFUSALS = [
    (dict(q=None), b"null pointer"), (dict(k=None), b"null pointer"), (dict(v=None), b"null pointer"),
    (dict(q_off=None), b"null pointer"), (dict(k_off=None), b"null pointer"),
    (dict(d=48), b"bad head dimension"), (dict(d=0), b"bad head dimension"), (dict(d=128), b"bad head dimension"),
    (dict(b=-1), b"bad shape"), (dict(h=0), b"bad shape"), (dict(rq=-1), b"bad shape"), (dict(rk=-1), b"bad shape"),
    (dict(max_q_len=-1), b"bad clip bound max_q_len=-1"), (dict(max_k_len=-2), b"bad clip bound max_q_len=8 max_k_len=-2"),
    (dict(qs=385), b"bad token stride 385"), (dict(qs=385), b"non-unit inner stride"), (dict(vs=258), b"bad token stride 258"),
    (dict(qs=-384), b"negative stride"), (dict(ks=-4), b"negative stride"),
    (dict(q=68), b"not aligned"), (dict(k=4), b"not aligned"), (dict(v=8), b"not aligned"),
    (dict(scale=float("nan")), b"bad scale"), (dict(scale=float("inf")), b"bad scale"),
    (dict(scale=float("-inf")), b"bad scale"),
    (dict(b=2 ** 31), b"too large"), (dict(rq=2 ** 31), b"too large"), (dict(rk=2 ** 31 - 1), b"too large"),
    (dict(b=2 ** 24, h=8, max_q_len=2 ** 12), b"too large"), (dict(max_q_len=2 ** 31 - 1), b"too large"),
]


@pytest.mark.parametrize("kw,msg", REFUSALS + [(dict(out=None), b"null pointer"), (dict(out=36), b"not aligned")])
def test_fwd_rejects_bad_arguments(lib, kw, msg):
    assert fwd(lib, **kw) == -1, kw
    err = lib.waldo_last_error_string()
    assert err.startswith(b"waldo_token_attention_clips_fwd:") and msg in err, (kw, err)


@pytest.mark.parametrize("kw,msg", REFUSALS + [(dict(out=None), b"null pointer"), (dict(lse=None), b"null pointer"),
                                               (dict(out=36), b"not aligned")])
def test_fwd_lse_rejects_what_the_forward_rejects(lib, kw, msg):
    assert fwd_lse(lib, **kw) == -1, kw
    err = lib.waldo_last_error_string()
    assert err.startswith(b"waldo_token_attention_clips_fwd_lse:") and msg in err, (kw, err)


@pytest.mark.parametrize("kw,msg", REFUSALS + [
    (dict(out=None), b"null pointer"), (dict(grad_out=None), b"null pointer"), (dict(lse=None), b"null pointer"),
    (dict(delta=None), b"null pointer"),
    (dict(out=36), b"not aligned"), (dict(grad_out=1028), b"not aligned"), (dict(lse=1540), b"not aligned"),
    (dict(delta=2056), b"not aligned"), (dict(grad_q=4100), b"not aligned"), (dict(grad_k=8200), b"not aligned"),
    (dict(grad_v=12292), b"not aligned"),
    (dict(b=2 ** 20, h=8, max_q_len=1, max_k_len=2 ** 14), b"too large"),   # the key blocks of all (clip, h)
])
def test_bwd_rejects_bad_arguments(lib, kw, msg):
    assert bwd(lib, **kw) == -1, kw
    err = lib.waldo_last_error_string()
    assert err.startswith(b"waldo_token_attention_clips_bwd:") and msg in err, (kw, err)


def test_the_shared_refusals_have_the_dense_sections_words(lib):
    """Head dimension, scale and the strides: the dense forward's messages, word for word, under the new name."""
    dense = (64, 3072, 384, 128, 3072, 384, 192, 3072, 384, None, 0, 0, None, 0, 0)
    for kw, dkw in ((dict(d=48), dict(d=48)), (dict(scale=float("nan")), dict(scale=float("nan"))),
                    (dict(qs=385), dict(qs=385)), (dict(qs=-384), dict(qs=-384))):
        args = list(dense)
        if "qs" in dkw:
            args[2] = dkw["qs"]
        assert lib.waldo_token_attention_fwd(*args, 512, dkw.get("scale", 0.125), 2, 2, dkw.get("d", 64), 8, 8, 0,
                                             None) == -1
        want = lib.waldo_last_error_string()
        assert fwd(lib, **kw) == -1
        got = lib.waldo_last_error_string()
        assert got == want.replace(b"waldo_token_attention_fwd:", b"waldo_token_attention_clips_fwd:"), (kw, got, want)


def test_calls_with_nothing_to_do_return_ok_without_a_launch(lib):
    null = dict(q=None, k=None, v=None, q_off=None, k_off=None, out=None)
    assert fwd(lib, b=0, **null) == 0
    assert fwd(lib, rq=0, **null) == 0
    assert fwd(lib, b=0, d=48, **null) == -1
    assert fwd(lib, max_q_len=0) == 0                  # no clip has a query: nothing to launch
    assert fwd_lse(lib, b=0, lse=None, **null) == 0
    assert fwd_lse(lib, rq=0, lse=None, **null) == 0
    assert bwd(lib, b=0, grad_out=None, lse=None, delta=None, **null) == 0
    assert bwd(lib, rq=0, grad_out=None, lse=None, delta=None, **null) == 0
    assert bwd(lib, grad_q=None, grad_k=None, grad_v=None) == 0                       # no gradient wanted
    assert bwd(lib, grad_q=None, grad_k=None, grad_v=None, out=None, lse=None) == 0   # (nothing else is looked at)
    assert bwd(lib, grad_q=None, grad_k=None, grad_v=None, d=48) == -1


# ---------------------------------------------------------------- the framework route (CPU)

def WF():
    from waldo_amd import functional
    return functional


def packed(lens, h=2, d=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    rq, rk = sum(n for n, _ in lens), sum(n for _, n in lens)
    qo = torch.tensor([0] + list(itertools.accumulate(n for n, _ in lens)), dtype=torch.int32)
    ko = torch.tensor([0] + list(itertools.accumulate(n for _, n in lens)), dtype=torch.int32)
    return torch.randn(rq, h, d, generator=g), torch.randn(rk, h, d, generator=g), torch.randn(rk, h, d, generator=g), qo, ko


def per_clip_loop(q, k, v, qo, ko, scale=None):
    fw = WF().token_attention_framework
    return torch.cat([fw(q[qo[b]:qo[b + 1]][None], k[ko[b]:ko[b + 1]][None], v[ko[b]:ko[b + 1]][None], scale=scale)[0]
                      for b in range(len(qo) - 1)])


@pytest.mark.parametrize("lens", [[(3, 4), (7, 2), (1, 9), (5, 5)],           # unequal lengths
                                  [(3, 4), (0, 5), (6, 1)],                    # a clip without queries
                                  [(17 * 3, 17 * 3)] * 3],                     # the all-true mask: T N rows each
                         ids=["unequal", "empty-query", "all-true"])
@pytest.mark.parametrize("scale", [None, -0.2])
def test_the_framework_route_is_a_per_clip_loop_of_the_dense_framework_route(lens, scale):
    q, k, v, qo, ko = packed(lens)
    mq, mk = max(n for n, _ in lens), max(n for _, n in lens)
    got = WF().token_attention_clips_framework(q, k, v, qo, ko, mq, mk, scale=scale)
    want = per_clip_loop(q, k, v, qo, ko, scale)
    assert got.shape == want.shape == (q.shape[0], 32)
    assert (got - want).abs().max().item() <= TOL
    # gradients too, the keys of the clip without queries at exact zero
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]
    go = torch.randn(got.shape, generator=torch.Generator().manual_seed(1))
    WF().token_attention_clips_framework(*leaves, qo, ko, mq, mk, scale=scale).backward(go)
    ref = [t.clone().requires_grad_() for t in (q, k, v)]
    per_clip_loop(*ref, qo, ko, scale).backward(go)
    for a, b in zip(leaves, ref):
        assert (a.grad - b.grad).abs().max().item() <= TOL
    for b, (nq, _) in enumerate(lens):
        if nq == 0:
            assert torch.count_nonzero(leaves[1].grad[ko[b]:ko[b + 1]]) == 0
            assert torch.count_nonzero(leaves[2].grad[ko[b]:ko[b + 1]]) == 0


def test_queries_without_keys_are_nan_rows_in_the_framework_route():
    q, k, v, qo, ko = packed([(3, 4), (2, 0), (6, 1)])
    out = WF().token_attention_clips_framework(q, k, v, qo, ko, 6, 4)
    assert torch.isnan(out[3:5]).all() and torch.isfinite(out[:3]).all() and torch.isfinite(out[5:]).all()


@pytest.mark.parametrize("route", ["kernel", "framework"])
def test_cpu_tensors_are_the_framework_route_with_its_gradients(route):
    q, k, v, qo, ko = packed([(3, 4), (7, 2), (0, 3), (5, 5)], seed=5)
    go = torch.randn(15, 32, generator=torch.Generator().manual_seed(6))

    def grads(fn):
        leaves = [t.clone().requires_grad_() for t in (q, k, v)]
        out = fn(*leaves, qo, ko, 7, 5)
        out.backward(go)
        return (out.detach(), *[t.grad for t in leaves])

    with WF().token_attention_backward_route(route):
        got = grads(WF().token_attention_clips)
    for x, y in zip(got, grads(WF().token_attention_clips_framework)):
        assert torch.equal(x, y)


def test_the_offsets_helper_counts_the_mask():
    g = torch.Generator().manual_seed(3)
    mask = torch.rand(5, 14, generator=g) < 0.4
    mask[2] = False
    mask[3] = True
    off = WF().clip_offsets(mask, 17)
    assert off.dtype == torch.int32 and off.shape == (6,) and int(off[0]) == 0
    assert (off[1:] - off[:-1]).tolist() == [17 * int(m.sum()) for m in mask]
    assert int(off[-1]) == 17 * int(mask.sum())
    with pytest.raises(ValueError, match="ctx_mask must be"):
        WF().clip_offsets(mask[0], 17)


def test_bad_operands_are_refused():
    q, k, v, qo, ko = packed([(3, 4), (7, 2)])
    wf = WF()
    with pytest.raises(ValueError, match="q must be"):
        wf.token_attention_clips(q[None], k, v, qo, ko, 7, 4)
    with pytest.raises(ValueError, match="k and v must be"):
        wf.token_attention_clips(q, k[:, :1], v, qo, ko, 7, 4)
    with pytest.raises(ValueError, match="q_offsets must be int32"):
        wf.token_attention_clips(q, k, v, qo.long(), ko, 7, 4)
    with pytest.raises(ValueError, match="B \\+ 1 entries each"):
        wf.token_attention_clips(q, k, v, qo, ko[:-1], 7, 4)
    with pytest.raises(ValueError, match="must be >= 0"):
        wf.token_attention_clips(q, k, v, qo, ko, -1, 4)
