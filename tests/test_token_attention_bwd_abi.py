"""CPU: the C ABI of the token attention's backward (include/waldo_hip.h "Token attention": waldo_token_attention_fwd_lse,
waldo_token_attention_bwd and its limits query), the route switch of ``WF.token_attention`` and its CPU route.  No kernel
is launched and no GPU is touched: every case is refused, or returns, on the host before a launch; the pointers are small
integers that are never dereferenced."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("waldo_token_attention_fwd_lse", "waldo_token_attention_bwd", "waldo_token_attention_bwd_limits")


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def views(q=64, qs=(3072, 384), k1=128, k1s=(3072, 384), v1=192, v1s=(3072, 384), k2=256, k2s=(2560, 256), v2=320,
          v2s=(2560, 256)):
    return (q, *qs, k1, *k1s, v1, *v1s, k2, *k2s, v2, *v2s)


def bwd(lib, out=512, grad_out=1024, lse=1536, delta=2048, grad_q=4096, grad_k1=8192, grad_v1=12288, grad_k2=16384,
        grad_v2=20480, scale=0.125, b=2, h=2, d=64, nq=8, nk1=8, nk2=10, **kw):
    """waldo_token_attention_bwd with one argument off."""
    return lib.waldo_token_attention_bwd(*views(**kw), out, grad_out, lse, delta, grad_q, grad_k1, grad_v1, grad_k2,
                                         grad_v2, scale, b, h, d, nq, nk1, nk2, None)


def fwd_lse(lib, out=512, lse=1536, scale=0.125, b=2, h=2, d=64, nq=8, nk1=8, nk2=10, **kw):
    return lib.waldo_token_attention_fwd_lse(*views(**kw), out, lse, scale, b, h, d, nq, nk1, nk2, None)


def kinds_of(section, name):
    """The ctypes kinds of a prototype's arguments, one to one: pointers, 64-bit strides, a float, the shape, the stream."""
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
    for name in NAMES:
        assert hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "waldo_hip.h")).read()
    sec = header[header.index(" * Token attention:"):]
    for needle in NAMES + ("NO SCORE-SIZED MEMORY", "NO ATOMICS", "forward and backward", "m + log(l)", "not wanted"):
        assert needle in sec, needle
    assert "forward only" not in sec
    for name in ("waldo_token_attention_fwd_lse", "waldo_token_attention_bwd"):
        sig = _lib.SIGNATURES[name]
        assert sig[-1] is ctypes.c_void_p
        assert kinds_of(sec, name) == sig, name
    assert "waldo_token_attention_bwd_limits" in _lib.PLAIN
    # the new prototypes come after the forward's, which the older tests parse as the first of the section
    assert sec.index("int waldo_token_attention_fwd(") < sec.index("int waldo_token_attention_fwd_lse(")
    assert sec.index("int waldo_token_attention_fwd(") < sec.index("int waldo_token_attention_bwd(")
    # lse follows out in the forward's argument list and nothing else moves
    fwd, lse = kinds_of(sec, "waldo_token_attention_fwd"), kinds_of(sec, "waldo_token_attention_fwd_lse")
    assert lse == fwd[:16] + [ctypes.c_void_p] + fwd[16:]
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION  # the symbols are additions: the version is unchanged


def test_the_backward_lives_in_a_file_of_its_own():
    from waldo_amd import build
    assert os.path.join(build.CSRC, "token_attention_bwd.hip") in build.sources()
    assert os.path.join(build.CSRC, "token_attention.hip") in build.sources()


def test_limits(lib):
    from waldo_amd import functional as WF
    lim = WF.token_attention_bwd_limits()
    assert set(lim) == {"q_tile", "k_tile", "head_dims"}
    assert lim["head_dims"] == (16, 32, 64) == WF.token_attention_limits()["head_dims"]
    assert lim["q_tile"] >= 16 and lim["q_tile"] % 16 == 0 and lim["k_tile"] >= 16 and lim["k_tile"] % 16 == 0
    buf = (ctypes.c_int * 1)()
    assert lib.waldo_token_attention_bwd_limits(buf, 1) == 5 and buf[0] == lim["q_tile"]
    assert lib.waldo_token_attention_bwd_limits(None, 0) == 5
    # the forward's five values are what they were
    fbuf = (ctypes.c_int * 8)()
    assert lib.waldo_token_attention_limits(fbuf, 8) == 5 and list(fbuf)[:5] == [64, 64, 16, 32, 64]


REFUSALS = [
    (dict(q=None), b"null pointer"), (dict(k1=None), b"null pointer"), (dict(v1=None), b"null pointer"),
    (dict(k2=None), b"null pointer"), (dict(v2=None), b"null pointer"),
    (dict(d=48), b"bad head dimension"), (dict(d=0), b"bad head dimension"), (dict(d=128), b"bad head dimension"),
    (dict(d=8), b"bad head dimension"),
    (dict(nk1=0), b"bad shape"), (dict(nk1=-1), b"bad shape"), (dict(nk2=-1), b"bad shape"), (dict(nq=-1), b"bad shape"),
    (dict(b=-1), b"bad shape"), (dict(h=0), b"bad shape"),
    (dict(qs=(3072, 385)), b"bad token stride 385"), (dict(qs=(3072, 385)), b"non-unit inner stride"),
    (dict(v2s=(2560, 258)), b"bad token stride 258"),
    (dict(k1s=(3073, 384)), b"bad batch stride 3073"),
    (dict(qs=(-3072, 384)), b"negative stride"), (dict(k2s=(2560, -256)), b"negative stride"),
    (dict(q=68), b"not aligned"), (dict(v1=8), b"not aligned"), (dict(k2=4), b"not aligned"),
    (dict(scale=float("nan")), b"bad scale"), (dict(scale=float("inf")), b"bad scale"),
    (dict(b=2 ** 31), b"too large"), (dict(nk1=2 ** 31 - 1, nk2=2 ** 31 - 1), b"too large"),
    (dict(b=2 ** 24, h=8, nq=2 ** 12), b"too large"),
]


@pytest.mark.parametrize("kw,msg", REFUSALS + [
    (dict(out=None), b"null pointer"), (dict(grad_out=None), b"null pointer"), (dict(lse=None), b"null pointer"),
    (dict(delta=None), b"null pointer"),
    (dict(out=36), b"not aligned"), (dict(grad_out=1028), b"not aligned"), (dict(lse=1540), b"not aligned"),
    (dict(delta=2056), b"not aligned"),
    (dict(grad_q=4100), b"not aligned"), (dict(grad_k1=8200), b"not aligned"), (dict(grad_v1=12292), b"not aligned"),
    (dict(grad_k2=16388), b"not aligned"), (dict(grad_v2=20484), b"not aligned"),
    (dict(b=2 ** 20, h=8, nq=1, nk1=2 ** 14), b"too large"),   # the key blocks of all (b, h)
])
def test_bwd_rejects_bad_arguments(lib, kw, msg):
    assert bwd(lib, **kw) == -1, kw
    err = lib.waldo_last_error_string()
    assert err.startswith(b"waldo_token_attention_bwd:") and msg in err, (kw, err)


@pytest.mark.parametrize("kw,msg", REFUSALS + [(dict(out=None), b"null pointer"), (dict(lse=None), b"null pointer"),
                                               (dict(out=36), b"not aligned")])
def test_fwd_lse_rejects_what_the_forward_rejects(lib, kw, msg):
    assert fwd_lse(lib, **kw) == -1, kw
    err = lib.waldo_last_error_string()
    assert err.startswith(b"waldo_token_attention_fwd_lse:") and msg in err, (kw, err)


def test_the_messages_are_the_forwards_under_another_name(lib):
    """Every refusal the forward makes, word for word, with the function's own name in front."""
    for kw, _ in REFUSALS:
        args = views(**{k: v for k, v in kw.items() if k in ("q", "qs", "k1", "k1s", "v1", "v1s", "k2", "k2s", "v2", "v2s")})
        shape = dict(scale=0.125, b=2, h=2, d=64, nq=8, nk1=8, nk2=10)
        shape.update({k: v for k, v in kw.items() if k in shape})
        assert lib.waldo_token_attention_fwd(*args, 512, *shape.values(), None) == -1
        want = lib.waldo_last_error_string()
        assert bwd(lib, **kw) == -1
        got = lib.waldo_last_error_string()
        assert got == want.replace(b"waldo_token_attention_fwd:", b"waldo_token_attention_bwd:"), (kw, got, want)


def test_calls_with_nothing_to_do_return_ok_without_a_launch(lib):
    none = dict(grad_q=None, grad_k1=None, grad_v1=None, grad_k2=None, grad_v2=None)
    assert bwd(lib, **none) == 0                        # no gradient wanted
    assert bwd(lib, **none, out=None, lse=None) == 0    # (nothing else is looked at then; a bad D still is)
    assert bwd(lib, **none, d=48) == -1
    # a single segment: the second one's gradients are not wanted whatever the pointers say
    assert bwd(lib, nk2=0, grad_q=None, grad_k1=None, grad_v1=None, grad_k2=4, grad_v2=4) == 0
    null = dict(q=None, k1=None, v1=None, k2=None, v2=None, out=None, grad_out=None, lse=None, delta=None)
    assert bwd(lib, b=0, **null) == 0
    assert bwd(lib, nq=0, **null) == 0
    assert bwd(lib, b=0, d=48, **null) == -1
    assert fwd_lse(lib, b=0, q=None, k1=None, v1=None, k2=None, v2=None, out=None, lse=None) == 0
    assert fwd_lse(lib, nq=0, q=None, out=None, lse=None) == 0


def test_the_route_switch():
    from waldo_amd import functional as WF
    default = WF.get_token_attention_backward_route()
    assert default in WF.TOKEN_ATTENTION_BACKWARD_ROUTES == ("kernel", "framework")
    for bad in ("Kernel", "sdpa", None, True, ""):
        with pytest.raises(ValueError, match="route must be one of"):
            WF.token_attention_backward_route(bad)
        assert WF.get_token_attention_backward_route() == default
    other = "kernel" if default == "framework" else "framework"
    with WF.token_attention_backward_route(other):
        assert WF.get_token_attention_backward_route() == other
        with WF.token_attention_backward_route(default):            # nests
            assert WF.get_token_attention_backward_route() == default
            with WF.token_attention_backward_route(other):
                assert WF.get_token_attention_backward_route() == other
            assert WF.get_token_attention_backward_route() == default
        assert WF.get_token_attention_backward_route() == other
    assert WF.get_token_attention_backward_route() == default
    with pytest.raises(RuntimeError, match="inside"):               # restores on exception
        with WF.token_attention_backward_route(other):
            raise RuntimeError("inside")
    assert WF.get_token_attention_backward_route() == default
    try:                                                            # a setter when not entered
        WF.token_attention_backward_route(other)
        assert WF.get_token_attention_backward_route() == other
    finally:
        WF.token_attention_backward_route(default)
    assert WF.get_token_attention_backward_route() == default


@pytest.mark.parametrize("route", ["kernel", "framework"])
def test_cpu_tensors_are_the_framework_route_with_its_gradients(route):
    from waldo_amd import functional as WF
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(2, 7, 3, 2, 16, generator=g)
    kv = torch.randn(2, 5, 2, 2, 16, generator=g)
    go = torch.randn(2, 7, 32, generator=g)

    def grads(fn):
        a, b = qkv.clone().requires_grad_(), kv.clone().requires_grad_()
        out = fn(*a.unbind(2), *b.unbind(2))
        out.backward(go)
        return out.detach(), a.grad, b.grad

    with WF.token_attention_backward_route(route):
        got = grads(WF.token_attention)
    for x, y in zip(got, grads(WF.token_attention_framework)):
        assert torch.equal(x, y)
