"""CPU: the C ABI of the 16-bit token attention's backward -- waldo_token_attention_fwd_lse_dt and
waldo_token_attention_bwd_dt (include/waldo_hip.h "Token attention on 16-bit operands").  No kernel is launched and no
GPU is touched: every case is refused, or returns, on the host before a launch; the pointers are small integers that are
never dereferenced."""
import ctypes
import os

import pytest

from test_token_attention_bwd_abi import kinds_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, BF16 = 0, 1, 2   # enum waldo_dtype
LSE, BWD = "waldo_token_attention_fwd_lse_dt", "waldo_token_attention_bwd_dt"


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
        grad_v2=20480, scale=0.125, b=2, h=2, d=64, nq=8, nk1=8, nk2=10, dtype=BF16, **kw):
    """waldo_token_attention_bwd_dt with one argument off."""
    return lib.waldo_token_attention_bwd_dt(*views(**kw), out, grad_out, lse, delta, grad_q, grad_k1, grad_v1, grad_k2,
                                            grad_v2, scale, b, h, d, nq, nk1, nk2, dtype, None)


def fwd_lse(lib, out=512, lse=1536, scale=0.125, b=2, h=2, d=64, nq=8, nk1=8, nk2=10, dtype=BF16, **kw):
    return lib.waldo_token_attention_fwd_lse_dt(*views(**kw), out, lse, scale, b, h, d, nq, nk1, nk2, dtype, None)


def message(lib):
    return lib.waldo_last_error_string()


def test_symbols_are_exported_declared_and_bound(lib):
    from waldo_amd import _lib
    header = open(os.path.join(ROOT, "include", "waldo_hip.h")).read()
    sec = header[header.index("/* Token attention on 16-bit operands"):]
    for name, fp32, nargs in ((LSE, "waldo_token_attention_fwd_lse", 26), (BWD, "waldo_token_attention_bwd", 33)):
        assert hasattr(lib, name), name
        sig = _lib.SIGNATURES[name]
        assert len(sig) == nargs and sig[-1] is ctypes.c_void_p and sig[-2] is ctypes.c_int
        assert sig[:-2] == _lib.SIGNATURES[fp32][:-1]   # the fp32 prototype, a dtype code before the stream
        assert kinds_of(sec, name) == sig
        proto = sec[sec.index(f"int {name}("):]
        proto = proto[:proto.index(";")]
        assert proto.count(",") + 1 == nargs and "int dtype, waldo_stream_t stream)" in " ".join(proto.split())
    # lse follows out, as fp32; the views, out, grad_out and the gradients of the backward are void*, lse and delta float*
    proto = " ".join(sec[sec.index(f"int {LSE}("):sec.index(f"int {BWD}(")].split())
    assert "void* out, float* lse, float scale" in proto
    proto = " ".join(sec[sec.index(f"int {BWD}("):].split())
    assert ("const void* out, const void* grad_out, const float* lse, float* delta, void* grad_q, void* grad_k1, "
            "void* grad_v1, void* grad_k2, void* grad_v2, float scale") in proto
    comment = sec[:sec.index("*/")]
    for needle in (LSE, BWD, "m + log(l)", "OVERWRITTEN", "not wanted", "three launches at the most", "no atomics",
                   "no _lse form and no backward on 16-bit operands for"):
        assert needle in " ".join(comment.replace(" * ", " ").split()), needle
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION   # additions only: the version is unchanged


def test_the_backward_lives_in_a_file_of_its_own():
    from waldo_amd import build
    assert os.path.join(build.CSRC, "token_attention_16_bwd.hip") in build.sources()


def test_f32_is_refused_with_the_name_of_the_fp32_entry_point(lib):
    assert bwd(lib, dtype=F32) == -1
    assert message(lib).startswith(b"waldo_token_attention_bwd_dt:")
    assert message(lib).endswith(b"WALDO_DTYPE_F32 is served by waldo_token_attention_bwd")
    assert fwd_lse(lib, dtype=F32) == -1
    assert message(lib).startswith(b"waldo_token_attention_fwd_lse_dt:")
    assert message(lib).endswith(b"WALDO_DTYPE_F32 is served by waldo_token_attention_fwd_lse")


@pytest.mark.parametrize("dtype", [-1, 3, 7, 1 << 20])
def test_an_unknown_dtype_is_refused_before_anything_else(lib, dtype):
    assert bwd(lib, q=None, d=48, nk1=0, dtype=dtype) == -1 and b"unknown dtype" in message(lib)
    assert fwd_lse(lib, q=None, d=48, nk1=0, dtype=dtype) == -1 and b"unknown dtype" in message(lib)


REFUSALS = [
    (dict(q=None), b"null pointer"), (dict(k1=None), b"null pointer"), (dict(v1=None), b"null pointer"),
    (dict(k2=None), b"null pointer"), (dict(v2=None), b"null pointer"),
    (dict(d=48), b"bad head dimension D=48 (16, 32 or 64)"), (dict(d=0), b"bad head dimension"),
    (dict(d=128), b"bad head dimension"), (dict(d=8), b"bad head dimension"),
    (dict(nk1=0), b"bad shape"), (dict(nk1=-1), b"bad shape"), (dict(nk2=-1), b"bad shape"), (dict(nq=-1), b"bad shape"),
    (dict(b=-1), b"bad shape"), (dict(h=0), b"bad shape"),
    (dict(qs=(3072, 385)), b"bad token stride 385"), (dict(qs=(3072, 385)), b"non-unit inner stride"),
    (dict(v2s=(2560, 260)), b"bad token stride 260"),          # a multiple of 4, which the fp32 entry point takes
    (dict(v2s=(2560, 260)), b"a multiple of 8 values"),
    (dict(k1s=(3076, 384)), b"bad batch stride 3076"),
    (dict(qs=(-3072, 384)), b"negative stride"), (dict(k2s=(2560, -256)), b"negative stride"),
    (dict(q=68), b"not aligned"), (dict(v1=8), b"not aligned"), (dict(k2=4), b"not aligned"),
    (dict(scale=float("nan")), b"bad scale"), (dict(scale=float("inf")), b"bad scale"),
    (dict(b=2 ** 31), b"too large"), (dict(nk1=2 ** 31 - 1, nk2=2 ** 31 - 1), b"too large"),
    (dict(b=2 ** 24, h=8, nq=2 ** 12), b"too large"),
]


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("kw,msg", REFUSALS + [
    (dict(out=None), b"null pointer"), (dict(grad_out=None), b"null pointer"), (dict(lse=None), b"null pointer"),
    (dict(delta=None), b"null pointer"),
    (dict(out=36), b"not aligned"), (dict(grad_out=1028), b"not aligned"), (dict(lse=1540), b"not aligned"),
    (dict(delta=2056), b"not aligned"),
    (dict(grad_q=4100), b"not aligned"), (dict(grad_k1=8200), b"not aligned"), (dict(grad_v1=12292), b"not aligned"),
    (dict(grad_k2=16388), b"not aligned"), (dict(grad_v2=20484), b"not aligned"),
    (dict(b=2 ** 20, h=8, nq=1, nk1=2 ** 14), b"too large"),   # the key blocks of all (b, h)
])
def test_bwd_refuses(lib, dtype, kw, msg):
    assert bwd(lib, dtype=dtype, **kw) == -1, kw
    assert message(lib).startswith(b"waldo_token_attention_bwd_dt: ") and msg in message(lib), (kw, message(lib))


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("kw,msg", REFUSALS + [(dict(out=None), b"null pointer"), (dict(lse=None), b"null pointer"),
                                               (dict(out=36), b"not aligned"), (dict(lse=1540), b"not aligned")])
def test_fwd_lse_refuses_what_the_forward_refuses(lib, dtype, kw, msg):
    assert fwd_lse(lib, dtype=dtype, **kw) == -1, kw
    assert message(lib).startswith(b"waldo_token_attention_fwd_lse_dt: ") and msg in message(lib), (kw, message(lib))


def test_the_messages_are_the_16_bit_forwards_under_another_name(lib):
    """Every refusal the 16-bit forward makes, word for word, with the function's own name in front."""
    for kw, _ in REFUSALS:
        args = views(**{k: v for k, v in kw.items() if k in ("q", "qs", "k1", "k1s", "v1", "v1s", "k2", "k2s", "v2", "v2s")})
        shape = dict(scale=0.125, b=2, h=2, d=64, nq=8, nk1=8, nk2=10)
        shape.update({k: v for k, v in kw.items() if k in shape})
        assert lib.waldo_token_attention_fwd_dt(*args, 512, *shape.values(), BF16, None) == -1
        want = message(lib)
        for call, name in ((bwd, BWD), (fwd_lse, LSE)):
            assert call(lib, **kw) == -1
            assert message(lib) == want.replace(b"waldo_token_attention_fwd_dt:", name.encode() + b":"), (kw, name)


def test_the_refusals_come_in_the_fp32_backwards_order(lib):
    """dtype, shape, head dimension, scale, size, strides, (empty / nothing wanted: ok), pointers."""
    order = [(dict(dtype=9), b"unknown dtype"), (dict(nk1=0), b"bad shape"), (dict(d=48), b"bad head dimension"),
             (dict(scale=float("nan")), b"bad scale"), (dict(b=2 ** 31), b"too large"),
             (dict(qs=(3072, 4)), b"bad token stride"), (dict(lse=None), b"null pointer"), (dict(grad_v2=8), b"not aligned")]
    for i, (_, msg) in enumerate(order):
        kw = {}
        for later, _ in order[i:]:
            kw.update(later)
        assert bwd(lib, **kw) == -1 and msg in message(lib), (kw, message(lib))


def test_calls_with_nothing_to_do_return_ok_without_a_launch(lib):
    none = dict(grad_q=None, grad_k1=None, grad_v1=None, grad_k2=None, grad_v2=None)
    null = dict(q=None, k1=None, v1=None, k2=None, v2=None, out=None, grad_out=None, lse=None, delta=None)
    for dtype in (F16, BF16):
        assert bwd(lib, dtype=dtype, **none) == 0                        # no gradient wanted
        assert bwd(lib, dtype=dtype, **none, out=None, lse=None) == 0    # (nothing else is looked at then; a bad D still is)
        assert bwd(lib, dtype=dtype, **none, d=48) == -1
        # a single segment: the second one's gradients are not wanted whatever the pointers say
        assert bwd(lib, dtype=dtype, nk2=0, grad_q=None, grad_k1=None, grad_v1=None, grad_k2=4, grad_v2=4) == 0
        assert bwd(lib, dtype=dtype, b=0, **null) == 0
        assert bwd(lib, dtype=dtype, nq=0, **null) == 0
        assert bwd(lib, dtype=dtype, b=0, d=48, **null) == -1
        assert fwd_lse(lib, dtype=dtype, b=0, q=None, k1=None, v1=None, k2=None, v2=None, out=None, lse=None) == 0
        assert fwd_lse(lib, dtype=dtype, nq=0, q=None, out=None, lse=None) == 0
    assert bwd(lib, dtype=F32, **none) == -1                             # the dtype's refusal comes before that
