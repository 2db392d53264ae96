"""CPU: the C ABI of the 16-bit token attention -- waldo_token_attention_fwd_dt, waldo_token_attention_clips_fwd_dt and
waldo_token_attention_dt_limits (include/waldo_hip.h "Token attention on 16-bit operands").  No kernel is launched and
no GPU is touched: every case is refused on the host before a launch; the pointers are small integers that are never
dereferenced."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, BF16 = 0, 1, 2   # enum waldo_dtype


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def dense(lib, q=16, qs=(4096, 64), k1=32, k1s=(4096, 64), v1=48, v1s=(4096, 64), k2=64, k2s=(4096, 64), v2=80,
          v2s=(4096, 64), out=96, scale=0.125, b=2, h=1, d=64, nq=64, nk1=64, nk2=9, dtype=BF16):
    """waldo_token_attention_fwd_dt with one argument off."""
    return lib.waldo_token_attention_fwd_dt(q, *qs, k1, *k1s, v1, *v1s, k2, *k2s, v2, *v2s, out, scale, b, h, d, nq, nk1,
                                            nk2, dtype, None)


def clips(lib, q=16, qs=64, k=32, ks=64, v=48, vs=64, q_off=64, k_off=68, out=96, scale=0.125, b=2, h=1, d=64, rq=100,
          rk=100, max_q=64, max_k=64, dtype=BF16):
    return lib.waldo_token_attention_clips_fwd_dt(q, qs, k, ks, v, vs, q_off, k_off, out, scale, b, h, d, rq, rk, max_q,
                                                  max_k, dtype, None)


def message(lib):
    return lib.waldo_last_error_string()


def test_symbols_are_exported_declared_and_bound(lib):
    from waldo_amd import _lib
    header = open(os.path.join(ROOT, "include", "waldo_hip.h")).read()
    for name, nargs in (("waldo_token_attention_fwd_dt", 25), ("waldo_token_attention_clips_fwd_dt", 19)):
        assert hasattr(lib, name), name
        sig = _lib.SIGNATURES[name]
        assert len(sig) == nargs and sig[-1] is ctypes.c_void_p and sig[-2] is ctypes.c_int
        assert sig[:-2] == _lib.SIGNATURES[name[:-3]][:-1]   # the fp32 prototype, a dtype code before the stream
        proto = header[header.index(f"int {name}("):]
        proto = proto[:proto.index(";")]
        assert proto.count(",") + 1 == nargs and "int dtype, waldo_stream_t stream)" in proto
    assert "int waldo_token_attention_dt_limits(int* out, int n);" in header
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION   # additions only: the version is unchanged


def test_the_limits_are_the_fp32_kernels(lib):
    buf = (ctypes.c_int * 8)()
    assert lib.waldo_token_attention_dt_limits(buf, 8) == 5 and list(buf)[:5] == [64, 64, 16, 32, 64]
    short = (ctypes.c_int * 2)()
    assert lib.waldo_token_attention_dt_limits(short, 2) == 5 and list(short) == [64, 64]
    assert lib.waldo_token_attention_dt_limits(None, 0) == 5
    from waldo_amd import functional as WF
    assert WF.token_attention_16bit_limits() == WF.token_attention_limits()


def test_f32_is_refused_with_the_name_of_the_fp32_entry_point(lib):
    assert dense(lib, dtype=F32) == -1
    assert message(lib).startswith(b"waldo_token_attention_fwd_dt:") and b"waldo_token_attention_fwd" in message(lib)
    assert b"WALDO_DTYPE_F32 is served by waldo_token_attention_fwd" in message(lib)
    assert clips(lib, dtype=F32) == -1
    assert b"WALDO_DTYPE_F32 is served by waldo_token_attention_clips_fwd" in message(lib)


@pytest.mark.parametrize("dtype", [-1, 3, 7, 1 << 20])
def test_an_unknown_dtype_is_refused_before_anything_else(lib, dtype):
    assert dense(lib, q=None, d=48, nk1=0, dtype=dtype) == -1 and b"unknown dtype" in message(lib)
    assert clips(lib, q=None, d=48, max_q=-1, dtype=dtype) == -1 and b"unknown dtype" in message(lib)


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("kw,msg", [
    (dict(d=48), b"bad head dimension D=48 (16, 32 or 64)"),
    (dict(qs=(4096, 4)), b"bad token stride 4"),
    (dict(v1s=(4096, 68)), b"bad token stride 68"),            # a multiple of 4, which the fp32 entry point takes
    (dict(k1s=(4100, 64)), b"bad batch stride 4100"),
    (dict(k2s=(12, 64)), b"bad batch stride 12"),
    (dict(qs=(-4096, 64)), b"negative stride"),
    (dict(q=None), b"null pointer"), (dict(v1=None), b"null pointer"), (dict(out=None), b"null pointer"),
    (dict(k2=None), b"null pointer"),
    (dict(q=24), b"pointer not aligned to 16 bytes"), (dict(v2=8), b"pointer not aligned to 16 bytes"),
    (dict(out=98), b"pointer not aligned to 16 bytes"),
    (dict(nk1=0), b"bad shape"), (dict(nq=-1), b"bad shape"), (dict(h=0), b"bad shape"),
    (dict(scale=float("inf")), b"bad scale"),
    (dict(nk1=2 ** 31 - 60), b"too large"),
])
def test_the_dense_entry_point_refuses(lib, dtype, kw, msg):
    assert dense(lib, dtype=dtype, **kw) == -1, kw
    assert message(lib).startswith(b"waldo_token_attention_fwd_dt: ") and msg in message(lib), (kw, message(lib))


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("kw,msg", [
    (dict(d=48), b"bad head dimension D=48 (16, 32 or 64)"),
    (dict(ks=4), b"bad token stride 4"), (dict(qs=-64), b"negative stride"),
    (dict(max_q=-1), b"bad clip bound max_q_len=-1"), (dict(max_k=-5), b"bad clip bound"),
    (dict(rq=-1), b"bad shape"), (dict(h=0), b"bad shape"),
    (dict(k=None), b"null pointer"), (dict(q_off=None), b"null pointer"), (dict(k_off=None), b"null pointer"),
    (dict(out=None), b"null pointer"),
    (dict(v=40), b"pointer not aligned to 16 bytes"), (dict(out=100), b"pointer not aligned to 16 bytes"),
    (dict(scale=float("nan")), b"bad scale"),
    (dict(rk=2 ** 31), b"too large"),
])
def test_the_clips_entry_point_refuses(lib, dtype, kw, msg):
    assert clips(lib, dtype=dtype, **kw) == -1, kw
    assert message(lib).startswith(b"waldo_token_attention_clips_fwd_dt: ") and msg in message(lib), (kw, message(lib))


def test_the_refusals_come_in_the_fp32_entry_points_order(lib):
    """shape, head dimension, scale, size, strides, (empty: ok), pointers -- as waldo_token_attention_fwd."""
    order = [(dict(nk1=0), b"bad shape"), (dict(d=48), b"bad head dimension"), (dict(scale=float("nan")), b"bad scale"),
             (dict(qs=(4096, 4)), b"bad token stride"), (dict(q=None), b"null pointer"), (dict(out=8), b"not aligned")]
    for i, (_, msg) in enumerate(order):
        kw = {}
        for later, _ in order[i:]:
            kw.update(later)
        assert dense(lib, **kw) == -1 and msg in message(lib), (kw, message(lib))
    # the table pointers of the clips form are not held to 16 bytes; a second segment that is absent is not looked at
    assert dense(lib, nk2=0, k2=None, v2=None, k2s=(3, 3), v2s=(5, 5), b=0) == 0


def test_empty_calls_return_ok_without_a_launch(lib):
    for dtype in (F16, BF16):
        assert dense(lib, b=0, q=None, k1=None, v1=None, k2=None, v2=None, out=None, dtype=dtype) == 0
        assert dense(lib, nq=0, q=None, k1=None, v1=None, k2=None, v2=None, out=None, dtype=dtype) == 0
        assert clips(lib, rq=0, q=None, k=None, v=None, q_off=None, k_off=None, out=None, dtype=dtype) == 0
        assert clips(lib, max_q=0, dtype=dtype) == 0   # no clip has a query


def test_the_route_switch_on_the_cpu():
    import torch
    from waldo_amd import functional as WF
    assert WF.get_token_attention_16bit_route() == "framework"
    with WF.token_attention_16bit_route("kernel"):
        assert WF.get_token_attention_16bit_route() == "kernel"
        with WF.token_attention_16bit_route("framework"):
            assert WF.get_token_attention_16bit_route() == "framework"
        assert WF.get_token_attention_16bit_route() == "kernel"
        # CPU tensors are unchanged under the switch
        q = torch.randn(1, 5, 2, 16, generator=torch.Generator().manual_seed(0)).bfloat16()
        assert WF._token_attention_served_16bit(q, q, q, None, None) is None
        assert torch.equal(WF.token_attention(q, q, q), WF.token_attention_framework(q, q, q))
    assert WF.get_token_attention_16bit_route() == "framework"
    with pytest.raises(ValueError, match="route must be one of"):
        WF.token_attention_16bit_route("mfma")
    with pytest.raises(RuntimeError):
        with WF.token_attention_16bit_route("kernel"):
            raise RuntimeError("x")
    assert WF.get_token_attention_16bit_route() == "framework"
