"""CPU: the C ABI of the token attention (include/waldo_hip.h "Token attention": waldo_token_attention_fwd and the
limits query) and the CPU route of ``WF.token_attention``.  No kernel is launched and no GPU is touched: every case is
refused, or returns, on the host before a launch; the pointers are small integers that are never dereferenced."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("waldo_token_attention_fwd", "waldo_token_attention_limits")


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def fwd(lib, q=64, qs=(3072, 384), k1=128, k1s=(3072, 384), v1=192, v1s=(3072, 384), k2=256, k2s=(2560, 256), v2=320,
        v2s=(2560, 256), out=512, scale=0.125, b=2, h=2, d=64, nq=8, nk1=8, nk2=10):
    """waldo_token_attention_fwd with one argument off."""
    return lib.waldo_token_attention_fwd(q, *qs, k1, *k1s, v1, *v1s, k2, *k2s, v2, *v2s, out, scale, b, h, d, nq, nk1,
                                         nk2, None)


def test_symbol_is_exported_and_matches_the_header(lib):
    from waldo_amd import _lib
    for name in NAMES:
        assert hasattr(lib, name), name
    sig = _lib.SIGNATURES["waldo_token_attention_fwd"]
    assert sig[-1] is ctypes.c_void_p and "waldo_token_attention_limits" in _lib.PLAIN
    header = open(os.path.join(ROOT, "include", "waldo_hip.h")).read()
    sec = header[header.index(" * Token attention:"):]
    for needle in NAMES + ("NO SCORE MATRIX", "NO ATOMICS", "FOLLOWED BY", "never copied", "16, 32 or 64"):
        assert needle in sec, needle
    # the prototype's arguments, one to one: pointers, 64-bit strides, a float, the shape, the stream
    proto = sec[sec.index("int waldo_token_attention_fwd("):]
    proto = proto[proto.index("(") + 1:proto.index(");")]
    kinds = []
    for arg in proto.split(","):
        arg = " ".join(arg.split())
        kinds.append(ctypes.c_void_p if "*" in arg or arg.startswith("waldo_stream_t") else
                     ctypes.c_int64 if arg.startswith("int64_t") else ctypes.c_float if arg.startswith("float") else
                     ctypes.c_int)
    assert kinds == sig
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION  # the symbols are additions: the version is unchanged


def test_the_kernel_lives_in_a_file_of_its_own():
    from waldo_amd import build
    assert os.path.join(build.CSRC, "token_attention.hip") in build.sources()


def test_limits(lib):
    from waldo_amd import functional as WF
    lim = WF.token_attention_limits()
    assert set(lim) == {"q_tile", "k_tile", "head_dims"}
    assert lim["head_dims"] == (16, 32, 64)
    assert lim["q_tile"] >= 16 and lim["q_tile"] % 16 == 0 and lim["k_tile"] >= 16 and lim["k_tile"] % 16 == 0
    buf = (ctypes.c_int * 1)()
    assert lib.waldo_token_attention_limits(buf, 1) == 5 and buf[0] == lim["q_tile"]  # (writes no more than asked)
    assert lib.waldo_token_attention_limits(None, 0) == 5


@pytest.mark.parametrize("kw,msg", [
    (dict(q=None), b"null pointer"), (dict(k1=None), b"null pointer"), (dict(v1=None), b"null pointer"),
    (dict(out=None), b"null pointer"), (dict(k2=None), b"null pointer"), (dict(v2=None), b"null pointer"),
    (dict(d=48), b"bad head dimension"), (dict(d=0), b"bad head dimension"), (dict(d=128), b"bad head dimension"),
    (dict(d=8), b"bad head dimension"),
    (dict(nk1=0), b"bad shape"), (dict(nk1=-1), b"bad shape"), (dict(nk2=-1), b"bad shape"), (dict(nq=-1), b"bad shape"),
    (dict(b=-1), b"bad shape"), (dict(h=0), b"bad shape"),
    # a view with a non-unit inner stride: its rows are not D consecutive floats, and the prototype has no argument
    # for it -- what such a caller can pass is a token stride that is no whole number of 16-byte pieces, refused with
    # a message of its own; a batch stride off the boundaries is another refusal
    (dict(qs=(3072, 385)), b"bad token stride 385"), (dict(qs=(3072, 385)), b"non-unit inner stride"),
    (dict(v2s=(2560, 258)), b"bad token stride 258"),
    (dict(k1s=(3073, 384)), b"bad batch stride 3073"),
    (dict(qs=(-3072, 384)), b"negative stride"), (dict(k2s=(2560, -256)), b"negative stride"),
    (dict(q=68), b"not aligned"), (dict(v1=8), b"not aligned"), (dict(out=36), b"not aligned"), (dict(k2=4), b"not aligned"),
    (dict(scale=float("nan")), b"bad scale"), (dict(scale=float("inf")), b"bad scale"),
    (dict(b=2 ** 31), b"too large"), (dict(nk1=2 ** 31 - 1, nk2=2 ** 31 - 1), b"too large"),
    (dict(b=2 ** 24, h=8, nq=2 ** 12), b"too large"),
])
def test_fwd_rejects_bad_arguments(lib, kw, msg):
    assert fwd(lib, **kw) == -1, kw
    err = lib.waldo_last_error_string()
    assert err.startswith(b"waldo_token_attention_fwd:") and msg in err, (kw, err)


def test_the_two_stride_refusals_are_told_apart(lib):
    assert fwd(lib, k1s=(3073, 384)) == -1 and b"inner stride" not in lib.waldo_last_error_string()
    assert fwd(lib, qs=(3072, 386)) == -1 and b"batch stride" not in lib.waldo_last_error_string()


def test_empty_calls_return_ok_without_a_launch(lib):
    null = dict(q=None, k1=None, v1=None, k2=None, v2=None, out=None)
    assert fwd(lib, b=0, **null) == 0
    assert fwd(lib, nq=0, **null) == 0
    # a single segment: the second one's pointers and strides are not looked at (a bad D still is)
    assert fwd(lib, b=0, nk2=0, k2s=(1, -3), **null) == 0
    assert fwd(lib, nk2=0, k2=None, v2=None, q=None) == -1 and b"null pointer" in lib.waldo_last_error_string()
    assert fwd(lib, b=0, d=48, **null) == -1


def _spelled_out(q, k, v, k2=None, v2=None, scale=None):
    """The reference's lines, on (B, H, N, D) permutes of the views."""
    b, nq, h, d = q.shape
    scale = d ** -0.5 if scale is None else scale
    qh, kh, vh = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    attn = (qh @ kh.transpose(-2, -1)) * scale
    if k2 is not None:
        attn = torch.cat([attn, (qh @ k2.permute(0, 2, 1, 3).transpose(-2, -1)) * scale], dim=-1)
        vh = torch.cat([vh, v2.permute(0, 2, 1, 3)], dim=2)
    return (attn.softmax(dim=-1) @ vh).transpose(1, 2).reshape(b, nq, h * d)


def test_cpu_tensors_take_the_spelled_out_ops():
    from waldo_amd import functional as WF
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(2, 7, 3, 2, 16, generator=g)
    kv = torch.randn(2, 5, 2, 2, 16, generator=g)
    q, k, v = qkv.unbind(2)
    k2, v2 = kv.unbind(2)
    assert torch.equal(WF.token_attention(q, k, v), _spelled_out(q, k, v))
    assert torch.equal(WF.token_attention(q, k, v, k2, v2), _spelled_out(q, k, v, k2, v2))
    assert torch.equal(WF.token_attention(q, k, v, k2, v2, scale=0.7), _spelled_out(q, k, v, k2, v2, 0.7))
    assert torch.equal(WF.token_attention_framework(q, k, v, k2, v2), _spelled_out(q, k, v, k2, v2))
    # D = 48 and a non-unit inner stride are framework shapes everywhere
    w = torch.randn(1, 3, 2, 96, generator=g)
    assert torch.equal(WF.token_attention(w[..., :48], w[..., 48:], w[..., :48]),
                       _spelled_out(w[..., :48], w[..., 48:], w[..., :48]))
    assert torch.equal(WF.token_attention(w[..., ::2], w[..., 1::2], w[..., ::2]),
                       _spelled_out(w[..., ::2], w[..., 1::2], w[..., ::2]))
    # differentiable like any framework expression
    ql = q.clone().requires_grad_()
    WF.token_attention(ql, k, v, k2, v2).square().sum().backward()
    assert ql.grad is not None and torch.isfinite(ql.grad).all()


def test_python_surface_checks_shapes_before_anything_else():
    from waldo_amd import functional as WF
    q, k = torch.zeros(2, 3, 2, 16), torch.zeros(2, 5, 2, 16)
    with pytest.raises(ValueError, match="B, Nq, H, D"):
        WF.token_attention(q[0], k, k)
    with pytest.raises(ValueError, match="k and v must be"):
        WF.token_attention(q, k, k[:, :4])
    with pytest.raises(ValueError, match="k and v must be"):
        WF.token_attention(q, k[:, :0], k[:, :0])
    with pytest.raises(ValueError, match="k and v must be"):
        WF.token_attention(q, torch.zeros(2, 5, 4, 8), torch.zeros(2, 5, 4, 8))
    with pytest.raises(ValueError, match="come together"):
        WF.token_attention(q, k, k, k2=k)
    with pytest.raises(ValueError, match="k2 and v2 must be"):
        WF.token_attention(q, k, k, k2=k[:1], v2=k[:1])
