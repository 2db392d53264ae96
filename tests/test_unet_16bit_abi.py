"""CPU: the 16-bit form of the plane norm -- the C ABI of waldo_plane_norm_gelu_fwd_dt / _bwd_dt (include/waldo_hip.h
"Plane norm"), ``WF.plane_norm_gelu(..., out_dtype=...)`` on CPU tensors and ``modules.UNet.act_dtype``.  No kernel is
launched and no GPU is touched: every ABI case is refused on the host before a launch; the pointers are small integers
that are never dereferenced."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("waldo_plane_norm_gelu_fwd_dt", "waldo_plane_norm_gelu_bwd_dt")
F32, F16, BF16 = 0, 1, 2   # enum waldo_dtype
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def fwd(lib, x=16, xs=(512, 64), gamma=16, beta=16, eps=1e-5, skip=16, ss=(192, 64), out=16, os_n=704, mean=16, rstd=16,
        ws=None, ws_bytes=0, n=1, c=8, cs=3, h=8, w=8, dtype=BF16):
    """waldo_plane_norm_gelu_fwd_dt with one argument off."""
    return lib.waldo_plane_norm_gelu_fwd_dt(x, *xs, gamma, beta, eps, skip, *ss, out, os_n, mean, rstd, ws, ws_bytes, n, c,
                                            cs, h, w, dtype, None)


def bwd(lib, x=16, xs=(512, 64), gamma=16, beta=16, mean=16, rstd=16, go=16, gs=(704, 64), gx=16, sums=16, ws=None,
        ws_bytes=0, n=1, c=8, h=8, w=8, dtype=BF16):
    return lib.waldo_plane_norm_gelu_bwd_dt(x, *xs, gamma, beta, mean, rstd, go, *gs, gx, sums, ws, ws_bytes, n, c, h, w,
                                            dtype, None)


def test_symbols_are_exported_declared_and_bound(lib):
    from waldo_amd import _lib
    header = open(os.path.join(ROOT, "include", "waldo_hip.h")).read()
    for name, nargs in zip(NAMES, (22, 20)):
        assert hasattr(lib, name), name
        assert f"int {name}(" in header, name
        sig = _lib.SIGNATURES[name]
        assert len(sig) == nargs and sig[-1] is ctypes.c_void_p and sig[-2] is ctypes.c_int
        assert sig[:-2] == _lib.SIGNATURES[name[:-3]][:-1]   # the fp32 prototype, a dtype code before the stream
        proto = header[header.index(f"int {name}("):]
        proto = proto[:proto.index(";")]
        assert proto.count(",") + 1 == nargs and "int dtype, waldo_stream_t stream)" in proto
    assert "unknown dtype" in header[header.index("int waldo_plane_norm_gelu_bwd(") :]
    assert lib.waldo_version() == 1020 == _lib.ABI_VERSION  # additions only: the version is unchanged


def test_the_instances_are_compile_units_of_their_own():
    from waldo_amd import build
    srcs = build.sources()
    for f in ("plane_norm.hip", "plane_norm_bf16.hip", "plane_norm_f16.hip"):
        assert os.path.join(build.CSRC, f) in srcs
    assert os.path.exists(os.path.join(build.CSRC, "plane_norm_kernels.hip.h"))


@pytest.mark.parametrize("dtype", [-1, 3, 7, 1 << 20])
def test_an_unknown_dtype_is_refused_before_any_pointer_is_looked_at(lib, dtype):
    null = dict(x=None, gamma=None, beta=None, mean=None, rstd=None)
    assert fwd(lib, skip=None, out=None, dtype=dtype, **null) == -1
    assert b"unknown dtype" in lib.waldo_last_error_string()
    assert bwd(lib, go=None, gx=None, sums=None, dtype=dtype, **null) == -1
    assert b"unknown dtype" in lib.waldo_last_error_string()
    # (a known one then looks at them)
    assert fwd(lib, skip=None, out=None, dtype=BF16, **null) == -1 and b"null pointer" in lib.waldo_last_error_string()


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("kw,msg", [
    (dict(x=17), b"not aligned"), (dict(out=15), b"not aligned"), (dict(skip=3), b"not aligned"),
    (dict(gamma=17), b"not aligned"), (dict(gamma=18), b"not aligned"), (dict(mean=6), b"not aligned"),   # fp32: to 4
    (dict(n=-1), b"bad shape"), (dict(c=0), b"bad shape"), (dict(cs=-1), b"bad shape"), (dict(h=0), b"bad shape"),
    (dict(w=-3), b"bad shape"),
    (dict(xs=(-512, 64)), b"negative stride"), (dict(os_n=703), b"bad stride"), (dict(eps=float("nan")), b"bad eps"),
    (dict(x=None), b"null pointer"), (dict(skip=None), b"null pointer"),
    (dict(h=32768, w=32769), b"too large"),
    (dict(h=128, w=128, os_n=11 * 128 * 128), b"workspace too small"),   # two chunks per plane and no workspace
    (dict(h=128, w=128, os_n=11 * 128 * 128, ws=16, ws_bytes=8 * 2 * 2 * 4 - 4), b"workspace too small"),
])
def test_fwd_rejects_bad_arguments(lib, dtype, kw, msg):
    assert fwd(lib, dtype=dtype, **kw) == -1, kw
    assert msg in lib.waldo_last_error_string(), (kw, lib.waldo_last_error_string())


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("kw,msg", [
    (dict(x=17), b"not aligned"), (dict(go=5), b"not aligned"), (dict(gx=1), b"not aligned"),
    (dict(sums=18), b"not aligned"), (dict(rstd=6), b"not aligned"),
    (dict(n=-1), b"bad shape"), (dict(c=0), b"bad shape"), (dict(h=0), b"bad shape"),
    (dict(gs=(704, -64)), b"negative stride"), (dict(go=None), b"null pointer"), (dict(sums=None), b"null pointer"),
    (dict(n=2 ** 31), b"too large"),
    (dict(h=128, w=128), b"workspace too small"), (dict(h=128, w=128, ws=16, ws_bytes=100), b"workspace too small"),
])
def test_bwd_rejects_bad_arguments(lib, dtype, kw, msg):
    assert bwd(lib, dtype=dtype, **kw) == -1, kw
    assert msg in lib.waldo_last_error_string(), (kw, lib.waldo_last_error_string())


def test_the_alignment_check_is_per_element_size(lib):
    """A 16-bit buffer on a 2-byte boundary passes the alignment check (refused later, for its workspace: nothing is
    launched); the same address as fp32 does not."""
    big = dict(h=128, w=128, os_n=11 * 128 * 128)
    for dtype in (F16, BF16):
        assert fwd(lib, x=18, skip=6, out=10, dtype=dtype, **big) == -1
        assert b"workspace too small" in lib.waldo_last_error_string()
        assert bwd(lib, x=18, go=6, gx=10, dtype=dtype, h=128, w=128) == -1
        assert b"workspace too small" in lib.waldo_last_error_string()
    assert fwd(lib, x=18, dtype=F32, **big) == -1 and b"not aligned" in lib.waldo_last_error_string()
    assert bwd(lib, gx=10, dtype=F32, h=128, w=128) == -1 and b"not aligned" in lib.waldo_last_error_string()


def test_f32_is_the_fp32_entry_point(lib):
    assert fwd(lib, dtype=F32, os_n=703) == -1
    assert lib.waldo_last_error_string().startswith(b"waldo_plane_norm_gelu_fwd:")
    assert bwd(lib, dtype=F32, c=0) == -1
    assert lib.waldo_last_error_string().startswith(b"waldo_plane_norm_gelu_bwd:")


def test_empty_batch_returns_ok_without_a_launch(lib):
    for dtype in (F32, F16, BF16):
        assert fwd(lib, n=0, x=None, gamma=None, beta=None, skip=None, out=None, mean=None, rstd=None, dtype=dtype) == 0
        assert bwd(lib, n=0, x=None, gamma=None, beta=None, mean=None, rstd=None, go=None, gx=None, sums=None,
                   dtype=dtype) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the op and the module on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def _operands(dtype, seed=0, n=2, c=3, cs=2, h=5, w=7):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, c, h, w, generator=g) * 1.5 + 0.3).to(dtype)
    skip = torch.randn(n, cs, h, w, generator=g).to(dtype)
    return x, 1 + 0.3 * torch.randn(c, generator=g), 0.4 * torch.randn(c, generator=g), skip


@pytest.mark.parametrize("bad", [torch.int8, torch.float32, torch.float64, "bf16"])
def test_any_other_out_dtype_raises(bad):
    from waldo_amd import functional as WF
    x, weight, bias, skip = _operands(torch.float32)
    with pytest.raises(ValueError, match="out_dtype"):
        WF.plane_norm_gelu(x, weight, bias, skip, out_dtype=bad)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_route_is_the_framework_ops_on_fp32_copies_cast(dtype):
    from waldo_amd import functional as WF
    x, weight, bias, skip = _operands(dtype)
    for sk in (skip, None):
        got = WF.plane_norm_gelu(x, weight, bias, sk, out_dtype=dtype)
        want = WF.plane_norm_gelu_framework(x.float(), weight, bias, None if sk is None else sk.float()).to(dtype)
        assert got.dtype == dtype and torch.equal(got, want)
    assert torch.equal(WF.plane_norm_gelu(x, weight, bias, skip, out_dtype=dtype)[:, 3:], skip)   # skip's bits
    # operands of another type are cast to out_dtype FIRST: the statistics are those of the rounded values
    x32, _, _, skip32 = _operands(torch.float32)
    got = WF.plane_norm_gelu(x32, weight, bias, skip32, out_dtype=dtype)
    want = WF.plane_norm_gelu_framework(x32.to(dtype).float(), weight, bias, skip32.to(dtype).float()).to(dtype)
    assert got.dtype == dtype and torch.equal(got, want)
    # out_dtype=None on the CPU: as ever
    assert torch.equal(WF.plane_norm_gelu(x32, weight, bias, skip32), WF.plane_norm_gelu_framework(x32, weight, bias, skip32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_route_carries_the_gradients_in_their_types(dtype):
    from waldo_amd import functional as WF
    x, weight, bias, skip = (t.requires_grad_() for t in _operands(dtype))
    out = WF.plane_norm_gelu(x, weight, bias, skip, out_dtype=dtype)
    out.float().sum().backward()
    assert x.grad.dtype == dtype and skip.grad.dtype == dtype
    assert weight.grad.dtype == torch.float32 and bias.grad.dtype == torch.float32
    assert all(bool(torch.isfinite(t.grad.float()).all()) for t in (x, weight, bias, skip))


def _net(seed=3):
    from waldo_amd.modules import UNet
    torch.manual_seed(seed)
    return UNet(4, 3, 8, "ln2d", 2, 1, False, "bilinear")


def test_act_dtype_accepts_three_values_only():
    net = _net()
    assert net.act_dtype is None
    for ok in (torch.bfloat16, torch.float16, None):
        net.act_dtype = ok
        assert net.act_dtype is ok
    for bad in (torch.float32, torch.int8, "bf16"):
        with pytest.raises(ValueError, match="act_dtype"):
            net.act_dtype = bad
    assert net.act_dtype is None
    assert not any("act_dtype" in k for k in net.state_dict())   # the state dict's names are unchanged


@pytest.mark.parametrize("dtype", DTYPES)
def test_unet_with_act_dtype_returns_that_type_on_the_cpu(dtype):
    net = _net()
    x = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(4))
    net.act_dtype = dtype
    with torch.no_grad():
        out = net(x)
        net.fused = False
        plain = net(x)
    assert out.dtype == dtype and plain.dtype == dtype and out.shape == (1, 3, 8, 8)
    assert bool(torch.isfinite(out.float()).all())


def test_unet_without_act_dtype_is_unchanged_on_the_cpu():
    net = _net()
    x = torch.randn(2, 4, 8, 16, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        fused = net(x)
        net.fused = False
        plain = net(x)
    assert fused.dtype == torch.float32 and torch.equal(fused, plain)


def test_with_unet_and_the_demo_take_the_type():
    from waldo_amd.nets import WIF
    from waldo_amd.tools import demo
    opt = demo.demo_opt(dim=16, aspect_ratio=2.0, num_obj=2, num_lyt=5, ii_embed_dim=16, ii_depth=2)
    assert WIF.with_unet(opt).unet.act_dtype is None
    wif = WIF.with_unet(opt, act_dtype=torch.bfloat16)
    assert wif.unet.act_dtype is torch.bfloat16
    assert sorted(wif.state_dict()) == sorted(WIF.with_unet(opt).state_dict())
    with pytest.raises(ValueError, match="act_dtype"):
        WIF.with_unet(opt, act_dtype=torch.float64)
    with pytest.raises(ValueError, match="unet_dtype"):
        demo.run("nowhere", unet_dtype=torch.bfloat16)   # (needs a checkpoint; refused before the clip is read)
