"""CPU: the argument checks of the batched border-object entry points (``waldo_border_objects_fwd``,
``waldo_points_in_polygon_dev_fwd``) and of their Python wrappers -- rejected on the host, with a message, before any
launch (no GPU is touched), as tests/test_abi.py does for the others."""
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from waldo_amd import _lib, build
    import os
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def border_args(B=1, Tc=1, Tp=1, L=3, H=8, W=8, ptr=None, strides=(1, 1, 1, 1, 1, 1)):
    fb, fc, sb, stc, stp, sl = strides
    return [ptr, fb, fc, ptr, ptr, sb, stc, stp, sl, ptr, ptr, ptr, ptr, B, Tc, Tp, L, H, W, None]


def test_version_is_unchanged(lib):
    assert lib.waldo_version() == 1020


def test_border_objects_rejects_bad_arguments(lib):
    assert lib.waldo_border_objects_fwd(*border_args(L=33)) == -1                       # more than 32 layers
    assert b"L=33" in lib.waldo_last_error_string() and b"bad arguments" in lib.waldo_last_error_string()
    assert lib.waldo_border_objects_fwd(*border_args(L=1)) == -1                        # no object layer
    assert lib.waldo_border_objects_fwd(*border_args(Tc=0)) == -1
    assert lib.waldo_border_objects_fwd(*border_args(Tp=0)) == -1
    assert lib.waldo_border_objects_fwd(*border_args(H=0)) == -1
    assert lib.waldo_border_objects_fwd(*border_args(W=40000)) == -1
    assert lib.waldo_border_objects_fwd(*border_args(B=-1)) == -1
    assert lib.waldo_border_objects_fwd(*border_args(strides=(1, 1, -1, 1, 1, 1))) == -1
    assert b"bad arguments" in lib.waldo_last_error_string()
    assert lib.waldo_border_objects_fwd(*border_args()) == -1                           # NULL tensors, NULL outputs
    assert b"null pointer" in lib.waldo_last_error_string()
    buf = torch.zeros(64, dtype=torch.float64)                                          # host memory: never dereferenced
    args = border_args(ptr=buf.data_ptr())
    args[9] = None                                                                      # a NULL output (`valid`)
    assert lib.waldo_border_objects_fwd(*args) == -1
    assert b"null pointer" in lib.waldo_last_error_string()
    args = border_args(ptr=buf.data_ptr())
    args[12] = None                                                                     # no workspace
    assert lib.waldo_border_objects_fwd(*args) == -1
    assert lib.waldo_border_objects_fwd(*border_args(B=0)) == 0                         # nothing to do
    assert lib.waldo_border_objects_workspace_bytes(0) == 0
    assert lib.waldo_border_objects_workspace_bytes(3) >= 3 * 2 * (31 + 7) * 4


def test_device_polygon_rejects_bad_arguments(lib):
    f = lib.waldo_points_in_polygon_dev_fwd
    assert f(None, None, 8, None, 1, 17, None, 1, 4, None) == -1                        # at most 16 corners
    assert b"bad arguments" in lib.waldo_last_error_string()
    assert f(None, None, -8, None, 1, 4, None, 1, 4, None) == -1                        # negative stride
    assert f(None, None, 8, None, -1, 4, None, 1, 4, None) == -1
    assert f(None, None, 8, None, 1, 4, None, -1, 4, None) == -1
    assert f(None, None, 8, None, 1, 4, None, 1, 4, None) == -1                         # NULL points / output
    assert b"null pointer" in lib.waldo_last_error_string()
    buf = torch.zeros(64, dtype=torch.float64)
    assert f(buf.data_ptr(), buf.data_ptr(), 8, None, 0, 4, None, 1, 4, None) == -1     # a NULL output
    assert b"null pointer" in lib.waldo_last_error_string()
    assert f(buf.data_ptr(), buf.data_ptr(), 8, None, 0, 4, buf.data_ptr(), 70000, 4, None) == -1
    assert b"too many" in lib.waldo_last_error_string()
    assert f(None, None, 8, None, 1, 4, None, 0, 4, None) == 0                          # no polygon, no point: nothing
    assert f(None, None, 8, None, 1, 4, None, 2, 0, None) == 0


def test_wrappers_reject_bad_shapes_and_host_tensors():
    from waldo_amd import functional as WF
    from waldo_amd._lib import WaldoHipError
    with pytest.raises(WaldoHipError):                                                  # no CPU fallback
        WF.border_objects(torch.zeros(1, 2, 8, 8), torch.zeros(8, 8, 2), torch.zeros(1, 1, 1, 3, 8, 8))
    with pytest.raises(WaldoHipError):
        WF.points_in_polygon(torch.zeros(4, 2), torch.zeros(1, 4, 2, dtype=torch.float64))


def test_per_clip_object_ids_are_checked():
    """``Warper.grid_to_obj_flow_from_ref_to_pred`` with a tensor of object ids: (B,) long, nothing else."""
    from waldo_amd.nets import Warper
    grid = [torch.zeros(2, 4, 3, 4, 4, 2), torch.zeros(2, 4, 3, 8, 8, 2), None, None]
    for bad in (torch.zeros(3, dtype=torch.long), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.long)):
        with pytest.raises(ValueError):
            Warper.grid_to_obj_flow_from_ref_to_pred(None, grid, 2, -1, bad)
