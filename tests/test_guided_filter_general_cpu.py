"""The general guided-filter entry points (any plane size, one-channel guide, gradient for y) without a GPU: they are exported
and bound, and every argument check answers before anything is launched -- on a machine without a GPU a launch would come back as
FFWM_ERR_LAUNCH (-4), never as the argument codes asserted here."""
import ctypes

import pytest

NEW = ("ffwm_guided_filter_forward_general", "ffwm_guided_filter_backward_general", "ffwm_guided_filter_workspace_bytes")
ERR_ARG, ERR_DTYPE, ERR_SIZE = -1, -2, -3


@pytest.fixture(scope="module")
def hiplib():
    from ffwm_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def ptr():
    buf = (ctypes.c_float * 16)()
    yield ctypes.cast(buf, ctypes.c_void_p)


def test_new_entry_points_are_exported_and_bound(hiplib):
    from ffwm_amd import _lib
    for name in NEW:
        assert name in _lib.EXPORTS
        assert hasattr(hiplib, name)
    assert len(_lib._SIGNATURES["ffwm_guided_filter_forward_general"]) == 13
    assert len(_lib._SIGNATURES["ffwm_guided_filter_backward_general"]) == 14
    assert hiplib.ffwm_guided_filter_workspace_bytes.restype is ctypes.c_int64
    assert hiplib.ffwm_abi_version() == 5          # additive change


def _fwd(lib, x, y, out, saved, ws, px, py, H, W, r, dtype=0):
    return lib.ffwm_guided_filter_forward_general(x, y, out, saved, ws, px, py, H, W, r, 1e-8, dtype, None)


def _bwd(lib, x, y, saved, g, gx, gy, ws, px, py, H, W, r, dtype=0):
    return lib.ffwm_guided_filter_backward_general(x, y, saved, g, gx, gy, ws, px, py, H, W, r, dtype, None)


def test_forward_argument_errors(hiplib, ptr):
    p, err = ptr, hiplib.ffwm_last_error
    for hole in range(4):                                              # x, y, output, saved
        args = [p, p, p, p]
        args[hole] = None
        assert _fwd(hiplib, *args, p, 1, 1, 200, 200, 3) == ERR_ARG and b"NULL tensor pointer" in err()
    assert _fwd(hiplib, p, p, p, p, None, 1, 1, 200, 200, 3) == ERR_ARG and b"workspace" in err()      # a long line needs one
    assert _fwd(hiplib, p, p, p, p, None, 1, 3, 64, 64, 3) == ERR_ARG and b"workspace" in err()        # so does a one-channel guide
    assert _fwd(hiplib, p, p, p, p, p, 1, 1, 200, 200, 3, dtype=7) == ERR_DTYPE and b"dtype" in err()
    assert _fwd(hiplib, p, p, p, p, p, 2, 3, 200, 200, 3) == ERR_ARG and b"planes_x" in err()          # Cx = 2, Cy = 3
    assert _fwd(hiplib, p, p, p, p, p, 0, 3, 200, 200, 3) == ERR_ARG and b"positive" in err()
    assert _fwd(hiplib, p, p, p, p, p, 1, 1, 9, 200, 4) == ERR_ARG and b"H > 2r+1" in err()            # H = 2r+1
    assert _fwd(hiplib, p, p, p, p, p, 1, 1, 200, 9, 4) == ERR_ARG and b"W > 2r+1" in err()
    assert _fwd(hiplib, p, p, p, p, p, 1, 1, 8193, 16, 1) == ERR_SIZE and b"8192" in err() and b"H=8193" in err()
    assert _fwd(hiplib, p, p, p, p, p, 1, 1, 16, 8193, 1) == ERR_SIZE and b"W=8193" in err()
    assert _fwd(hiplib, p, p, p, p, p, 1 << 30, 1 << 30, 512, 512, 1) == ERR_SIZE and b"planes" in err()


def test_backward_argument_errors(hiplib, ptr):
    p, err = ptr, hiplib.ffwm_last_error
    for hole in range(4):                                              # x, y, saved, grad_output
        args = [p, p, p, p]
        args[hole] = None
        assert _bwd(hiplib, *args, p, p, p, 1, 1, 200, 200, 3) == ERR_ARG and b"NULL tensor pointer" in err()
    assert _bwd(hiplib, p, p, p, p, None, None, p, 1, 1, 200, 200, 3) == ERR_ARG and b"grad_x and grad_y" in err()
    assert _bwd(hiplib, p, p, p, p, p, None, None, 1, 1, 200, 200, 3) == ERR_ARG and b"workspace" in err()
    assert _bwd(hiplib, p, p, p, p, p, p, p, 1, 1, 200, 200, 3, dtype=-1) == ERR_DTYPE and b"dtype" in err()
    assert _bwd(hiplib, p, p, p, p, None, p, p, 4, 6, 200, 200, 3) == ERR_ARG and b"planes_x" in err()
    assert _bwd(hiplib, p, p, p, p, p, None, p, 1, 1, 200, 7, 3) == ERR_ARG and b"W > 2r+1" in err()
    assert _bwd(hiplib, p, p, p, p, p, p, p, 1, 1, 8200, 8200, 3) == ERR_SIZE and b"8192" in err()


def test_the_original_entry_points_keep_their_line_limit_and_say_where_to_go(hiplib, ptr):
    p = ptr
    assert hiplib.ffwm_guided_filter_forward(p, p, p, p, 1, 129, 64, 3, 1e-8, 0, None) == ERR_SIZE
    assert b"ffwm_guided_filter_forward_general" in hiplib.ffwm_last_error()


def test_workspace_bytes(hiplib):
    ws = hiplib.ffwm_guided_filter_workspace_bytes
    assert ws(24, 24, 128, 128, 0, 0) == 0                              # the four-launch kernels need none forward
    assert ws(24, 24, 128, 129, 0, 0) == 2 * 48 * 128 * 129 * 4
    assert ws(8, 24, 64, 48, 1, 0) == 2 * 32 * 64 * 48 * 8              # one-channel guide, float64
    assert ws(8, 24, 512, 512, 0, 1) == 4 * 32 * 512 * 512 * 4
    assert ws(24, 24, 128, 128, 0, 1) == 4 * 48 * 128 * 128 * 4         # at least the [2, planes, H, W] of the four-launch backward
    assert ws(2, 3, 64, 64, 0, 1) == ERR_ARG and b"planes_x" in hiplib.ffwm_last_error()
    assert ws(1, 1, 9000, 64, 0, 1) == ERR_SIZE
    assert ws(1, 1, 64, 64, 3, 0) == ERR_DTYPE


def test_python_layer_checks_channels_before_the_library():
    import torch
    from ffwm_amd import external_function as E, ops
    with pytest.raises(AssertionError):
        E.GuidedFilter(3)(torch.rand(1, 2, 16, 16), torch.rand(1, 3, 16, 16))       # the reference's own assertion
    with pytest.raises(NotImplementedError):
        ops.guided_filter_forward(torch.rand(1, 1, 16, 16), torch.rand(1, 3, 16, 16), 3)   # CPU tensors are refused
