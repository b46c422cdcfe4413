"""ctypes binding of libhockey_render.so (include/hockey_render.h, csrc/hk_render.hip): arenas drawn on the GPU.

``render_states`` draws raw state rows (``hk_get_state`` layout: ``VecHockeyEnv.get_state()[0]`` or a logged
trajectory) as the reference's ``render("rgb_array")`` frames (hockey/hockey_env.py:697-744), by the written
per-pixel coverage law of csrc/hk_render.h, at any size: RGB frames or palette indices (``PALETTE[index] == rgb``).

The call is asynchronous on torch's current stream and, after the first call at a size (which builds that size's
background), graph-capturable.  There is no CPU path: it fails loudly without the library or a GPU tensor.
"""
import ctypes
import os

import torch

from . import _native
from .learner_hip import stream_ptr

LIB_PATH = os.environ.get("HK_RENDER_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib",
                                                           "libhockey_render.so")
RGB, INDEX = 0, 1
STATIC_ONLY = 1
NATIVE_HEIGHT, NATIVE_WIDTH = 480, 600
# colour of every palette index: white, grey, goal orange, black, player 1, player 2
PALETTE = ((255, 255, 255), (204, 204, 204), (239, 203, 138), (0, 0, 0), (235, 98, 53), (93, 158, 199))
EXPORTS = ["hkr_last_error", "hkr_palette", "hkr_render", "hkr_release"]

_FORMATS = {"rgb": RGB, "index": INDEX}
_lib = None


def lib():
    """The loaded render library; raises HockeyNativeError if it is missing (no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise _native.HockeyNativeError(
                f"{LIB_PATH} not found: build it with `make -C hockey-env_amd/csrc render` (hipcc, gfx950)")
        L = ctypes.CDLL(LIB_PATH)
        vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
        L.hkr_last_error.restype = ctypes.c_char_p
        L.hkr_palette.argtypes = [vp]
        L.hkr_palette.restype = None
        L.hkr_render.argtypes = [vp, i64, vp, i64, i32, i32, i32, i32, vp, vp, vp]
        L.hkr_render.restype = ctypes.c_int
        L.hkr_release.restype = None
        _lib = L
    return _lib


def render_states(state, idx=None, height=NATIVE_HEIGHT, width=NATIVE_WIDTH, format="rgb", static_only=False,
                  out=None, bad_index_count=None):
    """Draw raw state rows.  state: [n, 18] float32 device tensor (hk_get_state layout); idx: [m] int32 device tensor
    of the rows to draw, or None for all of them in order.  Returns a uint8 device tensor [m, height, width, 3]
    (format "rgb") or [m, height, width] (format "index"); ``out`` is filled and returned when given.

    An idx entry outside [0, n) leaves its frame untouched and adds one to ``bad_index_count`` (a one-element int64
    device tensor) when that is given."""
    if not isinstance(state, torch.Tensor) or not state.is_cuda:
        raise _native.HockeyNativeError("render_states draws on the GPU: state must be a device tensor")
    if state.dtype != torch.float32 or state.dim() != 2 or state.shape[1] != _native.STATE_DIM:
        raise ValueError("state must be float32 [n, 18]")
    if format not in _FORMATS:
        raise ValueError(f"format must be one of {sorted(_FORMATS)}")
    state = state.contiguous()
    dev = state.device
    if idx is not None:
        idx = torch.as_tensor(idx, dtype=torch.int32, device=dev).contiguous().reshape(-1)
    m = state.shape[0] if idx is None else idx.shape[0]
    shape = (m, int(height), int(width), 3) if format == "rgb" else (m, int(height), int(width))
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif (out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != dev or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous uint8 tensor of shape {shape} on {dev}")
    if bad_index_count is not None and (bad_index_count.dtype != torch.int64 or bad_index_count.device != dev
                                        or bad_index_count.numel() != 1):
        raise ValueError(f"bad_index_count must be a one-element int64 tensor on {dev}")
    if m == 0:
        return out
    with torch.cuda.device(dev):
        rc = lib().hkr_render(_native.ptr(state), state.shape[0], _native.ptr(idx), m, int(height), int(width),
                              _FORMATS[format], STATIC_ONLY if static_only else 0, _native.ptr(out),
                              _native.ptr(bad_index_count), stream_ptr(dev))
    if rc != 0:
        raise _native.HockeyNativeError(f"hkr_render failed ({rc}): {lib().hkr_last_error().decode()}")
    return out
