"""The host build's exact arena copies (hkh_snapshot / hkh_restore / hkh_copy_arenas: hk_arena_copy.h's copy_arena
looped on the CPU) behind the product's ArenaSnapshot, for tests/test_arena_copy.py.  TEST INFRASTRUCTURE ONLY.

A snapshot taken here is a hockey_amd.snapshot.ArenaSnapshot whose blob is a CPU tensor: the blob layout is the
library's (one header), which bind() asserts.
"""
import ctypes

import numpy as np
import torch

import hostcheck as H
from hockey_amd import _native as N
from hockey_amd import snapshot as S

_bound = False


def bind():
    global _bound
    L = H.lib()
    if not _bound:
        vp, i64 = ctypes.c_void_p, ctypes.c_int64
        L.hkh_snapshot_bytes.restype = i64
        L.hkh_snapshot_bytes.argtypes = [i64]
        L.hkh_snapshot_layout.restype = None
        L.hkh_snapshot_layout.argtypes = [vp]
        L.hkh_snapshot.restype = ctypes.c_int
        L.hkh_snapshot.argtypes = [vp, vp, i64, vp]
        L.hkh_restore.restype = ctypes.c_int
        L.hkh_restore.argtypes = [vp, vp, i64, vp, i64, vp]
        L.hkh_copy_arenas.restype = ctypes.c_int
        L.hkh_copy_arenas.argtypes = [vp, vp, vp, vp, i64]
        lay = np.zeros(5, np.int32)
        L.hkh_snapshot_layout(lay.ctypes.data)
        assert tuple(int(x) for x in lay) == S.library_layout(), "host build and library share one layout"
        for m in (0, 1, 37, 64, 101):
            assert L.hkh_snapshot_bytes(m) == S.snapshot_bytes(m)
        _bound = True
    return L


def _idx(a):
    return None if a is None else np.ascontiguousarray(a, np.int64)


def _p(a):
    return None if a is None else a.ctypes.data


def snapshot(hv, idx=None):
    """ArenaSnapshot (CPU blob) of arenas idx (all when None) of the HostVec hv."""
    L = bind()
    ix = _idx(idx)
    m = hv.n if ix is None else ix.size
    blob = torch.zeros(S.snapshot_bytes(m), dtype=torch.uint8)
    assert L.hkh_snapshot(hv.h, _p(ix), m, blob.data_ptr()) == 0
    return S.ArenaSnapshot(blob, m, S.library_version(), S.library_layout(), bool(hv._cfg[0]), bool(hv._cfg[3]))


def restore(hv, snap, idx=None, rows=None):
    L = bind()
    snap.check(what="restore")
    ix, rw = _idx(idx), _idx(rows)
    m = ix.size if ix is not None else (rw.size if rw is not None else snap.count)
    assert L.hkh_restore(hv.h, _p(ix), m, snap.blob.data_ptr(), snap.count, _p(rw)) == 0


def copy(dst, dst_idx, src, src_idx):
    """hkh_copy_arenas; returns its status (0, or -1 for contexts that differ in keep_mode / vel_ref)."""
    L = bind()
    d, s = _idx(dst_idx), _idx(src_idx)
    m = s.size if s is not None else (d.size if d is not None else min(dst.n, src.n))
    return L.hkh_copy_arenas(dst.h, _p(d), src.h, _p(s), m)


def bad_index_count(hv):
    return int(hv.counters()[N.CNT_BAD_INDEX])
