"""ArenaSnapshot: the exact state of a list of arenas (hk_snapshot / hk_restore, include/hockey.h), and the index
checks of the snapshot / restore / fork calls.

A snapshot holds every word of its arenas that outlives a step -- body rows, packed int words with the episode /
step words that key the device draws, the three BasicOpponent phase rows and all manifold records -- as one opaque
blob.  The blob's layout follows the library's internal enums, so it is valid only for the hk_version() that wrote
it; the snapshot carries that string and the layout numbers, and loading or restoring one that differs raises.
Counters are per context and are not part of a snapshot.
"""
import numpy as np
import torch

from . import _native as N

LAYOUT_FIELDS = ("NFF", "NPW", "phase_rows", "NSOLID", "NMF")


def library_version():
    return N.lib().hk_version().decode()


def library_layout():
    """(NFF, NPW, phase rows, NSOLID, NMF) of the loaded library (hk_snapshot_layout)."""
    import ctypes

    out = (ctypes.c_int32 * 5)()
    N.check(N.lib().hk_snapshot_layout(out), "hk_snapshot_layout")
    return tuple(int(x) for x in out)


def snapshot_bytes(m):
    return int(N.lib().hk_snapshot_bytes(int(m)))


class ArenaSnapshot:
    """blob: uint8 tensor of hk_snapshot_bytes(count) bytes; count: its rows; version: the writer's hk_version();
    layout: (NFF, NPW, phase rows, NSOLID, NMF); keep_mode / vel_ref: the writer's, which a restoring env must
    share (the arenas' words mean the same only then)."""

    def __init__(self, blob, count, version, layout, keep_mode, vel_ref):
        self.blob = blob
        self.count = int(count)
        self.version = str(version)
        self.layout = tuple(int(x) for x in layout)
        self.keep_mode = bool(keep_mode)
        self.vel_ref = bool(vel_ref)

    @property
    def device(self):
        return self.blob.device

    def _with(self, blob):
        return ArenaSnapshot(blob, self.count, self.version, self.layout, self.keep_mode, self.vel_ref)

    def cpu(self):
        return self._with(self.blob.cpu())

    def to(self, device):
        return self._with(self.blob.to(device))

    def check(self, version=None, layout=None, what="snapshot"):
        """Raise unless this snapshot was written by `version` / `layout` (default: the loaded library's)."""
        version = library_version() if version is None else version
        layout = library_layout() if layout is None else tuple(layout)
        if self.version != version:
            raise N.HockeyNativeError(f"{what}: written by {self.version!r}, this library is {version!r}")
        if self.layout != layout:
            theirs = dict(zip(LAYOUT_FIELDS, self.layout))
            ours = dict(zip(LAYOUT_FIELDS, layout))
            raise N.HockeyNativeError(f"{what}: layout {theirs} differs from this library's {ours}")
        if self.blob.numel() != snapshot_bytes(self.count):
            raise N.HockeyNativeError(f"{what}: blob of {self.blob.numel()} bytes, {self.count} arenas take "
                                      f"{snapshot_bytes(self.count)}")

    def save(self, path):
        """An .npz of plain arrays (no pickle)."""
        with open(path, "wb") as f:
            np.savez(f, blob=self.blob.detach().cpu().numpy(), count=np.int64(self.count),
                     version=np.frombuffer(self.version.encode(), np.uint8), layout=np.array(self.layout, np.int32),
                     keep_mode=np.uint8(self.keep_mode), vel_ref=np.uint8(self.vel_ref))

    @classmethod
    def load(cls, path, version=None, layout=None):
        """The snapshot saved at `path`, on the CPU; HockeyNativeError (naming both sides) if its writer's version or
        layout is not `version` / `layout` (default: the loaded library's)."""
        with np.load(path, allow_pickle=False) as z:
            snap = cls(torch.from_numpy(np.ascontiguousarray(z["blob"], np.uint8).copy()), int(z["count"]),
                       z["version"].tobytes().decode(), z["layout"].tolist(), bool(z["keep_mode"]), bool(z["vel_ref"]))
        snap.check(version, layout, what=f"snapshot {path}")
        return snap


def index_tensor(idx, device):
    """An index list as the int64 contiguous tensor the library reads (None stays None: the identity)."""
    if idx is None:
        return None
    t = torch.as_tensor(idx, device=device)
    if t.dtype == torch.bool or t.is_floating_point():
        raise ValueError("arena indices must be integers")
    return t.to(torch.int64).reshape(-1).contiguous()


def check_indices(dst, n_dst, src, n_src, m, same_env=False, what="fork"):
    """The caller's contract of hk_snapshot / hk_restore / hk_copy_arenas (include/hockey.h), checked in torch:
    every index in range, destinations distinct, and -- within one env -- no destination that is also a source.
    dst / src: int64 tensors of m entries, or None for the identity 0..m-1."""
    for name, t, n in (("destination", dst, n_dst), ("source", src, n_src)):
        if t is None:
            if m > n:
                raise ValueError(f"{what}: {m} entries but only {n} {name} arenas")
        else:
            if t.numel() != m:
                raise ValueError(f"{what}: {name} list has {t.numel()} entries, expected {m}")
            if m and bool(((t < 0) | (t >= n)).any()):
                raise ValueError(f"{what}: {name} index out of range [0, {n})")
    if dst is not None and torch.unique(dst).numel() != m:
        raise ValueError(f"{what}: duplicate destination indices")
    if same_env and m:
        d = dst if dst is not None else torch.arange(m, device=src.device if src is not None else None)
        s = src if src is not None else torch.arange(m, device=d.device)
        if bool(torch.isin(d, s).any()):
            raise ValueError(f"{what}: a destination arena is also a source within one env")
