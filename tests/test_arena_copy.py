"""Exact arena snapshots, restore and fork on the CPU: the host build of hk_arena_copy.h (the copy kernel's source,
looped per entry) against the oracle, which is never snapshotted -- it runs every history uninterrupted and is the
independent side.  Every comparison is at tolerance zero (bit patterns).
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import arena_copy_host as AC  # noqa: E402
from arena_copy_cases import N_ARENAS, fork_follows_the_oracle, interrupted  # noqa: E402
from arena_copy_cases import scen, want  # noqa: E402,F401  (module-scoped fixtures: the scenarios, the oracle's run)
import hostcheck as H  # noqa: E402
from hockey_amd import _native as N  # noqa: E402
from hockey_amd import snapshot as S  # noqa: E402
from scene_lockstep import STEP_FIELDS, scene_env  # noqa: E402


def _host(scen, n=N_ARENAS):  # noqa: F811
    return scene_env(H.HostVec, scen["state"][:n], scen["aux"][:n])


def _step(hv, scen, t):  # noqa: F811
    return vars(hv.step(scen["actions"][t][:hv.n], with_agent_two=True))


def test_resume_from_snapshot_equals_uninterrupted_oracle(scen, want):  # noqa: F811
    """(1) snapshot -> every arena reset and stepped -> restore -> the oracle's uninterrupted trajectory."""
    ok = interrupted(_host(scen), scen, want, "hk_step", AC.snapshot, AC.restore)
    assert ok.all(), "arenas %s left the oracle's trajectory after restore" % np.nonzero(~ok)[0].tolist()


def test_resume_from_get_state_is_not_exact(scen, want):  # noqa: F811
    """(2) the power of (1): the same interruption with get_state / set_state (the reference's 18 + 5 words) does
    NOT resume these scenarios exactly, so (1) passes because of what only the snapshot carries."""
    ok = interrupted(_host(scen), scen, want, "hk_step", lambda hv: hv.get_state(), lambda hv, s: hv.set_state(*s))
    assert not ok.all(), "set_state alone resumed every arena exactly: the scenarios show nothing"


# ------------------------------------------------------------------------------------------------ fork
def _fork(hv, src, dst):
    assert AC.copy(hv, dst, hv, src) == 0


def test_fork_to_other_indices_follows_the_oracle(oracle):
    """(3) arena_copy_cases.fork_follows_the_oracle with hkh_copy_arenas as the fork."""
    fork_follows_the_oracle(oracle, H.HostVec(128), "hk_step", _fork)


# ------------------------------------------------------------------------------------------------ round trips, errors
@pytest.fixture(scope="module")
def played(scen):
    """A context two steps into the scenarios (contacts stored), read-only for the tests below."""
    hv = _host(scen)
    for t in range(2):
        _step(hv, scen, t)
    yield hv
    hv.close()


@pytest.mark.parametrize("m", [1, 37, 64, 101])
def test_snapshot_save_load_restore_round_trip(played, scen, tmp_path, m):
    """(4) snapshot -> save -> load -> restore over a list of m entries is exact: the restored arenas' snapshot is
    byte-identical, and they step like their sources."""
    idx = np.random.default_rng(m).permutation(N_ARENAS)[:m]
    snap = AC.snapshot(played, idx)
    assert snap.blob.numel() == S.snapshot_bytes(m) and snap.count == m
    path = os.path.join(tmp_path, "arenas.npz")
    snap.save(path)
    back = S.ArenaSnapshot.load(path)
    assert torch.equal(back.blob, snap.blob) and (back.count, back.version, back.layout, back.keep_mode,
                                                  back.vel_ref) == (m, snap.version, snap.layout, True, False)
    with np.load(path, allow_pickle=False) as z:  # plain arrays: readable without pickle
        assert set(z.files) == {"blob", "count", "version", "layout", "keep_mode", "vel_ref"}
    other = H.HostVec(N_ARENAS, policies=("external", "external"), auto_reset=False)
    AC.restore(other, back, idx)
    assert torch.equal(AC.snapshot(other, idx).blob, snap.blob)
    a = scen["actions"][2]
    g0 = vars(_step_twin(played, a))
    g1 = vars(other.step(a, with_agent_two=True))
    for f in STEP_FIELDS:
        assert (g0[f][idx].reshape(m, -1).view(np.uint8) == g1[f][idx].reshape(m, -1).view(np.uint8)).all(), f
    assert AC.bad_index_count(other) == 0
    other.close()


def _step_twin(hv, actions):
    """One step of a full copy of hv (hv itself stays as it is)."""
    twin = H.HostVec(hv.n, policies=("external", "external"), auto_reset=False)
    assert AC.copy(twin, None, hv, None) == 0
    out = twin.step(actions, with_agent_two=True)
    twin.close()
    return out


def test_restore_rows_replicates_one_row(played):
    snap = AC.snapshot(played, [10, 20, 30])
    other = H.HostVec(16, policies=("external", "external"), auto_reset=False)
    AC.restore(other, snap, idx=np.arange(4, 13), rows=np.full(9, 1))
    one = AC.snapshot(played, [20]).blob
    for a in range(4, 13):
        assert torch.equal(AC.snapshot(other, [a]).blob, one), a
    fresh = H.HostVec(16, policies=("external", "external"), auto_reset=False)
    rest = [a for a in range(16) if not 4 <= a < 13]
    assert torch.equal(AC.snapshot(other, rest).blob, AC.snapshot(fresh, rest).blob)  # nothing else was written
    other.close()
    fresh.close()


def test_out_of_range_entries_copy_nothing_and_are_counted(played):
    other = H.HostVec(16, policies=("external", "external"), auto_reset=False)
    before = AC.snapshot(other)
    # entries 1 and 3 have a bad destination, entry 4 a bad source
    assert AC.copy(other, [0, -1, 2, 16, 5], played, [7, 8, 9, 10, N_ARENAS]) == 0
    assert AC.bad_index_count(other) == 3 and AC.bad_index_count(played) == 0
    assert torch.equal(AC.snapshot(other, [0, 2]).blob, AC.snapshot(played, [7, 9]).blob)
    rest = [a for a in range(16) if a not in (0, 2)]
    probe = H.HostVec(16, policies=("external", "external"), auto_reset=False)
    AC.restore(probe, before)  # `other` as it was
    assert torch.equal(AC.snapshot(other, rest).blob, AC.snapshot(probe, rest).blob)
    snap = AC.snapshot(played, [1, 2])
    AC.restore(other, snap, idx=[3, 4, 5], rows=[0, 2, -1])  # rows 2 and -1 do not exist
    assert AC.bad_index_count(other) == 5
    assert torch.equal(AC.snapshot(other, [3]).blob, AC.snapshot(played, [1]).blob)
    assert torch.equal(AC.snapshot(other, [4, 5]).blob, AC.snapshot(probe, [4, 5]).blob)
    other.close()
    probe.close()


def test_version_or_layout_mismatch_raises(played, tmp_path):
    snap = AC.snapshot(played, [0, 1])
    path = os.path.join(tmp_path, "s.npz")
    old = S.ArenaSnapshot(snap.blob, 2, "hockey-mi355x 0.1 (other)", snap.layout, True, False)
    old.save(path)
    with pytest.raises(N.HockeyNativeError) as e:
        S.ArenaSnapshot.load(path)
    assert "hockey-mi355x 0.1 (other)" in str(e.value) and S.library_version() in str(e.value)
    lay = list(snap.layout)
    lay[3] += 1
    S.ArenaSnapshot(snap.blob, 2, snap.version, lay, True, False).save(path)
    with pytest.raises(N.HockeyNativeError) as e:
        S.ArenaSnapshot.load(path)
    assert str(lay[3]) in str(e.value) and str(snap.layout[3]) in str(e.value)
    with pytest.raises(N.HockeyNativeError):  # restore checks too, not only load
        AC.restore(played, old)
    S.ArenaSnapshot(snap.blob[:-16], 2, snap.version, snap.layout, True, False).save(path)
    with pytest.raises(N.HockeyNativeError):
        S.ArenaSnapshot.load(path)
    other = H.HostVec(4, keep_mode=False, policies=("external", "external"))
    assert AC.copy(other, [0], played, [0]) == -1  # keep_mode differs
    other.close()


def test_python_index_checks():
    """Duplicate destinations, an overlap within one env and an index out of range raise before any call."""
    t = lambda *a: torch.tensor(a, dtype=torch.int64)  # noqa: E731
    S.check_indices(t(4, 5, 6), 8, t(0, 0, 1), 8, 3, same_env=True)
    S.check_indices(None, 8, t(0, 0, 1), 4, 3)
    with pytest.raises(ValueError, match="duplicate"):
        S.check_indices(t(4, 5, 4), 8, t(0, 1, 2), 8, 3)
    with pytest.raises(ValueError, match="also a source"):
        S.check_indices(t(4, 5, 1), 8, t(0, 1, 2), 8, 3, same_env=True)
    S.check_indices(t(4, 5, 1), 8, t(0, 1, 2), 8, 3, same_env=False)  # two envs: no overlap to speak of
    with pytest.raises(ValueError, match="also a source"):
        S.check_indices(None, 8, t(5, 1, 7), 8, 3, same_env=True)  # identity destinations 0..2 hold source 1
    with pytest.raises(ValueError, match="out of range"):
        S.check_indices(t(4, 8), 8, t(0, 1), 8, 2)
    with pytest.raises(ValueError, match="out of range"):
        S.check_indices(t(4, 5), 8, t(0, -1), 8, 2)
    with pytest.raises(ValueError, match="entries"):
        S.check_indices(t(4, 5), 8, t(0,), 8, 2)
    with pytest.raises(ValueError):
        S.index_tensor([0.5, 1.0], "cpu")
