"""The wave-composition zoo on the CPU (tests/wave_zoo.py): the fixture's labels are current, the composition table
covers every dispatch arm and event of the velocity families, the dispatch predictor agrees with the kernel source's
host build where one lane can tell, and every scenario runs bit-exact through that host build.

The lane MIXES themselves run only on the GPU (tests/test_gpu_wave_zoo.py): the host build steps one lane at a time.
"""
import numpy as np
import pytest

import wave_zoo as W
from hostcheck import HostVec, velocity_diag
from scene_lockstep import check_run, oracle_run, scene_env


@pytest.fixture(scope="module")
def zoo():
    return W.Zoo()


@pytest.fixture(scope="module")
def batch(zoo):
    return W.Batch(zoo)


def test_fixture_is_plain_runtime_data(zoo):
    import os

    assert os.path.getsize(W.FIXTURE) < 200_000
    d = zoo.d
    n = zoo.n
    assert d["state"].shape == (n, 18) and d["state"].dtype == np.float32
    assert d["aux"].shape == (n, 5) and d["aux"].dtype == np.int32
    assert d["actions"].shape == (n, W.K, 8) and d["actions"].dtype == np.float32
    assert set(d) == {"state", "aux", "actions", *W.LABEL_FIELDS}


def test_labels_are_current(oracle, zoo):
    """(a) Every scenario's labels re-derived with the probe equal the fixture's: a changed oracle (or probe)
    cannot silently stale them.  The replays stay finite and not done through K steps."""
    d = zoo.d
    rec, ok = W.probe_replay(d["state"], d["aux"], np.ascontiguousarray(d["actions"].transpose(1, 0, 2)))
    assert ok.all(), np.nonzero(~ok)[0]
    lab = W.labels_of(rec)
    for f in W.LABEL_FIELDS:
        bad = np.nonzero((lab[f] != d[f]).reshape(zoo.n, -1).any(1))[0]
        assert bad.size == 0, (f, bad[:8], lab[f][bad[:2]], d[f][bad[:2]])


def test_needed_classes_are_in_the_fixture(zoo):
    """Each needed class, several distinct scenarios where the harvest yields them (>= 4 for the common ones)."""
    need4 = ["idle", W.R1, W.R1L, W.R2, W.R2L, W.D1, W.D1L, W.S2A, W.S2AL, W.S2B, W.S2BL, W.TB, W.TBL, W.S3, W.S3L,
             W.SEP(1, 1, "SS"), W.SEP(1, 2, "SS"), W.SEP(2, 1, "SS"), W.SEP(2, 2, "SS"), W.SEPD("SS"),
             W.SEP(1, 1, "SL"), W.SEP(1, 1, "LS"), W.S2SEP("SS"), W.G3, W.G3P2, "toi1", "toi2", "toi3", "toim2"]
    need1 = [W.TBS, W.F4, W.G3P2L, W.SEP(1, 1, "LL")]
    for c in need4:
        assert len(zoo.pool.get((W.J, c), [])) >= 4, c
    for c in need1:
        assert len(zoo.pool.get((W.J, c), [])) >= 1, c
    assert any(c == W.BIG for (_, c) in zoo.pool), "no lane with more than 4 island contacts"
    for c in (W.S3L, W.S2A, W.S2AL, W.R1, W.D1):  # fresh contacts (label step 0: no warm start)
        assert zoo.pool.get((0, c)), c


def test_table_covers_every_arm_and_event(batch):
    """(b) The predictor's output over the composition table is the full arm / event list minus UNREACHABLE; each
    row yields the arms and events it exists for; no row is refused for an island with 24 < cur < 100."""
    assert len(W.UNREACHABLE) <= 4 and set(W.UNREACHABLE) <= set(W.ARMS)
    got, missing_by_row = set(), {}
    for ri, row in enumerate(W.TABLE):
        if not row.predict:
            continue
        p = batch.predict_row(ri)  # raises MidCur on a refused wave
        assert p["arms"] <= set(W.ARMS), (row.name, p["arms"])
        out = p["arms"] | (p["events"] & set(W.EVENTS))
        got |= out
        if not row.expect <= out:
            missing_by_row[row.name] = (sorted(row.expect - out), p["trace"], sorted(p["events"]))
    assert not missing_by_row, missing_by_row
    want = (set(W.ARMS) | set(W.EVENTS)) - set(W.UNREACHABLE)
    assert got == want, {"missing": sorted(want - got), "unexpected": sorted(got - want)}


def test_table_placement_and_sizes(batch):
    assert 60 * 64 <= batch.n <= 90 * 64 and batch.n % 64 == 37
    rows = {r.name: i for i, r in enumerate(W.TABLE)}
    a = np.array(batch.rows)
    full = batch.idx[a == rows["full_wave_one_s2_long"]]
    assert full.size == 64 and (full == full[0]).all()
    one = [c for c in (batch.zoo.cls[i][W.J] for i in batch.idx[a == rows["one_live_lane"]]) if c != "idle"]
    assert one == [W.S2AL]
    toi = batch.toi[a == rows["toi_every_lane"], W.J]
    assert toi.size == 64 and (toi > 0).all()
    assert (batch.toi[a == rows["toi_single_lane"], W.J] > 0).sum() == 1
    t23 = batch.toi[a == rows["toi_2_and_3_events"], W.J]
    assert (t23 == 2).sum() >= 2 and (t23 >= 3).sum() >= 2
    assert batch.large > 0


def test_predictor_vs_host_build(oracle, zoo):
    """(c) Each multi-contact scenario alone through the kernel source's host build: for a one-lane wave the
    predictor and the host build's coverage counters agree on zero / non-zero -- island retired beside a running
    one, live contacts swapped into slots 0/1, S3 family entered, S2 / aliased chunk run.  The prediction is read
    over all K steps here (no checkpoint restriction: one lane's dispatch follows from its own cur values), and a
    TOI mini-island of two contacts (two static contacts on one body: a TB lane) runs the aliased chunk."""
    velocity_diag()
    d = zoo.d
    bad = []
    ran = 0
    for i in range(zoo.n):
        if d["ncont"][i].max() < 2 and d["toi_n2"][i].max() == 0:
            continue
        want = np.zeros(4, bool)
        for t in range(W.K):
            p = W.predict([zoo.lane(i, t)], strict=False)
            ev = p["events"]
            want |= np.array(["retire" in ev, "swap" in ev, "s3_entry" in ev, "s2_chunk" in ev])
            want[3] |= d["toi_n2"][i, t] > 0
        env = HostVec(1)
        env.set_state(d["state"][i:i + 1], d["aux"][i:i + 1])
        for t in range(W.K):
            env.step(d["actions"][i:i + 1, t], with_agent_two=True)
        env.close()
        got = velocity_diag() > 0
        ran += 1
        if not np.array_equal(got, want):
            bad.append((i, zoo.cls[i], got.tolist(), want.tolist()))
    assert ran > 100
    assert not bad, bad[:6]


def test_composed_batch_host_build_vs_oracle(oracle, batch):
    """(d) The composed batch through the host build is bit-exact to the oracle.  Lane by lane: this checks the
    scenarios (and that the GPU test's reference is the kernel source's own answer), not the mixes."""
    want = oracle_run(oracle, batch.state, batch.aux, batch.actions)
    assert len(want["steps"]) == W.K and not any(s["done"].any() for s in want["steps"])
    check_run(scene_env(HostVec, batch.state, batch.aux), batch.actions, "hk_step", want, "host build",
              describe=batch.describe, toi=batch.toi, large=batch.large)
