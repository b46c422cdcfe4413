"""hkl_eval_begin / hkl_eval_step / hkl_eval_fold (include/hockey_eval.h, csrc/hkl_eval.h) on the GPU against the laws in
numpy (hockey_amd.evaluator.eval_*_law, the Evaluator's torch backend), every word compared as integers, and the
Evaluator end to end.  Outputs start as sentinels, so a word that should not have been written, or was not, shows.

The shapes are the smallest that can go wrong: rows_per_cell 1, 5, 64, 65, 257, 513 (cells inside one wave, one
workgroup, cells that straddle workgroups, more than two rows per lane of the fold) with 1, 3 and 130 cells (more than
HKL_GROUP_MAX), and one cell of 4 097 rows.

This file captures no graph and takes no stream from torch's pool (tests/test_gpu_facade.py's blocked-stream test runs
after it and depends on the streams handed out before): the training test is in tests/test_gpu_population_eval.py.
"""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hockey_amd import evaluator as E  # noqa: E402
from hockey_amd import learner_hip as LH  # noqa: E402

DEV = "cuda:0"
SHAPES = [(C, n) for C in (1, 3, 130) for n in (1, 5, 64, 65, 257, 513)] + [(1, 4097)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Rig:
    """The struct's arrays as device tensors full of sentinels, and the law's state beside them."""

    SENTINEL = {"step": -9, "live": 7, "ret": float("nan"), "length": -9, "winner": -5, "count": -9,
                "opp_inc": float("nan"), "outcomes": -9, "length_sum": -9, "return_sum": float("nan")}

    def __init__(self, C, n, seed, info_ld=4, with_inc=True):
        rng = self.rng = np.random.default_rng(seed)
        self.C, self.n, self.N, self.info_ld, self.with_inc = C, n, C * n, info_ld, with_inc
        NN = self.N
        self.seeds = [int(x) for x in rng.integers(0, 2 ** 63, C)]
        self.seeds[0] = 2 ** 64 - 5
        full = lambda sh, dt, k: torch.full(sh, self.SENTINEL[k], dtype=dt, device=DEV)  # noqa: E731
        t = self.t = {"seeds": dev(np.array(self.seeds, np.uint64).view(np.int64)),
                      "step": full((1,), torch.int64, "step"), "live": full((NN,), torch.uint8, "live"),
                      "ret": full((NN,), torch.float64, "ret"), "length": full((NN,), torch.int32, "length"),
                      "winner": full((NN,), torch.int8, "winner"), "count": full((C,), torch.int32, "count"),
                      "opp_inc": full((NN, 2), torch.float64, "opp_inc"),
                      "outcomes": full((C, 4), torch.int64, "outcomes"),
                      "length_sum": full((C,), torch.int64, "length_sum"),
                      "return_sum": full((C,), torch.float64, "return_sum")}
        io = self.io = LH.EvalIO()
        io.n_rows, io.rows_per_cell, io.info_ld = NN, n, info_ld
        for k, v in t.items():
            if k != "opp_inc" or with_inc:
                setattr(io, k, v.data_ptr())
        self.state = None
        self.keep = None
        self.folded = False

    def call(self, name):
        LH.check(getattr(LH.lib(), name)(ctypes.byref(self.io), LH.stream_ptr(torch.device(DEV))), name)

    def check_state(self, what):
        torch.cuda.synchronize()
        t, st = self.t, self.state
        for k in ("live", "length", "winner", "count", "step"):
            assert np.array_equal(host(t[k]), st[k]), (what, k)
        assert np.array_equal(bits(host(t["ret"])), bits(st["ret"])), what
        if self.with_inc:
            assert np.array_equal(bits(host(t["opp_inc"])), bits(st["opp_inc"])), what
        else:
            assert np.isnan(host(t["opp_inc"])).all(), what

    def begin(self):
        self.call("hkl_eval_begin")
        self.state = E.eval_begin_law(self.seeds, self.n)
        self.check_state("begin")
        if not self.folded:  # the fold's outputs are the fold's alone
            for k in ("outcomes", "length_sum"):
                assert (host(self.t[k]) == -9).all()

    def inputs(self, p_done=0.3):
        rng, NN = self.rng, self.N
        reward = rng.standard_normal(NN).astype(np.float32)
        done = (rng.random(NN) < p_done).astype(np.uint8)
        info = rng.standard_normal((NN, self.info_ld)).astype(np.float32)
        info[:, 0] = rng.integers(-1, 2, NN)
        return reward, done, info

    def step(self, reward, done, info, what="step", check=True):
        self.keep = [dev(x) for x in (reward, done, info)]
        self.io.reward, self.io.done, self.io.info = (x.data_ptr() for x in self.keep)
        self.call("hkl_eval_step")
        self.state = E.eval_step_law(self.seeds, self.n, self.state, reward, done, info[:, 0])
        if check:
            self.check_state(what)

    def fold(self, what="fold", check=True):
        self.call("hkl_eval_fold")
        self.folded = True
        torch.cuda.synchronize()
        st = self.state
        want = E.eval_fold_law(self.n, st["live"], st["ret"], st["length"], st["winner"])
        got = tuple(host(self.t[k]) for k in ("outcomes", "length_sum", "return_sum"))
        if check:
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
            assert np.array_equal(bits(got[2]), bits(want[2])), what
        return got


@pytest.mark.parametrize("C,n", SHAPES)
def test_begin_step_and_fold_equal_the_laws_word_for_word(C, n):
    """begin, then three step calls with about 30 % of the rows finishing per call and a fold after each: live, length,
    winner, count, step, the bits of ret and opp_inc and the fold's three outputs (return_sum as bits) equal the laws."""
    rig = Rig(C, n, seed=1000 * C + n)
    rig.begin()
    rig.fold("fold after begin")  # nobody finished: zeros, and the live count
    assert (host(rig.t["outcomes"])[:, 3] == n).all() and not host(rig.t["return_sum"]).any()
    for c in range(3):
        rig.step(*rig.inputs(), what=f"step {c}")
        rig.fold(f"fold {c}")
    if C * n >= 64:
        assert 0 < rig.state["count"].sum() < C * n  # some finished, some still play
    assert rig.state["count"].sum() == rig.state["live"].sum()


def test_a_finished_batch_and_a_second_begin():
    """Every row finishes in one call (count reaches zero in every cell, live rows of the fold are zero); a second
    begin on the used buffers equals a fresh one."""
    rig = Rig(3, 257, seed=5)
    rig.begin()
    reward, done, info = rig.inputs()
    rig.step(reward, np.ones_like(done), info)
    assert not host(rig.t["count"]).any()
    out = rig.fold()
    assert not out[0][:, 3].any() and (out[0][:, :3].sum(1) == 257).all() and (out[1] == 257).all()
    rig.step(*rig.inputs())  # a step with nobody live changes nothing but step and opp_inc
    assert (host(rig.t["length"]) == 1).all()
    rig.begin()
    rig.step(*rig.inputs())


@pytest.mark.parametrize("info_ld,with_inc", [(1, True), (4, False), (7, True)])
def test_info_stride_and_a_null_opp_inc(info_ld, with_inc):
    """info rows of 1, 4 and 7 floats (column 0 is read); opp_inc NULL: nothing of it is written."""
    rig = Rig(3, 65, seed=info_ld, info_ld=info_ld, with_inc=with_inc)
    rig.begin()
    for c in range(2):
        rig.step(*rig.inputs(), what=f"step {c}")
    rig.fold()


@pytest.mark.parametrize("bad_info", [math.inf, -math.inf, math.nan])
def test_a_non_finite_row_reaches_only_itself_and_its_cells_return_sum(bad_info):
    """One row with a NaN reward and a +-Inf / NaN winner, finishing in that call: against the clean run only its ret
    (NaN), its winner (the sign; 0 for a NaN) and its cell's return_sum (NaN) differ -- no count, no other cell."""
    C, n, r0 = 3, 65, 65 + 17
    clean, dirty = Rig(C, n, seed=9), Rig(C, n, seed=9)
    want_w = 0 if math.isnan(bad_info) else int(math.copysign(1, bad_info))
    outs = []
    for rig, bad in ((clean, False), (dirty, True)):
        rig.begin()
        for c in range(2):
            reward, done, info = rig.inputs()
            if c == 0:
                done[r0], info[r0, 0] = 1, want_w
                if bad:
                    reward[r0], info[r0, 0] = np.nan, bad_info
            rig.step(reward, done, info, check=False)
        outs.append(rig.fold(check=False))
        torch.cuda.synchronize()
    others = np.arange(C * n) != r0
    for k in ("live", "length", "count", "step", "winner"):
        assert np.array_equal(host(clean.t[k]), host(dirty.t[k])), k
    assert int(host(dirty.t["winner"])[r0]) == want_w and int(host(dirty.t["live"])[r0]) == 0
    ret_c, ret_d = host(clean.t["ret"]), host(dirty.t["ret"])
    assert np.array_equal(bits(ret_c[others]), bits(ret_d[others])) and np.isnan(ret_d[r0]) and np.isfinite(ret_c[r0])
    assert np.array_equal(bits(host(clean.t["opp_inc"])), bits(host(dirty.t["opp_inc"])))
    (oc, lc, rc), (od, ld, rd) = outs
    assert np.array_equal(oc, od) and np.array_equal(lc, ld)
    assert np.array_equal(bits(rc[[0, 2]]), bits(rd[[0, 2]])) and np.isnan(rd[1]) and np.isfinite(rc[1])
    # the laws contain it the same way
    assert np.array_equal(dirty.state["winner"], host(dirty.t["winner"]))
    assert np.isnan(dirty.state["ret"][r0]) and np.array_equal(bits(dirty.state["ret"][others]), bits(ret_d[others]))


def test_refusals_and_the_struct_size():
    """Every HKL_E_INVALID case of the header, with a message that names it; hkl_eval_io_size() is the ctypes struct's."""
    from test_evaluator_law import refusal_cases

    L = LH.lib()
    assert L.hkl_eval_io_size() == ctypes.sizeof(LH.EvalIO)
    for name, rows in refusal_cases(LH).items():
        for io, word in rows:
            assert getattr(L, name)(None if io is None else ctypes.byref(io), None) == 1, (name, word)
            msg = L.hkl_last_error().decode()
            assert msg.startswith(name + ": ") and word in msg, (name, word, msg)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- end to end
EPISODES, REPLICAS = 6, 2
P1, P2, SEEDS = [0, 0, 1, 1], ["weak", "strong", "weak", "strong"], [42, 42, 7, 7]
PER_EPISODE = ("winner", "returns", "lengths")
CELL = ("win", "draw", "loss", "mean_return", "mean_length", "unfinished")


def _actors(k=2, seed=11):
    from hockey_amd.evaluate import Actor

    torch.manual_seed(seed)
    return [Actor().to(DEV).eval() for _ in range(k)]


def _bank(actors):
    from hockey_amd.policy_bank import PolicyBank

    bank = PolicyBank(len(actors), DEV)
    for a in actors:
        bank.add(a)
    return bank


def _same(a, b, rows=slice(None), rows_b=slice(None)):
    for k in PER_EPISODE + CELL:
        x, y = np.asarray(a[k])[rows], np.asarray(b[k])[rows_b]
        assert x.shape == y.shape and x.dtype == y.dtype, k
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                              y.view(np.uint64) if y.dtype == np.float64 else y), k


@pytest.fixture(scope="module")
def batch():
    """Two seeded random actors, 4 cells (2 x weak / strong), 6 episodes x 2 replicas, played to the end on the
    kernels: computed once, shared, left unchanged."""
    bank = _bank(_actors())
    ev = E.Evaluator(4, EPISODES, REPLICAS, device=DEV, backend="hip")
    r = ev.run(bank, P1, P2, SEEDS, per_episode=True)
    ev.close()
    assert not r["unfinished"].any() and r["winner"].shape == (4, REPLICAS, EPISODES)
    assert (r["lengths"] >= 1).all() and (r["lengths"] <= 251).all()
    assert np.allclose(r["win"] + r["draw"] + r["loss"], 1.0)
    return bank, r


def test_hip_and_torch_backends_agree_bit_for_bit(batch):
    bank, want = batch
    ev = E.Evaluator(4, EPISODES, REPLICAS, device=DEV, backend="torch")
    _same(ev.run(bank, P1, P2, SEEDS, per_episode=True), want)
    ev.close()


def test_a_cell_alone_equals_its_slice_of_the_batch(batch):
    bank, want = batch
    ev = E.Evaluator(1, EPISODES, REPLICAS, device=DEV, backend="hip")
    for c in range(4):
        got = ev.run(bank, P1[c:c + 1], P2[c:c + 1], SEEDS[c:c + 1], per_episode=True)
        _same(got, want, rows_b=slice(c, c + 1))
    ev.close()


@pytest.mark.parametrize("poll_every", [1, 1000])
def test_results_do_not_depend_on_poll_every(batch, poll_every):
    """The fixture polls every 16 steps; 1 stops at the longest game, 1 000 never polls."""
    bank, want = batch
    ev = E.Evaluator(4, EPISODES, REPLICAS, device=DEV, backend="hip", poll_every=poll_every)
    _same(ev.run(bank, P1, P2, SEEDS, per_episode=True), want)
    assert ev.steps == (int(want["lengths"].max()) if poll_every == 1 else 251)
    ev.close()


def test_a_reused_evaluator_equals_a_fresh_one(batch):
    """A second run with other seeds and opponents on the same Evaluator equals a fresh Evaluator's, and a third with
    the first seeds equals the fixture."""
    bank, want = batch
    p2, seeds = ["strong", "weak", "weak", "strong"], [5, 99, 5, 1234]
    ev = E.Evaluator(4, EPISODES, REPLICAS, device=DEV, backend="hip")
    ev.run(bank, P1, P2, SEEDS)
    second = ev.run(bank, P1, p2, seeds, per_episode=True)
    third = ev.run(bank, P1, P2, SEEDS, per_episode=True)
    ev.close()
    fresh = E.Evaluator(4, EPISODES, REPLICAS, device=DEV, backend="hip")
    _same(second, fresh.run(bank, P1, p2, seeds, per_episode=True))
    fresh.close()
    _same(third, want)


def test_cross_play_has_the_tournaments_shapes_and_evaluate_manys_bot_columns():
    """cross_play of 2 actors x 3 games: tournament_fold's keys and [K][cols] shapes, its rates tournament_fold's of
    the per-game winners; the bot columns (weak: K, strong: K + 1) equal evaluate_many's cells for the same seeds; an
    actor's slot as player 2 plays (the self column is not the bots')."""
    from hockey_amd.evaluate import tournament_fold

    actors = _actors(2, seed=4)
    cp = E.cross_play(actors, games=3, seed=42, device=DEV, per_game=True)
    ref = tournament_fold(cp["winner"].reshape(-1), np.zeros(2 * 4 * 3), 2, 3)
    assert set(cp) == set(ref) | {"winner"} and cp["winner"].shape == (2, 4, 3) and cp["winner"].dtype == np.int8
    for k, v in ref.items():
        assert cp[k].shape == v.shape == (2, 4), k
        if k != "mean_length":
            assert np.array_equal(cp[k], v), k
    em = E.evaluate_many(actors, episodes=3, seeds=42, opponents=("weak", "strong"), device=DEV, per_episode=True)
    assert em["win"].shape == (2, 2) and em["winner"].shape == (2, 2, 1, 3)
    for k in ("win", "draw", "loss", "mean_length"):
        assert np.array_equal(cp[k][:, 2:], em[k]), k
    assert np.array_equal(cp["winner"][:, 2:], em["winner"][:, :, 0])
    assert (cp["mean_length"] >= 1).all() and (cp["mean_length"] <= 251).all()
    no_bots = E.cross_play(actors, games=3, seed=42, device=DEV, include_bots=False, per_game=True)
    assert no_bots["win"].shape == (2, 2) and np.array_equal(no_bots["winner"], cp["winner"][:, :2])


def test_agreement_with_evaluate_in_distribution():
    """One random actor against the weak bot, 512 episodes, seed 42, through evaluate() and evaluate_many: the same
    placements and starting phases, increments that differ in distribution only.  |z| < 4 for the difference in loss
    rate (two-sample binomial, pooled) and in mean length (Welch).  evaluate() reports the mean length only, so its
    per-game variance is taken to be evaluate_many's, which it is under the hypothesis tested; the runs are positively
    correlated, so the bound is conservative."""
    from hockey_amd.evaluate import evaluate

    n = 512
    actor = _actors(1, seed=21)[0]
    a = evaluate(actor, episodes=n, seed=42, weak_opponent=True, device=DEV)
    b = E.evaluate_many([actor], episodes=n, seeds=42, opponents=("weak",), device=DEV, per_episode=True)
    assert b["episodes"] == n and not b["unfinished"].any()
    pa, pb = a["loss"], float(b["loss"][0, 0])
    pool = 0.5 * (pa + pb)
    se = math.sqrt(2.0 * pool * (1.0 - pool) / n)
    z_loss = (pa - pb) / se if se > 0 else 0.0
    var = float(b["lengths"].astype(np.float64).var(ddof=1))
    se = math.sqrt(2.0 * var / n)
    z_len = (a["mean_length"] - float(b["mean_length"][0, 0])) / se if se > 0 else 0.0
    print(f"loss {pa:.4f} / {pb:.4f} z {z_loss:.2f}; length {a['mean_length']:.2f} / "
          f"{float(b['mean_length'][0, 0]):.2f} z {z_len:.2f}")
    assert abs(z_loss) < 4 and abs(z_len) < 4
    assert abs(float(b["mean_length"][0, 0]) - b["lengths"].mean()) < 1e-9
