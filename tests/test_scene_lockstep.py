"""The harness of tests/scene_lockstep.py checked on itself: check_step / check_end / same_bits see one changed word,
and name the BATCH's arena (rows[i], not the row i of the context) and the step.

A real run of the host build -- the first wave of toi_lean_zoo's batch, 64 arenas, W.K steps -- is presented through a
wrapper that permutes the rows and changes exactly one thing.  Unchanged, the same run passes.  CPU only.
"""
import copy

import numpy as np
import pytest

import toi_lean_zoo as Z
import wave_zoo as W
from hockey_amd import _native as N
from hostcheck import HostVec
from scene_lockstep import (STEP_FIELDS, check_end, check_step, oracle_run, run_batch, same_bits, scene_env,
                            wave_permutation)

T, ROW = 2, 17  # the step and the context's row that the cases change


class Replay:
    """A finished run behind get_state / counters, its rows in the order `rows`."""

    def __init__(self, steps, state, counters, rows):
        self.steps = [{f: s[f][rows].copy() for f in STEP_FIELDS} for s in steps]
        self.state, self.aux = state[0][rows].copy(), state[1][rows].copy()
        self.c = np.array(counters, np.int64)

    def get_state(self):
        return self.state, self.aux

    def counters(self):
        return self.c


@pytest.fixture(scope="module")
def run(oracle):
    """(want, toi labels, the host build's run) of the wave, computed once."""
    b = Z.lean_batch()
    state, aux, actions, toi = b.state[:64], b.aux[:64], b.actions[:, :64], b.toi[:64]
    env = scene_env(HostVec, state, aux)
    steps = run_batch(env, actions, "hk_step")
    got = (steps, env.get_state(), env.counters())
    env.close()
    assert len(steps) == W.K and toi.sum() > 0
    return oracle_run(oracle, state, aux, actions), toi, got


def _flip(a, index):
    a.view(np.uint32 if a.dtype.itemsize == 4 else a.dtype)[index] ^= 1


CASES = {
    "obs_bit": lambda r: _flip(r.steps[T]["obs"], (ROW, 5)),
    "done_byte": lambda r: _flip(r.steps[T]["done"], ROW),
    "state_word": lambda r: _flip(r.state, (ROW, 3)),
    "aux_entry": lambda r: _flip(r.aux, (ROW, 2)),
    "toi_counter": lambda r: r.c.__setitem__(N.CNT_TOI, r.c[N.CNT_TOI] + 1),
}


def _check(replay, want, toi, rows):
    for t in range(W.K):
        check_step(t, replay.steps[t], want["steps"][t], "replay", rows, lambda arena, t: "scenario of %d" % arena)
    check_end(replay, want, "replay", rows, toi=toi, large=0)


@pytest.fixture(scope="module")
def rows():
    perm = wave_permutation(64)
    assert perm[ROW] != ROW
    return perm


def test_unchanged_run_passes(run, rows):
    want, toi, got = run
    _check(Replay(*got, np.arange(64)), want, toi, None)
    _check(Replay(*got, rows), want, toi, rows)


@pytest.mark.parametrize("case", list(CASES))
def test_one_changed_word_fails_and_names_the_batchs_arena(run, rows, case):
    want, toi, got = run
    replay = Replay(*got, rows)
    CASES[case](replay)
    with pytest.raises(AssertionError) as e:
        _check(replay, want, toi, rows)
    msg = str(e.value)
    if case == "toi_counter":
        assert "TOI counter" in msg
        return
    step = T if case in ("obs_bit", "done_byte") else W.K - 1
    assert "arena %d" % rows[ROW] in msg and "step %d" % step in msg, msg
    assert "arena %d " % ROW not in msg and "arena %d:" % ROW not in msg, msg
    if case in ("obs_bit", "done_byte"):
        assert "scenario of %d" % rows[ROW] in msg, msg


def test_same_bits_names_step_arena_and_label(run):
    _, _, (steps, _, _) = run
    stack = np.stack([s["obs"] for s in steps])
    assert stack.shape == (W.K, 64, 18)
    label = ["lane %d" % i for i in range(64)]
    same_bits(stack, copy.deepcopy(stack), "observation", label, first=10)
    changed = stack.copy()
    _flip(changed, (T, ROW, 7))
    with pytest.raises(AssertionError) as e:
        same_bits(changed, stack, "observation", label, first=10)
    msg = str(e.value)
    assert "step %d" % (T + 10) in msg and "arena %d (lane %d)" % (ROW, ROW) in msg, msg
    done = np.stack([s["done"] for s in steps])
    same_bits(done, done.copy(), "done")
    changed = done.copy()
    _flip(changed, (T, ROW))
    with pytest.raises(AssertionError, match="step %d, arena %d" % (T, ROW)):
        same_bits(changed, done, "done")
