"""TOI event waves for the step kernel's two event routines (hk_world.h solve_toi: toi_island_solve_one for a lane
whose mini-island has one contact on register slots, toi_island_solve otherwise).  TEST INFRASTRUCTURE ONLY.

Composed from the one-arena scenarios of tests/golden/wave_zoo.npz through wave_zoo.Zoo.pool, keys toi1 / toi2 / toi3 /
toim2 at the label step J.  The tests that use it compare against the oracle at tolerance zero: they pin what the
event path computes, whichever routine runs it.

Waves, in order:
  0  64 lanes, every lane a toi1 scenario whose events are all one-contact: the lean routine runs alone;
  1  toi1 lanes and one toim2 lane whose two-contact event is the lane's first of the step, so it falls into the
     same round as the toi1 lanes' events: both routines run in one round of one wave;
  2  toi2 / toi3 lanes beside toi1 lanes: later rounds have fewer event lanes, the routine is chosen again per round;
  3  a last wave of 37 lanes with one toi1 lane (`single`: its arena), the rest idle.
The same single scenario is also what the tests run as a one-arena context, where lane 0 is alone.
"""
import numpy as np

import wave_zoo as W
from scene_lockstep import wave_permutation

J = W.J
SINGLE_LANE = 11


def _pure(zoo, ids):
    """Scenarios whose TOI events, at every step, are one-contact mini-islands on register slots."""
    d = zoo.d
    return [i for i in ids if not d["toi_n2"][i].any() and not d["toi_big"][i].any() and (d["ncont"][i] <= 4).all()]


class LeanBatch:
    def __init__(self, zoo):
        d, pool = zoo.d, zoo.pool
        idle = pool[(J, "idle")]
        toi1 = _pure(zoo, pool[(J, "toi1")])
        toi2, toi3 = _pure(zoo, pool[(J, "toi2")]), _pure(zoo, pool[(J, "toi3")])
        # a two-contact mini-island as the lane's only event of the label step: it is in round one
        m2 = [i for i in pool[(J, "toim2")] if d["toi"][i, J] == 1 and d["toi_n2"][i, J] == 1 and not d["toi_big"][i].any()
              and (d["ncont"][i] <= 4).all()]
        m2.sort(key=lambda i: int(d["toi"][i].sum()))  # first: a scenario with no other event in its K steps
        assert len(toi1) >= 8 and toi2 and toi3 and m2 and idle
        self.toi1, self.m2 = toi1, m2

        def wave(width, at):
            w = [idle[k % len(idle)] for k in range(width)]
            for lane, i in at.items():
                w[lane] = i
            return w

        waves = [
            [toi1[k % len(toi1)] for k in range(64)],
            wave(64, {**{2 * k + 1: toi1[(k + 3) % len(toi1)] for k in range(20)}, 13: m2[0], 63: toi1[0]}),
            wave(64, {0: toi2[0], 7: toi3[0], 20: toi1[1], 21: toi1[2], 33: toi2[-1], 40: toi1[5], 63: toi3[-1],
                      50: toi1[4]}),
            wave(37, {SINGLE_LANE: toi1[0]}),
        ]
        self.wave0 = [len(w) for w in waves]
        self.idx = np.array([i for w in waves for i in w])
        self.n = len(self.idx)
        self.single = self.n - 37 + SINGLE_LANE
        self.state, self.aux = d["state"][self.idx], d["aux"][self.idx]
        self.actions = np.ascontiguousarray(d["actions"][self.idx].transpose(1, 0, 2))  # [K, n, 8]
        self.toi = d["toi"][self.idx].astype(np.int64)  # [n, K]
        # events of one-contact mini-islands: what solve_toi sends down the lean routine
        self.toi_one = self.toi - d["toi_n2"][self.idx] - d["toi_big"][self.idx]
        self.large = int((d["ncont"][self.idx] > 4).sum() + d["toi_big"][self.idx].sum())
        assert self.large == 0 and (self.toi[:64, J] == 1).all() and (self.toi_one[:64] == self.toi[:64]).all()

    def one(self, arena):
        """(state, aux, actions [K, 1, 8], toi [1, K]) of one arena of the batch, as a batch of its own."""
        s = slice(arena, arena + 1)
        return self.state[s], self.aux[s], np.ascontiguousarray(self.actions[:, s]), self.toi[s]

    def permutation(self, seed=64):
        """The lanes of every wave permuted (fixed seed)."""
        return wave_permutation(self.n, seed)

    def describe(self, arena, t):
        i = int(self.idx[arena])
        d = self.zoo_d
        return "wave %d lane %d scenario %d: toi %s two-contact %s" % (
            arena // 64, arena % 64, i, d["toi"][i].tolist(), d["toi_n2"][i].tolist())


def lean_batch():
    zoo = W.Zoo()
    b = LeanBatch(zoo)
    b.zoo_d = zoo.d
    return b
