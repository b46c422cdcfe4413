"""hkl_opp_draw and hkl_collect (include/hockey_collect.h, csrc/hkl_collect.h) on the GPU against the laws in numpy
(hockey_amd.collect.opp_draw_law / collect_law, the Collector's torch backend): every output word, every ring byte and
every accumulator, compared as integers.  Outputs start as sentinels, so a word that should not have been written, or
was not, shows.

The shapes are the smallest that can go wrong: rows_per_member 1, 5, 64, 65, 257 (members inside one workgroup, members
that straddle workgroups) with 1, 3 and 64 members, one member of 4 097 rows (17 workgroups: the scan's prefix), rings
of n + 3 rows that wrap in every sequence, ragged pools with lengths 0 and pmax.

This file captures no graph and takes no stream from torch's pool (tests/test_gpu_facade.py's blocked-stream test runs
after it and depends on the streams handed out before): the graph and training tests are in
tests/test_gpu_population_collect.py.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hockey_amd import collect as C  # noqa: E402
from hockey_amd import learner_hip as LH  # noqa: E402

DEV = "cuda:0"
CELLS = [(S, n) for S in (1, 3, 64) for n in (1, 5, 64, 65, 257)]
P = 4


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def pools(S, seed):
    """Ragged pools: lengths cycle through 0, pmax and the values between (out-of-range ones included, which the
    kernel cuts), scores in [0.1, 10], slots unique."""
    rng = np.random.default_rng(seed)
    lens = np.array([(0, P, 1, 2, P + 3, 3, -2)[m % 7] for m in range(S)], np.int32)
    if S == 1:
        lens[:] = 3
    scores = rng.uniform(0.1, 10.0, (S, P)).astype(np.float32)
    slots = rng.permutation(S * P).astype(np.int32).reshape(S, P) + 7
    return lens, scores, slots


class DrawRig:
    """hkl_opp_draw's arguments as device tensors, and the same state in numpy for the law."""

    def __init__(self, S, n, seed=1, with_alive=False):
        rng = np.random.default_rng(seed)
        self.S, self.n = S, n
        N = S * n
        self.seeds = [int(x) for x in rng.integers(0, 2 ** 63, S)] if S > 1 else [2 ** 64 - 5]
        self.lens, self.scores, self.slots = pools(S, seed)
        self.probs = np.tile(np.float32([0.5, 0.5]), (S, 1))
        self.probs[::2, 0] = 0.75
        self.alive = (rng.random(N) < 0.6).astype(np.uint8) if with_alive else None
        self.calls = rng.integers(0, 2 ** 40, S).astype(np.int64)
        self.counts, self.snap_counts = rng.integers(0, 99, (S, 3)), rng.integers(0, 99, S * P)
        t = self.t = {"seeds": dev(np.array(self.seeds, np.uint64).view(np.int64)), "calls": dev(self.calls),
                      "probs": dev(self.probs), "len": dev(self.lens), "scores": dev(self.scores),
                      "slots": dev(self.slots), "policy2": torch.full((N,), 99, dtype=torch.uint8, device=DEV),
                      "policy": torch.full((N,), -7, dtype=torch.int32, device=DEV),
                      "snap": torch.full((N,), -7, dtype=torch.int32, device=DEV),
                      "opp_inc": torch.full((N, 2), float("nan"), dtype=torch.float64, device=DEV),
                      "counts": dev(self.counts), "snap_counts": dev(self.snap_counts)}
        if with_alive:
            t["alive"] = dev(self.alive)
        io = self.io = LH.OppDrawIO()
        io.n_rows, io.rows_per_member, io.pmax = N, n, P
        for k, v in t.items():
            setattr(io, k, v.data_ptr())

    def call(self):
        LH.check(LH.lib().hkl_opp_draw(ctypes.byref(self.io), LH.stream_ptr(torch.device(DEV))), "hkl_opp_draw")

    def law(self):
        r = C.opp_draw_law(self.seeds, self.n, self.calls, self.probs, self.lens, self.scores, self.slots, self.alive,
                           self.counts, self.snap_counts)
        self.calls, self.counts, self.snap_counts = r["calls"], r["counts"], r["snap_counts"]
        return r


@pytest.mark.parametrize("with_alive", [False, True])
@pytest.mark.parametrize("S,n", CELLS)
def test_opp_draw_equals_the_law_word_for_word(S, n, with_alive):
    """Two consecutive calls: policy2, policy, snap, opp_inc (as bits), counts, snap_counts and calls equal the law."""
    rig = DrawRig(S, n, seed=10 * S + n, with_alive=with_alive)
    seen_sp = 0
    for c in range(2):
        rig.call()
        want = rig.law()
        torch.cuda.synchronize()
        for k in ("policy2", "policy", "snap", "counts", "snap_counts", "calls"):
            assert np.array_equal(host(rig.t[k]).reshape(-1), np.asarray(want[k]).reshape(-1)), (c, k)
        assert np.array_equal(host(rig.t["opp_inc"]).view(np.uint64), want["opp_inc"].view(np.uint64)), c
        seen_sp += int((want["snap"] >= 0).sum())
    if S * n >= 64:
        assert seen_sp > 0
    if S > 1:  # the members without snapshots drew none
        empty = np.repeat(np.clip(rig.lens, 0, P) == 0, n)
        assert (host(rig.t["snap"])[empty] == -1).all() and (host(rig.t["policy2"])[empty] != 0).all()


class StoreRig:
    """hkl_collect's arguments as device tensors at cap = n + 3, the state in numpy, and the law applied to it."""

    RING = (("s", 18), ("a", 4), ("r", 0), ("s2", 18), ("d", 0))

    def __init__(self, S, n, alive=None, seed=3, alias=True):
        rng = self.rng = np.random.default_rng(seed)
        self.S, self.n, self.cap = S, n, n + 3
        N, cap = S * n, self.cap
        f = lambda *sh: rng.standard_normal(sh).astype(np.float32)  # noqa: E731
        self.h = {"obs": f(N, 18), "obs2": f(N, 18), "ep_reward": f(N), "pos": rng.integers(0, cap, S),
                  "size": rng.integers(0, cap + 1, S), "steps": rng.integers(0, 50, S), "live": rng.integers(0, 5, S),
                  "alive": None if alive is None else np.array(alive, np.uint8)}
        for k, w in self.RING:  # sentinels: a slot that was never written keeps them
            self.h[k] = np.full((S * cap, w) if w else (S * cap,), -3.0, np.float32)
        self.t = {k: dev(v) for k, v in self.h.items() if v is not None}
        z = lambda sh, dt, fill=0: torch.full(sh, fill, dtype=dt, device=DEV)  # noqa: E731
        self.t.update(push_pos=z((S,), torch.int64, -9), push_n=z((S,), torch.int64, -9),
                      count=z((S,), torch.int32, -9), tally=z((S * P, 2), torch.int64),
                      scratch=z((int(LH.lib().hkl_collect_scratch_ints(N, n)),), torch.int32),
                      act=z((N, 8), torch.float32), keep_obs=self.t["obs"] if alias else z((N, 18), torch.float32))
        self.alias = alias

    def step(self, c):
        """One call on fresh random step outputs and the law beside it; returns the law's dict."""
        S, n, cap, h, t, rng = self.S, self.n, self.cap, self.h, self.t, self.rng
        N = S * n
        f = lambda *sh: rng.standard_normal(sh).astype(np.float32)  # noqa: E731
        act, obs_next, obs2_next, reward = f(N, 8), f(N, 18), f(N, 18), f(N)
        done = (rng.random(N) < 0.3).astype(np.uint8)
        snap = rng.integers(-1, S * P + 1, N).astype(np.int32)  # S P itself: out of range, tallies nothing
        snap[:2] = (-5, 2 ** 30)[:len(snap[:2])]
        t["act"].copy_(dev(act))
        keep = [dev(x) for x in (obs_next, obs2_next, reward, done, snap)]
        io = LH.CollectIO()
        io.n_rows, io.rows_per_member, io.pmax, io.act_ld, io.cap = N, n, P, 8, cap
        for k in ("obs", "act", "s", "a", "r", "s2", "d", "pos", "size", "ep_reward", "tally", "push_pos", "push_n",
                  "count", "steps", "live", "keep_obs", "scratch") + (("alive",) if "alive" in t else ()):
            setattr(io, k, t[k].data_ptr())
        io.keep_obs2 = t["obs2"].data_ptr()
        io.obs_next, io.obs2_next, io.reward, io.done, io.snap = (x.data_ptr() for x in keep)
        t["tally"].zero_()
        LH.check(LH.lib().hkl_collect(ctypes.byref(io), LH.stream_ptr(torch.device(DEV))), "hkl_collect")
        r = C.collect_law(n, cap, reward, done, snap, h["alive"], h["pos"], h["size"], h["ep_reward"], h["steps"], S * P)
        rows = np.nonzero(r["dst"] >= 0)[0]
        at = r["dst"][rows]
        h["s"][at], h["a"][at], h["r"][at] = h["obs"][rows], act[rows, :4], reward[rows]
        h["s2"][at], h["d"][at] = obs_next[rows], done[rows].astype(np.float32)
        h["live"] = h["live"] + r["live"]
        for k in ("pos", "size", "steps", "ep_reward"):
            h[k] = r[k]
        if h["alive"] is not None:
            h["alive"] = r["alive"]
        before = h["obs"]
        h["obs"], h["obs2"] = obs_next if self.alias else before, obs2_next
        torch.cuda.synchronize()
        bits = lambda a: np.ascontiguousarray(a).view(np.int32)  # noqa: E731
        for k, _ in self.RING:
            assert np.array_equal(bits(host(t[k])), bits(h[k])), (c, k)
        for k in ("pos", "size", "steps", "live"):
            assert np.array_equal(host(t[k]), h[k]), (c, k)
        assert np.array_equal(bits(host(t["ep_reward"])), bits(h["ep_reward"])), c
        assert np.array_equal(host(t["tally"]), r["tally"]) and np.array_equal(host(t["push_pos"]), r["push_pos"])
        assert np.array_equal(host(t["push_n"]), r["push_n"]), c
        assert np.array_equal(bits(host(t["keep_obs"])), bits(obs_next)) and np.array_equal(bits(host(t["obs2"])),
                                                                                            bits(obs2_next))
        if not self.alias:
            assert np.array_equal(bits(host(t["obs"])), bits(before))
        if h["alive"] is not None:
            assert np.array_equal(host(t["alive"]), h["alive"]) and np.array_equal(host(t["count"]), r["count"]), c
        else:
            assert (host(t["count"]) == -9).all()
        assert not host(t["scratch"])[:64].any()  # the ticket words are zero again
        return r


def _alive(pattern, S, n, rng):
    if pattern == "null":
        return None
    a = np.ones(S * n, np.uint8)
    if pattern == "none":
        a[:] = 0
    elif pattern == "member":
        a[(S // 2) * n:(S // 2 + 1) * n] = 0
    elif pattern == "random":
        a = (rng.random(S * n) < 0.5).astype(np.uint8)
    return a


@pytest.mark.parametrize("pattern", ["null", "all", "none", "member", "random"])
@pytest.mark.parametrize("S,n", CELLS + [(1, 4097)])
def test_collect_equals_the_law_byte_for_byte(S, n, pattern):
    """Four consecutive calls at cap = n + 3 with keep_obs aliased to obs: every ring byte, pos, size, push_pos,
    push_n, ep_reward, the tally, steps, live, alive and count equal the law; a snap outside [-1, S pmax) tallies
    nothing; under alive == NULL count is not written."""
    rig = StoreRig(S, n, _alive(pattern, S, n, np.random.default_rng(S + n)), seed=S * 1000 + n)
    stored = 0
    for c in range(4):
        stored += int(rig.step(c)["push_n"].sum())
    if pattern == "null":
        assert stored == 4 * S * n and (rig.h["size"] == n + 3).all()  # the rings wrapped
    elif pattern == "all":
        assert stored >= S * n  # the first call stored every row; the done rows left afterwards
    elif pattern == "none":
        assert stored == 0


def test_collect_unaliased_keep_and_a_bad_position():
    """keep_obs in a buffer of its own leaves obs alone; a member whose pos lies outside [0, cap) stores nothing and
    keeps pos / size, the others are not disturbed."""
    rig = StoreRig(3, 65, _alive("random", 3, 65, np.random.default_rng(2)), seed=8, alias=False)
    rig.h["pos"][1] = rig.cap
    rig.t["pos"].copy_(dev(rig.h["pos"]))
    r = rig.step(0)
    assert r["push_n"][1] == 0 and r["pos"][1] == rig.cap and r["push_n"][0] > 0
    rig.h["pos"][1] = -1
    rig.t["pos"].copy_(dev(rig.h["pos"]))
    assert rig.step(1)["push_n"][1] == 0


def test_collect_then_per_push_group_equals_single_prioritized_rings():
    """The Collector's store on a PopulationPrioritizedRing (hkl_collect, then hkl_per_push_group on the push_pos /
    push_n / size arrays it left) over five steps of random survivors: each member's weights, block sums and maxima,
    fill level and columns equal a DevicePrioritizedRing fed the same rows by push."""
    from hockey_amd.opponents import PopulationOpponentMix
    from hockey_amd.population import PopulationPrioritizedRing
    from hockey_amd.td3 import DevicePrioritizedRing, TD3Config

    S, n, cap = 3, 65, 150
    cfg = TD3Config(use_self_play=False)
    mix = PopulationOpponentMix([cfg] * S, [1, 2, 3], n, DEV, sampling="arena")
    ring = PopulationPrioritizedRing(S, cap, device=DEV, init_weight=1.0)
    twins = [DevicePrioritizedRing(cap, device=DEV, init_weight=1.0) for _ in range(S)]
    col = C.Collector(None, None, mix, ring, None, [1, 2, 3], n, backend="hip", episode_end="done")
    g = torch.Generator().manual_seed(5)
    rnd = lambda *sh: torch.randn(*sh, generator=g).to(DEV)  # noqa: E731
    col.begin_round(rnd(S * n, 18), rnd(S * n, 18), 5)
    for t in range(5):
        alive = (torch.rand(S * n, generator=g) < 0.6).to(DEV)
        col.alive.copy_(alive.to(torch.uint8))
        obs = col.obs.clone()
        col.act8.copy_(rnd(S * n, 8))
        o2, o22, r = rnd(S * n, 18), rnd(S * n, 18), rnd(S * n)
        d = (torch.rand(S * n, generator=g) < 0.2).to(DEV).to(torch.uint8)
        col.store(o2, o22, r, d)
        for j, tw in enumerate(twins):
            rows = torch.nonzero(alive[j * n:(j + 1) * n]).squeeze(1) + j * n
            tw.push(obs[rows], col.act8[rows, :4], r[rows], o2[rows], d[rows])
        torch.cuda.synchronize()
        for j, tw in enumerate(twins):
            m = ring.member(j)
            for k in ("w", "_bsum", "_bmax", "s", "a", "r", "s2", "d"):
                assert torch.equal(getattr(m, k), getattr(tw, k)), (t, j, k)
            assert int(m.size_t) == tw.size and int(ring.pos_t[j]) == tw.pos
        # new priorities between the pushes, so that the next pushed maximum depends on the ring's history
        for j, tw in enumerate(twins):
            w = torch.rand(cap, generator=g).to(DEV) * (t + 1)
            tw.w.copy_(w)
            tw.refresh()
            ring.w[j * ring.wstride:j * ring.wstride + cap].copy_(w)
        ring.refresh()
