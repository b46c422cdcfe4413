"""hockey_amd.collect without a GPU: the store law (the Collector's torch backend) against store_step +
PopulationRing.push + the mix's tally, the draw law's shares, shape cases and per-member keying, the C ABI's struct
layout, exports and host-side refusals, and train / train_population with collect="device" on the kernel source's host
build."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from hockey_amd import _native as N
from hockey_amd import collect as C
from hockey_amd.opponents import PopulationOpponentMix
from hockey_amd.population import PopulationRing
from hockey_amd.td3 import TD3Config, store_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mix(S, n, pool=3):
    cfg = TD3Config(use_self_play=True, self_play_pool_size=pool, curriculum_name="stage3")
    return PopulationOpponentMix([cfg] * S, list(range(11, 11 + S)), n, "cpu", sampling="arena")


# ---------------------------------------------------------------------------------------------------- the store law
@pytest.mark.parametrize("episode_end", ["max_steps", "done"])
@pytest.mark.parametrize("S,n", [(S, n) for S in (1, 3) for n in (1, 5, 65)])
def test_store_law_equals_store_step_push_and_tally(S, n, episode_end):
    """Four steps of random rows through ``Collector(backend="torch").store`` and through today's code -- store_step,
    the ragged PopulationRing.push and the mix's per-step tally -- at cap = n + 3 (every ring wraps within three
    steps): ring columns, write positions, fill levels, episode rewards, alive flags and tallies are byte-equal."""
    NN, cap, P, done_mode = S * n, n + 3, 3, episode_end == "done"
    g = torch.Generator().manual_seed(100 * S + n)
    rnd = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    snap = torch.randint(-1, P, (NN,), generator=g)
    snap = torch.where(snap >= 0, snap + P * (torch.arange(NN) // n), snap).to(torch.int32)  # fixed: (member, k) or -1
    alive0 = torch.rand(NN, generator=g) < 0.7
    obs0, obs20 = rnd(NN, 18), rnd(NN, 18)
    # ---- today's code
    ring, mix = PopulationRing(S, cap, device="cpu"), _mix(S, n)
    mix._snap, mix._sp_mask = snap.clamp(min=0).long(), snap >= 0
    member_of = torch.arange(NN) // n
    alive, ep = alive0.clone(), torch.zeros(NN)

    def store(rows, res, *row):
        # PopulationRing.push refuses a batch of more rows than ONE ring holds, which S n rows are at cap = n + 3:
        # the step's rows go in as one ragged push per member, in member order (what push states it equals)
        m = member_of if rows is None else member_of[rows]
        for j in range(S):
            ring.push(m[m == j], *[x[m == j] for x in row])

    # ---- the Collector
    ring2 = PopulationRing(S, cap, device="cpu")
    col = C.Collector(None, None, _mix(S, n), ring2, None, list(range(11, 11 + S)), n, backend="torch",
                      episode_end=episode_end)
    col.begin_round(obs0, obs20, 4)
    col.alive.copy_(alive0.to(torch.uint8))
    obs = obs0
    for t in range(4):
        a, r, o2, o22 = rnd(NN, 4), rnd(NN), rnd(NN, 18), rnd(NN, 18)
        d = (torch.rand(NN, generator=g) < 0.3).to(torch.uint8)
        store_step(store, mix, done_mode, alive, ep, None, obs, a, r, o2, d)
        col.act8[:, :4] = a
        col.snap.copy_(snap)
        col.store(o2, o22, r, d)
        obs = o2
        for k in ("s", "a", "r", "s2", "d", "pos_t", "size_t"):
            assert torch.equal(getattr(ring, k), getattr(ring2, k)), (t, k)
        assert torch.equal(ep, col.ep_reward) and torch.equal(mix._outcomes[t], col.tally[t]), t
        assert torch.equal(col.obs, o2) and torch.equal(col.obs2, o22)
        if done_mode:
            assert torch.equal(alive.to(torch.uint8), col.alive)
            assert torch.equal(alive.view(S, n).sum(1).to(torch.int32), col.count)
    assert int(ring.size_t.max()) == cap or (done_mode and n == 1)  # the rings wrapped


def test_store_law_skips_a_member_with_a_bad_position():
    r = C.collect_law(2, 5, np.ones(4, np.float32), np.zeros(4), None, None, [7, 1], [0, 0], np.zeros(4), [0, 0], 2)
    assert r["dst"].tolist() == [-1, -1, 5 + 1, 5 + 2] and r["pos"].tolist() == [7, 3]
    assert r["push_n"].tolist() == [0, 2] and r["size"].tolist() == [0, 2] and r["steps"].tolist() == [2, 2]


# ---------------------------------------------------------------------------------------------------- the draw law
def _draw(seeds, n, lens, scores, calls=None, p=(0.25, 0.5), alive=None):
    S, P = len(seeds), np.asarray(scores).shape[1]
    slots = np.arange(S * P, dtype=np.int32).reshape(S, P) + 100
    return C.opp_draw_law(seeds, n, np.zeros(S, np.int64) if calls is None else calls,
                          np.tile(np.float32(p), (S, 1)), lens, scores, slots, alive)


def test_draw_law_shares_within_five_sigma():
    """p_self = 0.25, p_strong = 0.5 (exact float32), scores [1, 2, 5], 200 000 rows of one member at a fixed seed:
    the strong, weak, self-play and per-snapshot shares each lie within a 5-sigma binomial bound."""
    n = 200_000
    r = _draw([20261021], n, [3], [[1.0, 2.0, 5.0]])
    want = {"strong": 0.375, "weak": 0.375, "sp": 0.25}
    got = {"strong": (r["policy2"] == N.POLICY_BASIC_STRONG).sum(), "weak": (r["policy2"] == N.POLICY_BASIC_WEAK).sum(),
           "sp": (r["policy2"] == N.POLICY_EXTERNAL).sum()}
    for k, sc in enumerate((1.0, 2.0, 5.0)):
        want[f"snap{k}"] = 0.25 * sc / 8.0
        got[f"snap{k}"] = (r["snap"] == k).sum()
    for key, p in want.items():
        assert abs(int(got[key]) - n * p) <= 5.0 * np.sqrt(n * p * (1 - p)), (key, got[key], n * p)
    assert r["counts"].tolist() == [[got["strong"], got["weak"], got["sp"]]]
    assert r["snap_counts"].tolist() == [got["snap0"], got["snap1"], got["snap2"]]
    assert np.array_equal(r["policy"] >= 0, r["snap"] >= 0) and np.array_equal(r["policy"][r["snap"] >= 0] - 100,
                                                                                r["snap"][r["snap"] >= 0])
    assert r["opp_inc"].min() >= 0 and r["opp_inc"].max() < 0.2 and abs(r["opp_inc"].mean() - 0.1) < 1e-3
    assert r["calls"].tolist() == [1]


def test_draw_law_shape_cases():
    """A member with len 0 and a member with a non-finite or non-positive total draw no self-play; u_snap close to 1
    picks len - 1; len is cut to [0, pmax]; counts are taken over alive rows only, every row is drawn."""
    n = 4000
    sc = np.array([[1, 1, 1], [1, np.inf, 1], [1, np.nan, 1], [0, 0, 0], [1, 2, 5]], np.float32)
    r = _draw([5, 6, 7, 8, 9], n, [0, 3, 3, 3, 7], sc, p=(1.0, 0.5))
    sp = (r["policy2"] == N.POLICY_EXTERNAL).reshape(5, n)
    assert not sp[:4].any() and sp[4].all()  # p_self = 1: every row of the one member that can
    assert (r["snap"][:4 * n] == -1).all() and (r["policy"][:4 * n] == -1).all()
    k = r["snap"][4 * n:] - 4 * 3
    assert k.min() == 0 and k.max() == 2  # len 7 is cut to pmax = 3
    # u_snap close to 1: the row whose 53-bit draw is the largest picks the last snapshot, also past a rounding
    w = C.draw_words(9, C.KEY_OPP, n, 0)
    u = C.u53(w[:, 2], w[:, 3])
    assert k[u.argmax()] == 2 and u.max() > 0.999
    tiny = _draw([9], n, [3], np.array([[5, 2, 1e-30]], np.float32), p=(1.0, 0.5))
    assert set(np.unique(tiny["snap"])) <= {0, 1, 2} and (tiny["snap"] >= 0).all()
    alive = np.zeros(5 * n, np.uint8)
    alive[4 * n:4 * n + 10] = 1
    r2 = _draw([5, 6, 7, 8, 9], n, [0, 3, 3, 3, 3], sc, p=(1.0, 0.5), alive=alive)
    assert r2["counts"].sum() == 10 and r2["counts"][4].tolist() == [0, 0, 10] and r2["snap_counts"].sum() == 10
    assert np.array_equal(r2["policy2"], r["policy2"])


def test_draws_are_keyed_per_member():
    """Member j's draws and opp_inc are the same bits at S = 1 and as member 2 of 3."""
    n, P = 257, 3
    sc = np.array([[1, 2, 5]], np.float32)
    solo = _draw([77], n, [3], sc, calls=np.array([5]), p=(0.5, 0.5))
    pop = _draw([3, 4, 77], n, [1, 0, 3], np.array([[9, 9, 9], [1, 1, 1], [1, 2, 5]], np.float32),
                calls=np.array([0, 9, 5]), p=(0.5, 0.5))
    rows = slice(2 * n, 3 * n)
    assert np.array_equal(solo["policy2"], pop["policy2"][rows])
    assert np.array_equal(solo["opp_inc"].view(np.uint64), pop["opp_inc"][rows].view(np.uint64))
    sp = solo["snap"] >= 0
    assert sp.any() and np.array_equal(sp, pop["snap"][rows] >= 0)
    assert np.array_equal(solo["snap"][sp], pop["snap"][rows][sp] - 2 * P)
    assert np.array_equal(C.phase_rows(77, n), C.phase_rows(77, n)) and C.phase_rows(77, n).shape == (n, 3)
    assert 0 <= C.phase_rows(77, n).min() and C.phase_rows(77, n).max() < np.pi
    assert not np.array_equal(C.phase_rows(78, n), C.phase_rows(77, n))


# ---------------------------------------------------------------------------------------------------- C ABI
def test_collect_abi_layout_exports_and_refusals(tmp_path):
    """include/hockey_collect.h as the C compiler lays it out against the ctypes structs; the library exports the
    entry points; each call refuses a malformed struct on the host (no GPU: nothing is launched) with HKL_E_INVALID
    and a message that names it."""
    from hockey_amd import learner_hip as LH

    probes = {"OppDrawIO": "hkl_opp_draw_io", "CollectIO": "hkl_collect_io"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hockey_learner.h"', "int main(void) {"]
    for py, cname in probes.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in getattr(LH, py)._fields_:
            lines.append(f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines += ['  printf("keys %llx %llx\\n", (unsigned long long)HKL_COLLECT_KEY_OPP, '
              '(unsigned long long)HKL_COLLECT_KEY_PHASE);',
              '  printf("ids %d %d %d\\n", HKL_P2_EXTERNAL, HKL_P2_WEAK, HKL_P2_STRONG);', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    want = dict(line.split(None, 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for py, cname in probes.items():
        S = getattr(LH, py)
        assert ctypes.sizeof(S) == int(want[cname]), cname
        for f, _ in S._fields_:
            assert getattr(S, f).offset == int(want[f"{cname}.{f}"]), (cname, f)
    assert want["keys"].split() == [f"{C.KEY_OPP:x}", f"{C.KEY_PHASE:x}"]
    assert [int(x) for x in want["ids"].split()] == [N.POLICY_EXTERNAL, N.POLICY_BASIC_WEAK, N.POLICY_BASIC_STRONG]

    L = LH.lib()
    assert all(hasattr(L, name) for name in LH.COLLECT_EXPORTS)
    assert L.hkl_opp_draw_io_size() == ctypes.sizeof(LH.OppDrawIO)
    assert L.hkl_collect_io_size() == ctypes.sizeof(LH.CollectIO)
    assert L.hkl_collect_scratch_ints(3 * 257, 257) == 64 + 3 * 3 * 2 and L.hkl_collect_scratch_ints(0, 4) == 0

    def good(S, n_rows=40, rpm=20, **kw):
        io = S()
        for f, t in S._fields_:
            if t is ctypes.c_void_p:
                setattr(io, f, 256)
        io.n_rows, io.rows_per_member, io.pmax = n_rows, rpm, 3
        if S is LH.CollectIO:
            io.act_ld, io.cap = 8, 100
        for k, v in kw.items():
            setattr(io, k, v)
        return io

    D, K = LH.OppDrawIO, LH.CollectIO
    layout = [(dict(rpm=0), "rows_per_member"), (dict(n_rows=41), "multiple"), (dict(n_rows=0), "multiple"),
              (dict(n_rows=65, rpm=1), "n_members"), (dict(pmax=0), "pmax")]
    cases = {"hkl_opp_draw": [(None, "null")] + [(good(D, **kw), w) for kw, w in layout] + [
                 (good(D, seeds=None), "seeds"), (good(D, calls=None), "calls"), (good(D, scores=None), "scores"),
                 (good(D, policy2=None), "policy2"), (good(D, snap_counts=None), "snap_counts")],
             "hkl_collect": [(None, "null")] + [(good(K, **kw), w) for kw, w in layout] + [
                 (good(K, cap=19), "cap"), (good(K, cap=0), "cap"), (good(K, act_ld=3), "act_ld"),
                 (good(K, obs=None), "obs"), (good(K, done=None), "done"), (good(K, s2=None), "ring"),
                 (good(K, pos=None), "pos"), (good(K, push_n=None), "push_n"), (good(K, scratch=None), "scratch"),
                 (good(K, tally=None), "tally"), (good(K, count=None), "count"),
                 (good(K, obs2_next=None), "obs2_next")]}
    for name, rows in cases.items():
        for io, word in rows:
            assert L.hkl_tanh_probe(None, None, 0, None) == 1  # another entry point's message in between
            assert getattr(L, name)(None if io is None else ctypes.byref(io), None) == 1, (name, word)
            msg = L.hkl_last_error().decode()
            assert msg.startswith(name + ": ") and word in msg, (name, word, msg)


# ---------------------------------------------------------------------------------------------------- training
def _cfg(**kw):
    base = dict(batch_size=32, use_self_play=False, curriculum_name="stage1", max_steps=30, start_steps=60,
                noise_mode="gaussian", buffer_size=4000)
    base.update(kw)
    return TD3Config(**base)


@pytest.mark.parametrize("episode_end", ["max_steps", "done"])
def test_train_collect_device_on_host_build(episode_end):
    """train(explore="device", collect="device") on the kernel source's host build (the Collector's torch backend),
    two rounds of 8 arenas: the documented stats, counts that add up, and the refusals."""
    from hockey_amd.td3 import train
    from hostcheck import HostTorchEnv

    n, steps = 8, 30 if episode_end == "max_steps" else 100
    env = HostTorchEnv(n, policies=("external", "external"))
    kw = dict(n_arenas=n, rounds=2, device="cpu", env=env, seed=5, explore="device", collect="device",
              updates_per_round=2, graphs=False, episode_end=episode_end, poll_every=7)
    agent, st = train(cfg=_cfg(max_steps=steps, curriculum_name="noise_study"), **kw)
    assert agent.total_steps == st["env_steps"] == st["replay_size"] and st["updates"] == 4
    if episode_end == "max_steps":
        assert st["env_steps"] == 2 * steps * n
    else:
        assert 0 < st["env_steps"] <= 2 * steps * n
    assert len(st["mean_reward"]) == len(st["opponents"]) == len(st["pool_size"]) == 2
    for opp in st["opponents"]:
        assert opp["self_play"] == 0 and opp["strong"] > 0 and opp["weak"] > 0
    assert sum(o["strong"] + o["weak"] for o in st["opponents"]) == st["env_steps"]
    assert all(torch.isfinite(p).all() for p in agent.actor.parameters())
    for bad, word in ((dict(explore="torch"), "explore"), (dict(self_play_sampling="step"), "step"),
                      (dict(on_step=lambda *a: None), "on_step"), (dict(collect="gpu"), "collect")):
        with pytest.raises(ValueError, match=word):
            train(cfg=_cfg(), **{**kw, **bad})


def test_train_population_collect_device_on_host_build():
    """train_population(explore="device", collect="device", self_play="arena") on the host build: S = 2 members x 8
    arenas, two rounds, the second against the first round's snapshots.  Per member: the documented stats, the counts
    add up to the arena-steps, the faced snapshots to the self-play count; and the refusals."""
    from hockey_amd.population import train_population
    from hostcheck import HostTorchEnv

    S, n, steps = 2, 8, 30
    env = HostTorchEnv(S * n, policies=("external", "external"))
    members = [(_cfg(use_self_play=True, curriculum_name="stage3", self_play_interval=8, self_play_pool_size=2,
                     noise_mode=k), 3 + j) for j, k in enumerate(("gaussian", "uniform"))]
    kw = dict(n_arenas=n, rounds=2, device="cpu", env=env, explore="device", collect="device", updates_per_round=2,
              graphs=False, self_play="arena")
    agents, st = train_population(members, **kw)
    for j, ag in enumerate(agents):
        assert ag.total_steps == st[j]["env_steps"] == st[j]["replay_size"] == 2 * steps * n
        assert st[j]["pool_size"] == [1, 2] and st[j]["updates"] == 4 and len(st[j]["mean_reward"]) == 2
        first, second = st[j]["opponents"]
        assert first["self_play"] == 0 and first["snapshots"] == []
        assert second["self_play"] > 0 and sum(second["snapshots"]) == second["self_play"]
        for opp in (first, second):
            assert opp["strong"] + opp["weak"] + opp["self_play"] == steps * n
    assert st[0]["opponents"] != st[1]["opponents"]  # per member, keyed by the member's seed
    for bad, word in ((dict(explore="torch"), "explore"), (dict(self_play="step"), "step"),
                      (dict(on_step=lambda *a: None), "on_step"), (dict(collect="hip"), "collect")):
        with pytest.raises(ValueError, match=word):
            train_population(members, **{**kw, **bad})
    # without self_play: no pools, per-member counts
    plain = [(_cfg(curriculum_name="noise_study"), 9), (_cfg(curriculum_name="noise_study"), 10)]
    _, st = train_population(plain, **{**kw, "self_play": None, "rounds": 1})
    assert all(s["opponents"][0]["strong"] + s["opponents"][0]["weak"] == steps * n for s in st)
    assert "pool_size" not in st[0]
