"""hockey_amd.explore without a GPU: its Philox against learner_ref's, explore_ref's schedule against a real TD3
object, the torch backend (the law in numpy) against explore_ref, the draws' moments, the C ABI's host-side checks and
struct layout, and train / train_population with explore="device" on the kernel source's host build."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import explore_ref as XR
import learner_ref as R
from hockey_amd import explore as X
from hockey_amd.policy_bank import PolicyBank
from hockey_amd.td3 import TD3, Actor, TD3Config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(**kw):
    """The same member for the package and for the reference."""
    return X.Member(**kw), XR.member(**kw)


# ---------------------------------------------------------------------------------------------------- Philox
def test_package_philox_equals_learner_ref_and_the_known_answer():
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 2 ** 32, (4096, 4), dtype=np.uint64).astype(np.uint32)
    ctr[0], ctr[1] = 0, 0xFFFFFFFF
    for key in (0, 0xFFFFFFFFFFFFFFFF, 0x9E3779B97F4A7C15, 42 ^ X.KEY_NOISE):
        assert np.array_equal(X.philox4x32_10(key, ctr), R.philox4x32_10(key, ctr)), key
    keys = rng.integers(0, 2 ** 63, 4096, dtype=np.uint64)
    assert np.array_equal(X.philox4x32_10(keys, ctr), R.philox4x32_10(keys, ctr))
    out = X.philox4x32_10(0, np.zeros(4, np.uint32))  # Random123 kat_vectors: philox4x32 10, zero counter and key
    assert [f"{int(v):08x}" for v in out] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    assert X.KEY_NOISE == XR.KEY_NOISE and X.KEY_RANDOM == XR.KEY_RANDOM
    for seed, calls in ((7, 0), (2 ** 64 - 3, 2 ** 32 + 9)):
        for purpose in (X.KEY_NOISE, X.KEY_RANDOM):
            assert np.array_equal(X.draw_words(seed, purpose, 70, calls), XR.words(seed, purpose, 70, calls))


# ---------------------------------------------------------------------------------------------------- schedule
# (total_steps before the call, n, count, start_steps, max_total_steps): wholly random, straddling the end of the
# random phase (with count < n and count == n), the first step past it, mid-schedule, progress exactly 1 and > 1, a
# member whose arenas have all ended, and no schedule at all
SWEEP = [(0, 8, 8, 100, 4000), (90, 8, 8, 100, 4000), (96, 8, 3, 100, 4000), (92, 8, 8, 100, 4000),
         (99, 8, 1, 100, 4000), (100, 8, 8, 100, 4000), (1000, 20, 20, 100, 4000), (1000, 20, 7, 0, 4000),
         (3980, 20, 20, 100, 4000), (3990, 20, 20, 0, 4000), (9000, 20, 5, 0, 4000), (500, 8, 0, 100, 4000),
         (95, 8, 0, 100, 4000), (123, 5, 5, 0, None), (1, 3, 3, 5, 1)]


@pytest.mark.parametrize("anneal", ["linear", "exp", "off"])
def test_reference_schedule_equals_td3_act(anneal):
    """Drive a real TD3 on the CPU: its random-phase rows (where act's output is not the actor's: the noise generator
    is replaced by zeros) equal the reference's mask exactly, its noise_scale() rounded to float32 the reference's
    scale, and its total_steps the reference's T1."""
    cfg = TD3Config(use_noise_annealing=anneal != "off", noise_anneal_mode="linear" if anneal == "off" else anneal,
                    noise_min_scale=0.03, action_noise_scale=0.25)
    agent = TD3(cfg, "cpu", seed=3, max_total_steps=4000)
    g = torch.Generator().manual_seed(1)
    seen = set()
    for total, n, count, start, max_total in SWEEP:
        agent.cfg.start_steps, agent.max_total_steps, agent.total_steps = start, max_total, total
        agent.current_noise_scale = agent.initial_noise_scale  # a fresh agent's (read when there is no schedule)
        agent.noise = lambda n=n: torch.zeros(n, 4)
        obs = torch.randn(n, 18, generator=g)
        with torch.no_grad():
            plain = agent.actor(obs)
        got = agent.act(obs, count=count)
        mem = XR.member(seed=3, start_steps=start, max_total_steps=max_total or 0, init_scale=0.25, min_scale=0.03,
                        anneal="none" if anneal == "off" else anneal)
        t0, t1, all_random, mask = XR.phase(total, count, n, start)
        assert agent.total_steps == t1
        assert np.array_equal((got != plain).any(1).numpy(), mask), (total, n, count, start)
        assert np.float32(agent.noise_scale()) == np.float32(XR.scale64(mem, t1))
        assert X.noise_scale(X.Member(**mem), t1) == np.float32(agent.noise_scale())
        if not all_random:
            assert agent.current_noise_scale == XR.scale64(mem, t1)
        seen.add(("all" if all_random else "some" if mask.any() else "none", count < n,
                  bool(max_total) and t1 > max_total))
    assert {s[0] for s in seen} == {"all", "some", "none"} and any(s[1] for s in seen) and any(s[2] for s in seen)


# ---------------------------------------------------------------------------------------------------- torch backend
def _bank(S, seed=0):
    torch.manual_seed(seed)
    bank = PolicyBank(S, "cpu")
    for j in range(S):
        bank.replace(j, Actor())
    return bank


MODES = ("gaussian", "ornstein-uhlenbeck", "uniform", "external", "none")


def _run_both(noise, n=13, calls=4, start=30, z=None):
    """S = 2 members of one mode (different seeds, one annealed linearly, one exponentially) for ``calls`` calls that
    start inside the random phase, straddle its end and leave it; count varies.  Yields per call (package, reference,
    actor actions)."""
    kw = [dict(seed=11, start_steps=start, max_total_steps=200, init_scale=0.3, min_scale=0.05, anneal="linear",
               noise=noise),
          dict(seed=2 ** 63 + 5, start_steps=start + 7, max_total_steps=60, init_scale=0.2, min_scale=0.02,
               anneal="exp", noise=noise, theta=0.2, dt=0.5)]
    pk, rf = zip(*[_pair(**k) for k in kw])
    bank = _bank(2)
    ex = X.Explorer(bank, list(pk), n, backend="torch", keep_draws=True)
    g = torch.Generator().manual_seed(9)
    total, cl, x = np.zeros(2, np.int64), np.zeros(2, np.int64), np.zeros((2 * n, 4), np.float32)
    for c in range(calls):
        obs = torch.randn(2 * n, 18, generator=g)
        ext = torch.randn(2 * n, 4, generator=g) if noise == "external" else None
        count = torch.tensor([n, max(n - c, 0)], dtype=torch.int32)
        a = bank.act(obs, ex.policy, backend="torch")
        out = ex.explore(obs, torch.full((2 * n, 6), 7.0), 1, count=count, ext=ext)
        ref = XR.call(rf, n, total, cl, count.numpy(), a.numpy(), x, None if ext is None else ext.numpy(),
                      z=ex.z.numpy() if z == "package" else None)
        total, cl, x = ref["total"], ref["calls"], ref["x"]
        yield ex, out, ref


@pytest.mark.parametrize("noise", ["uniform", "external", "none"])
def test_torch_backend_equals_reference_exactly(noise):
    phases = set()
    for ex, out, ref in _run_both(noise):
        assert torch.all(out[:, 0] == 7.0) and torch.all(out[:, 5] == 7.0)  # the other columns are untouched
        assert np.array_equal(out[:, 1:5].numpy().view(np.int32), ref["out"].view(np.int32))
        assert np.array_equal(ex.z.numpy(), ref["z"]) and np.array_equal(ex.scale.numpy(), ref["scale"])
        assert np.array_equal(ex.total.numpy(), ref["total"]) and np.array_equal(ex.calls.numpy(), ref["calls"])
        phases.add((bool(ref["random"][:13].all()), bool(ref["random"][:13].any())))
    assert phases == {(True, True), (False, True), (False, False)}  # member 0: wholly random, straddling, past


def test_torch_backend_ou_equals_reference_given_the_normals():
    """OU (and gaussian) given the package's own normals: actions and the OU state are exact, call after call; the
    state stays zero while the member is wholly random."""
    for noise in ("ornstein-uhlenbeck", "gaussian"):
        moved = False
        for ex, out, ref in _run_both(noise, calls=6, z="package"):
            assert np.array_equal(out[:, 1:5].numpy().view(np.int32), ref["out"].view(np.int32)), noise
            assert np.array_equal(ex.x.numpy().view(np.int32), ref["x"].view(np.int32))
            for m in range(2):
                rows = slice(13 * m, 13 * (m + 1))
                if ref["random"][rows].all() and not moved:
                    assert not ex.x.numpy()[rows].any()
            moved |= bool(ex.x.numpy().any())
        assert moved == (noise == "ornstein-uhlenbeck")


def test_torch_backend_normals_within_the_float32_bound():
    """The package's float32 Box-Muller against the float64 reference, under the bound sample_noise is held to."""
    for seed, calls in ((5, 0), (2 ** 40 + 1, 123456789012)):
        w = XR.words(seed, XR.KEY_NOISE, 4096, calls)
        ref64, ref32 = XR.normals(w), XR.normals(w, np.float32)
        got = X.normals(X.draw_words(seed, X.KEY_NOISE, 4096, calls))
        assert got.dtype == np.float32
        assert R.rel_err(got, ref64) <= R.bound(R.rel_err(ref32, ref64))


def test_reference_draw_moments():
    """4 x 10^5 reference draws per kind (10^5 rows x 4 components, seed 2024, call 3): gaussian mean and variance
    within 5 standard errors of 0 and 1 (se(mean) = 1 / sqrt N, se(var) = sqrt(2 / N)); uniform inside [-sqrt 3, sqrt 3)
    with variance 1 within 5 se (se(var) = sqrt((9/5 - 1) / N), the uniform's fourth moment); the random-phase draw
    inside [-1, 1) with mean 0 and variance 1/3."""
    n = 100_000
    N = 4 * n
    z = XR.normals(XR.words(2024, XR.KEY_NOISE, n, 3)).ravel()
    assert abs(z.mean()) <= 5 / math.sqrt(N) and abs(z.var() - 1) <= 5 * math.sqrt(2 / N)
    u = XR.uniform_pm1(XR.words(2024, XR.KEY_NOISE, n, 3)).ravel() * math.sqrt(3.0)
    assert u.min() >= -math.sqrt(3.0) and u.max() < math.sqrt(3.0)
    assert abs(u.mean()) <= 5 / math.sqrt(N) and abs(u.var() - 1) <= 5 * math.sqrt(0.8 / N)
    r = XR.uniform_pm1(XR.words(2024, XR.KEY_RANDOM, n, 3)).ravel()
    assert r.min() >= -1 and r.max() < 1 and abs(r.mean()) <= 5 * math.sqrt(1 / 3 / N)
    assert abs(r.var() - 1 / 3) <= 5 * math.sqrt((1 / 5 - 1 / 9) / N)
    assert not np.array_equal(r, u / math.sqrt(3.0))  # the two purposes are different streams


# ---------------------------------------------------------------------------------------------------- composition
def test_member_of_a_population_equals_its_own_run_given_the_observations():
    """Member j of a 3-member Explorer (gaussian / OU / pink, different seeds and start_steps) against a single-member
    Explorer for j fed the same observation rows: actions, OU state, scale and counters are equal bit for bit over 6
    calls with a noise reset in between, wherever j stands in the population.  torch's CPU GEMM is not batch-invariant
    (a row's actor output differs in the last bit between a 21-row and a 7-row forward), so member j's own bank
    replays the actor outputs recorded from the population's forward of the same observations; the kernel's acting
    tile is batch-invariant, and tests/test_gpu_explore.py feeds the observations alone."""
    n, kinds = 7, ("gaussian", "ornstein-uhlenbeck", "pink")
    mk = lambda j: X.Member(seed=100 + j, start_steps=10 * j, max_total_steps=300, init_scale=0.3, min_scale=0.05,  # noqa
                            anneal="linear", noise=kinds[j], seq_len=4)
    bank = _bank(3)
    pop = X.Explorer(bank, [mk(j) for j in range(3)], n, backend="torch")
    recorded = {}

    class Replay(PolicyBank):
        def _act_torch(self, obs, policy, out, out_col, base_slot=0):
            rows, seen_obs, a = recorded[self.j]
            assert torch.equal(obs, seen_obs[rows])
            out[:, out_col:out_col + 4] = a[rows]

    solo = []
    for j in range(3):
        b = Replay(1, "cpu")
        b.j = j
        b.replace(0, bank.state_dict(j))
        solo.append(X.Explorer(b, [mk(j)], n, backend="torch"))
    g = torch.Generator().manual_seed(4)
    for c in range(6):
        if c == 3:
            for e in [pop] + solo:
                e.reset_noise()
        obs = torch.randn(3 * n, 18, generator=g)
        out = pop.explore(obs, torch.zeros(3 * n, 4))
        a = bank.act(obs, pop.policy, backend="torch")
        for j in range(3):
            rows = slice(j * n, (j + 1) * n)
            recorded[j] = (rows, obs, a)
            own = solo[j].explore(obs[rows].clone(), torch.zeros(n, 4))
            assert torch.equal(out[rows], own), (c, j)
            assert torch.equal(pop.x[rows], solo[j].x) and pop.scale[j] == solo[j].scale[0]
            assert pop.total[j] == solo[j].total[0] == (c + 1) * n and pop.calls[j] == c + 1
    assert pop.x[n:2 * n].abs().sum() > 0 and not pop.x[:n].any()


# ---------------------------------------------------------------------------------------------------- C ABI
def test_explore_abi_layout_exports_and_refusals(tmp_path):
    """include/hockey_explore.h as the C compiler lays it out against the ctypes structs; the library exports the
    three entry points; hkl_explore refuses every malformed call on the host (no GPU: nothing is launched) with
    HKL_E_INVALID and a message that names it."""
    from hockey_amd import learner_hip as LH

    probes = {"ExploreMember": "hkl_explore_member", "ExploreIO": "hkl_explore_io"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hockey_learner.h"', "int main(void) {"]
    for py, cname in probes.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in getattr(LH, py)._fields_:
            lines.append(f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines += ['  printf("keys %llx %llx\\n", (unsigned long long)HKL_EXPLORE_KEY_NOISE, '
              '(unsigned long long)HKL_EXPLORE_KEY_RANDOM);', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    want = dict(line.split(None, 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for py, cname in probes.items():
        S = getattr(LH, py)
        assert ctypes.sizeof(S) == int(want[cname]), cname
        for f, _ in S._fields_:
            assert getattr(S, f).offset == int(want[f"{cname}.{f}"]), (cname, f)
    assert want["keys"].split() == [f"{X.KEY_NOISE:x}", f"{X.KEY_RANDOM:x}"]

    L = LH.lib()
    assert all(hasattr(L, name) for name in LH.EXPLORE_EXPORTS)
    assert L.hkl_explore_io_size() == ctypes.sizeof(LH.ExploreIO)

    def good(n_rows=40, rpm=20, **kw):
        io = LH.ExploreIO()
        for f, t in LH.ActIO._fields_:
            if t is ctypes.c_void_p:
                setattr(io.act, f, 256)
        for f, t in LH.ExploreIO._fields_:
            if t is ctypes.c_void_p:
                setattr(io, f, 256)
        io.act.n_policies, io.act.n_rows, io.act.obs_ld, io.act.out_ld, io.rows_per_member = 2, n_rows, 18, 8, rpm
        for k, v in kw.items():
            setattr(io.act if hasattr(io.act, k) else io, k, v)
        return io

    def members(n=2, **kw):
        ms = (LH.ExploreMember * 65)()
        for k, v in kw.items():
            setattr(ms[n - 1], k, v)
        return ms

    cases = [(None, members(), "null"), (good(n_policies=65), members(), "n_policies"),
             (good(obs_ld=17), members(), "obs_ld"), (good(out_ld=3), members(), "out_ld"),
             (good(counts=None), members(), "scratch"), (good(rpm=0), members(), "rows_per_member"),
             (good(rpm=-4), members(), "rows_per_member"), (good(n_rows=41), members(), "multiple"),
             (good(n_rows=0), members(), "multiple"), (good(n_rows=65, rpm=1), members(), "n_members"),
             (good(members=None), members(), "null"), (good(), None, "null"), (good(total=None), members(), "total"),
             (good(calls=None), members(), "calls"), (good(count=None), members(), "count"),
             (good(), members(anneal=3), "member 1: anneal"), (good(), members(noise=5), "member 1: noise"),
             (good(), members(noise=-1), "member 1: noise"), (good(x=None), members(noise=3), "member 1: null x"),
             (good(ext=None), members(noise=4), "member 1: null ext")]
    for io, ms, word in cases:
        assert L.hkl_tanh_probe(None, None, 0, None) == 1  # another entry point's message in between
        assert L.hkl_explore(None if io is None else ctypes.byref(io), ms, None) == 1, word
        msg = L.hkl_last_error().decode()
        assert msg.startswith("hkl_explore: ") and word in msg, (word, msg)


# ---------------------------------------------------------------------------------------------------- training
def _cfg(noise, **kw):
    base = dict(batch_size=32, use_self_play=False, curriculum_name="stage1", max_steps=30, start_steps=100,
                noise_mode=noise)
    base.update(kw)
    return TD3Config(**base)


def test_train_explore_device_on_host_build():
    """train(explore="device") on the kernel source's host build (the Explorer's torch backend), two rounds of 30
    steps x 8 arenas: the stored action is the applied one and lies in [-1, 1], the agent's total_steps is the
    arena-steps played, and its noise scale is noise_scale() of that count."""
    from hockey_amd.td3 import train
    from hostcheck import HostTorchEnv

    n, seen = 8, []
    env = HostTorchEnv(n, policies=("external", "external"))
    agent, st = train(n_arenas=n, rounds=2, cfg=_cfg("ornstein-uhlenbeck"), device="cpu", env=env, seed=5,
                      explore="device", updates_per_round=2, graphs=False,
                      on_step=lambda o, a, r, o2, d, res: seen.append((a.clone(), res.actions.clone())))
    assert len(seen) == 60
    for a, applied in seen:
        assert torch.equal(applied[:, :4], a) and a.abs().max() <= 1
    a0 = torch.stack([a for a, _ in seen])
    assert a0[:12].abs().max() > 0.9 and a0.std() > 0.1  # 100 random arena-steps: U(-1, 1) actions
    assert agent.total_steps == st["env_steps"] == st["replay_size"] == 2 * 30 * n
    assert agent.current_noise_scale == agent.noise_scale() < agent.cfg.action_noise_scale
    assert st["updates"] == 4 and all(torch.isfinite(p).all() for p in agent.actor.parameters())
    with pytest.raises(ValueError, match="explore"):
        train(n_arenas=n, rounds=1, cfg=_cfg("gaussian"), device="cpu", env=env, explore="gpu")


@pytest.mark.parametrize("episode_end", ["max_steps", "done"])
def test_train_population_explore_device_on_host_build(episode_end):
    """train_population(explore="device"), S = 3 (gaussian / pink / uniform) x 8 arenas, two rounds: per member the
    stored actions are the applied ones in [-1, 1], total_steps equals the stored rows (episode_end="done": only the
    running arenas count, on the device), and the noise scale follows the member's own count."""
    from hockey_amd.population import train_population
    from hostcheck import HostTorchEnv

    S, n = 3, 8
    steps = 30 if episode_end == "max_steps" else 120
    env = HostTorchEnv(S * n, policies=("external", "external"))
    seen = []
    members = [(_cfg(k, max_steps=steps, start_steps=40 * j), 3 + j) for j, k in enumerate(("gaussian", "pink", "uniform"))]
    agents, st = train_population(members, n_arenas=n, rounds=2, device="cpu", env=env, explore="device",
                                  updates_per_round=2, graphs=False, episode_end=episode_end,
                                  on_step=lambda m, ar, o, a, r, o2, d, res: seen.append(
                                      (m.clone(), ar.clone(), a.clone(), res.actions.clone())))
    for m, ar, a, applied in seen:
        assert torch.equal(applied[ar, :4], a) and a.abs().max() <= 1
    for j, ag in enumerate(agents):
        stored = sum(int((m == j).sum()) for m, _, _, _ in seen)
        assert ag.total_steps == st[j]["env_steps"] == st[j]["replay_size"] == stored
        if episode_end == "max_steps":
            assert stored == 2 * steps * n
        assert ag.current_noise_scale == ag.noise_scale() == st[j]["noise_scale"][-1]
        assert ag.noise_scale() < ag.cfg.action_noise_scale
    with pytest.raises(ValueError, match="explore"):
        train_population(members, n_arenas=n, rounds=1, device="cpu", env=env, explore="hip")
