"""GPU tests of the drop-in surfaces: the gymnasium facades (Hockey-v0 / Hockey-One-v0) against the reference-
generated goldens and the oracle, the Q1 live-reference variant through the kernel, BeginContact scenarios, the
BASELINE C1 protocol, and the reference's own stage-3 actor under the reference's evaluation protocol.

Every facade value is compared exactly: obs as float64 of the kernel's float32, rewards and info in float64
(hk_info computes them in double like the reference)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hockey_amd import _native as N  # noqa: E402
from hockey_amd.placement import np_random, placement  # noqa: E402

INFO_KEYS = ("winner", "reward_closeness_to_puck", "reward_touch_puck", "reward_puck_direction")


def _vec(n, keep=True, mode=0, **kw):
    from hockey_amd.vec_env import VecHockeyEnv
    return VecHockeyEnv(n, keep_mode=keep, mode=mode, device="cuda:0", **kw)


def _np(t):
    return t.detach().cpu().numpy()


def _info_vec(d):
    return np.array([d[k] for k in INFO_KEYS], np.float64)


# ------------------------------------------------------------------------------------------------ goldens
def test_facade_g2_step_laws_exact(golden):
    """Hockey-v0 facade on every G2 case (keep_mode on and off, all modes): obs, obs_agent_two, float64 reward
    and info dicts, get_reward_agent_two(get_info_agent_two()), done, time -- equal to the reference's."""
    from hockey_amd.hockey_env import HockeyEnv

    g2 = golden("g2_step_presolve.npz")
    envs = {}
    bad = {}
    for i in range(len(g2["mode"])):
        keep, mode = bool(g2["keep_mode"][i]), int(g2["mode"][i])
        if (keep, mode) not in envs:
            e = HockeyEnv(keep_mode=keep, mode=mode)
            e._step_flags = N.STEP_SKIP_PHYSICS  # world.Step as a no-op, as in the golden harness
            envs[(keep, mode)] = e
        env = envs[(keep, mode)]
        env._vec.set_state(g2["state"][i][None, :], g2["aux"][i][None, :])
        env._refresh()
        act = g2["action"][i]
        a = act if keep else np.concatenate([act[0:3], act[4:7]])
        obs, r, d, trunc, info = env.step(a)
        k = 18 if keep else 16
        checks = {"obs": np.array_equal(obs, g2["obs"][i][:k]), "reward": r == g2["reward"][i],
                  "done": int(d) == g2["done"][i], "trunc": trunc is False,
                  "info": np.array_equal(_info_vec(info), g2["info"][i]),
                  "obs2": np.array_equal(env.obs_agent_two(), g2["obs2"][i][:k]),
                  "info2": np.array_equal(_info_vec(env.get_info_agent_two()), g2["info2"][i]),
                  "reward2": env.get_reward_agent_two(env.get_info_agent_two()) == g2["reward2"][i],
                  "reward_fn": env.get_reward(info) == g2["reward"][i],
                  "time": env.time == g2["has_after"][i][2],
                  "has": (env.player1_has_puck, env.player2_has_puck) == tuple(g2["has_after"][i][:2])}
        for f, ok in checks.items():
            if not ok:
                bad.setdefault(f, []).append(i)
    for e in envs.values():
        e.close()
    assert not bad, {k: v[:5] for k, v in bad.items()}


def test_kernel_g2r_live_reference_semantics(golden):
    """vel_ref_semantics=1 (SURVEY App. B Q1 "live reference") through the kernel == G2R bit for bit."""
    g2r = golden("g2r_step_presolve_live.npz")
    bad = {}
    for keep in (True, False):
        for mode in (0, 1, 2):
            idx = np.nonzero((g2r["keep_mode"] == int(keep)) & (g2r["mode"] == mode))[0]
            if len(idx) == 0:
                continue
            n = len(idx)
            env = _vec(n, keep=keep, mode=mode, vel_ref_semantics=True)
            env.reset_params(np.tile(np.array([8, 4, 3, 4, 0, 0], np.float32), (n, 1)))
            env.set_state(g2r["state"][idx], g2r["aux"][idx])
            dbg = torch.zeros((n, N.DEBUG_DIM), dtype=torch.float32, device="cuda:0")
            res = env.step(g2r["action"][idx], with_agent_two=True, debug=dbg, skip_physics=True)
            st, aux = env.get_state()
            i1, i2, r1, r2 = env.info()
            d = _np(dbg)
            got = {"force": d[:, 0:6].reshape(n, 3, 2), "torque": d[:, 6:8], "ldamp": d[:, 8:11],
                   "adamp": d[:, 11:13], "state_after": _np(st), "has_after": _np(aux)[:, 0:3],
                   "obs": _np(res.obs).astype(np.float64), "obs2": _np(res.obs2).astype(np.float64),
                   "done": _np(res.done).astype(np.int32), "info": _np(i1), "info2": _np(i2),
                   "reward": _np(r1), "reward2": _np(r2)}
            for f, v in got.items():
                ok = np.all(v.reshape(n, -1) == g2r[f][idx].reshape(n, -1), axis=1)
                if not ok.all():
                    bad.setdefault(f, []).extend(idx[~ok][:3].tolist())
            env.close()
    assert not bad, bad


def test_facade_set_state_g8(golden):
    """HockeyEnv.set_state through the facade: the bodies the reference's pybox2d setters leave, has_puck and
    the next observation (G8); the puck's angle and angular velocity stay untouched."""
    from hockey_amd.hockey_env import HockeyEnv

    g8 = golden("g8_set_state.npz")
    envs = {k: HockeyEnv(keep_mode=bool(k)) for k in (0, 1)}
    for i in range(len(g8["keep"])):
        keep = bool(g8["keep"][i])
        env = envs[int(keep)]
        env._vec.set_state(g8["raw_before"][i][None, :], np.zeros((1, 5), np.int32))
        env._refresh()
        env.set_state(g8["state"][i])
        st, _ = env._vec.get_state()
        assert np.array_equal(_np(st)[0], g8["raw_after"][i]), i
        k = 18 if keep else 16
        assert np.array_equal(env._get_obs(), g8["obs_after"][i][:k]), i
        if keep:
            assert (env.player1_has_puck, env.player2_has_puck) == tuple(g8["has_after"][i].astype(int)), i


# ------------------------------------------------------------------------------------------------ BeginContact
def test_begin_contact_scenarios(oracle):
    """Goal right / goal left / possession by player 1 and 2 (and a puck too fast for possession): set_state
    plus steps through the kernel, equal to the oracle, with the outcome ContactDetector.BeginContact
    prescribes (G7 pins that listener against the reference)."""
    base = np.array([2, 4, 0, 0, 0, 0, 8, 4, 0, 0, 0, 0, 5, 4, 0, 0, 0, 0], np.float32)
    scen = {  # puck x, y, vx -> expected (done, winner, has1, has2) after the first step
        "goal_right": ((9.25, 4.0, 0.0), (1, 1, 0, 0)), "goal_left": ((0.75, 4.0, 0.0), (1, -1, 0, 0)),
        "p1_catch": ((2.3, 4.0, 0.0), (0, 0, 15, 0)), "p2_catch": ((7.7, 4.0, 0.0), (0, 0, 0, 15)),
        "p1_too_fast": ((2.3, 4.0, 0.5), (0, 0, 0, 0)), "p2_too_fast": ((7.7, 4.0, -0.5), (0, 0, 0, 0))}
    n = len(scen)
    states = np.tile(base, (n, 1))
    for k, ((x, y, vx), _) in enumerate(scen.values()):
        states[k, 12:16] = [x, y, 0, vx]
    aux = np.zeros((n, 5), np.int32)
    env = _vec(n)
    env.reset_params(np.tile(np.array([8, 4, 5, 4, 0, 0], np.float32), (n, 1)))
    env.set_state(states, aux)
    ws = []
    for k in range(n):
        w = oracle.OracleWorld(True, 0)
        w.reset(np.array([8, 4, 5, 4, 0, 0], np.float32), 250)
        w.set_raw(states[k], aux[k])
        ws.append(w)
    zero = np.zeros((n, 8), np.float32)
    for t in range(3):
        res = env.step(zero)
        st, ax = env.get_state()
        for k, w in enumerate(ws):
            o, r, d, info, _ = w.step(zero[k])
            assert np.array_equal(_np(res.obs)[k], o) and bool(_np(res.done)[k]) == d, (t, k)
            wst, wax = w.get_raw()
            assert np.array_equal(_np(st)[k], wst) and np.array_equal(_np(ax)[k], wax), (t, k)
        if t == 0:
            a = _np(ax)
            for k, (name, (_, (dn, win, h1, h2))) in enumerate(scen.items()):
                assert (a[k, 3], a[k, 4], a[k, 0], a[k, 1]) == (dn, win, h1, h2), (name, a[k])
    env.close()


# ------------------------------------------------------------------------------------------------ facade runs
def test_facade_mode_switch_then_episode(oracle):
    """The reference's only working mode change is the setter (reset(mode=...) raises): after
    ``env.mode = 'TRAIN_DEFENSE'`` the next reset places a TRAIN_DEFENSE arena with max_timesteps 80, and the
    episode's info / reward / time limit use T = 80 (the kernel used to keep T = 250)."""
    from hockey_amd.hockey_env import HockeyEnv

    env = HockeyEnv()
    env.mode = "TRAIN_DEFENSE"
    obs, info = env.reset(seed=3)
    assert env.max_timesteps == 80
    rng, _ = np_random(3)
    params, max_t = placement(2, env.one_starts, rng)
    w = oracle.OracleWorld(True, 2)
    w.reset(params, max_t)
    assert np.array_equal(obs, w.obs().astype(np.float64))
    act = np.random.default_rng(5).uniform(-1, 1, (81, 8)).astype(np.float32)
    for t in range(81):
        obs, r, d, _, info = env.step(act[t])
        o, wr, wd, winfo, _ = w.step(act[t])
        assert np.array_equal(obs, o.astype(np.float64)) and r == wr and d == wd, t
        assert np.array_equal(_info_vec(info), winfo), t
        if t < 80 and not wd:
            assert not d
    assert d and env.time == 81
    env.close()


def test_c1_protocol_facade_vs_oracle(oracle):
    """BASELINE C1 through the Hockey-v0 facade: BasicOpponent(weak) from hockey_amd (host, global
    np.random phase stream) vs U(-1,1) from default_rng(0), reset(seed=episode) on done, 10 000 steps -- the
    observation sequence equals the oracle's run of the same protocol."""
    from hockey_amd.hockey_env import BasicOpponent, HockeyEnv

    steps = 10_000
    np.random.seed(0)
    p1 = BasicOpponent(weak=True)
    p2 = np.random.default_rng(0).uniform(-1, 1, (steps, 4))
    env = HockeyEnv()
    ep = 0
    obs, _ = env.reset(seed=ep)
    got = np.zeros((steps, 18))
    for t in range(steps):
        a = np.hstack([p1.act(obs), p2[t]])
        obs, r, d, _, info = env.step(a)
        got[t] = obs
        if d:
            ep += 1
            obs, _ = env.reset(seed=ep)
    env.close()
    legacy = np.random.RandomState(0)
    phase0 = legacy.uniform(0, np.pi)
    inc = legacy.uniform(0, 0.2, steps)
    params, one = [], True
    for e in range(ep + 1):
        one = not one
        rng, _ = np_random(e)
        params.append(placement(0, one, rng)[0])
    want, _, n_ep, _ = oracle.run_c1(p2.astype(np.float32), inc, phase0, np.stack(params))
    assert n_ep == ep + 1
    bad = np.nonzero(~np.all(got == want.astype(np.float64), axis=1))[0]
    assert len(bad) == 0, (int(bad[0]), got[bad[0]], want[bad[0]])
    assert ep >= 20


def test_hockey_one_seeded_run_vs_oracle(oracle):
    """Hockey-One-v0 reproduces a seeded reference run: the fused opponent takes the global np.random phase
    stream of the reference's BasicOpponent (init U(0, pi), U(0, 0.2) per act), so with np.random.seed(s) the
    facade equals the oracle driven by the same stream -- obs, float64 reward and info, done."""
    from hockey_amd.hockey_env import HockeyEnv_BasicOpponent

    np.random.seed(5)
    env = HockeyEnv_BasicOpponent(weak_opponent=False)
    legacy = np.random.RandomState(5)
    phase = legacy.uniform(0, np.pi)
    assert env.opponent.phase == phase
    seed = 11
    obs, _ = env.reset(seed=seed)
    rng, _ = np_random(seed)
    params, max_t = placement(0, env.one_starts, rng)
    w = oracle.OracleWorld(True, 0)
    w.reset(params, max_t)
    acts = np.random.default_rng(1).uniform(-1, 1, (600, 4))
    episodes = 0
    for t in range(600):
        inc = legacy.uniform(0, 0.2)
        a2, phase = oracle.basic_opponent(0, 1, phase, inc, w.obs_two().astype(np.float64))
        obs, r, d, _, info = env.step(acts[t])
        o, wr, wd, winfo, _ = w.step(np.concatenate([np.clip(acts[t], -1, 1), a2]).astype(np.float32))
        assert np.array_equal(obs, o.astype(np.float64)) and r == wr and d == wd, t
        assert np.array_equal(_info_vec(info), winfo), t
        if d:
            episodes += 1
            seed += 1
            obs, _ = env.reset(seed=seed)
            rng, _ = np_random(seed)
            params, max_t = placement(0, env.one_starts, rng)
            w.reset(params, max_t)
    assert episodes >= 2
    assert env.opponent.phase == phase
    env.close()


@pytest.mark.parametrize("staged,server", [("0", "1"), ("0", "0"), ("1", "0")])
def test_step_host_on_fresh_contexts_equals_hk_step(monkeypatch, staged, server):
    """hk_step_host (the facade's one-call step: the resident step server by default, one launch per step with a
    mapped completion word under HK_STEP_HOST_SERVER=0, or HK_STEP_HOST_STAGED=1 copies) on freshly created and
    destroyed single-arena contexts -- recycled pinned blocks included -- returns exactly what hk_step returns on a
    twin context built the same way: obs, obs2, done and the float64 step record, from the very first step on."""
    from hockey_amd.hockey_env import HockeyEnv

    monkeypatch.setenv("HK_STEP_HOST_STAGED", staged)
    monkeypatch.setenv("HK_STEP_HOST_SERVER", server)
    rng = np.random.default_rng(int(staged) + 2 * int(server))
    for k in range(6):
        host, twin = HockeyEnv(), HockeyEnv()
        host.reset(seed=100 + k)
        twin.reset(seed=100 + k)
        for t in range(1 + k):
            a = rng.uniform(-1, 1, 8).astype(np.float32)
            obs, r, d, _, info = host.step(a)
            res = twin._vec.step(a[None, :], with_agent_two=True, record=True)
            assert np.array_equal(obs, _np(res.obs)[0].astype(np.float64)), (k, t)
            assert np.array_equal(host.obs_agent_two(), _np(res.obs2)[0].astype(np.float64)), (k, t)
            assert bool(d) == bool(_np(res.done)[0]), (k, t)
            assert np.array_equal(host._out_f, _np(res.record)[0]), (k, t)
        host.close()
        twin.close()


def test_step_server_survives_idle_gaps_and_interleaved_calls(monkeypatch):
    """The resident step server (hk_kernels.h HostServer) against the launch-per-step path on a twin facade: the
    same actions through episodes with resets, set_state / get_state / observe calls between steps (each stops the
    server first), pauses past the server's idle limit (it exits; the next step starts another) and a
    kernel-counter read: every step's obs, obs2, record and the counters agree bit for bit."""
    import time

    from hockey_amd.hockey_env import HockeyEnv_BasicOpponent

    envs = {}
    for server in ("1", "0"):
        monkeypatch.setenv("HK_STEP_HOST_SERVER", server)
        np.random.seed(7)
        envs[server] = HockeyEnv_BasicOpponent()
    rng = np.random.default_rng(3)
    np.random.seed(11)
    st = np.random.get_state()
    for ep in range(3):
        for server, env in envs.items():
            np.random.set_state(st)
            env.reset(seed=40 + ep)
        for t in range(60):
            a = rng.uniform(-1, 1, 4)
            res = {}
            for server, env in envs.items():
                np.random.set_state(st)
                res[server] = env.step(a)
            st = np.random.get_state()
            o1, o0 = res["1"], res["0"]
            assert np.array_equal(o1[0], o0[0]) and o1[1] == o0[1] and o1[2] == o0[2] and o1[4] == o0[4], (ep, t)
            assert np.array_equal(envs["1"]._out_np, envs["0"]._out_np), (ep, t)
            if t == 20:
                time.sleep(0.05)  # past the server's idle limit (hk_host_step.cpp kSrvIdleMs)
            if t == 30:
                for env in envs.values():
                    env._vec.get_state()  # a device call between steps
                    env.set_state(o1[0])  # the state the last obs describes, on both twins
            if o1[2]:
                break
    c = [env._vec.counters() for env in envs.values()]
    assert np.array_equal(c[0], c[1]), c
    for env in envs.values():
        env.close()


def test_round_robin_facades_share_one_step_server():
    """Five facades stepped round-robin (a SyncVectorEnv of Hockey-One-v0 is this) plus torch work between rounds
    (ADVICE r04): at most one resident step server per device hands over between contexts, so no step waits for
    another context's idle server (the failure mode: ~20 ms per step).  Every facade returns exactly what a twin
    on the launch-per-step path returns, and the mean step time stays within 0.5 ms."""
    import os
    import time

    from hockey_amd.hockey_env import HockeyEnv

    envs = [HockeyEnv() for _ in range(5)]
    twins = [HockeyEnv() for _ in range(5)]
    for k, (e, t) in enumerate(zip(envs, twins)):
        e.reset(seed=70 + k)
        t.reset(seed=70 + k)
    rng = np.random.default_rng(5)
    acts = rng.uniform(-1, 1, (60, 5, 8)).astype(np.float32)
    x = torch.ones(256, 256, device="cuda:0")
    step_s = []
    for t in range(60):
        for k in range(5):
            if t == 0:  # a context picks its step path at its first hk_step_host call
                os.environ["HK_STEP_HOST_SERVER"] = "0"
                try:
                    o2, r2, d2, _, info2 = twins[k].step(acts[t, k])
                finally:
                    del os.environ["HK_STEP_HOST_SERVER"]
            else:
                o2, r2, d2, _, info2 = twins[k].step(acts[t, k])
            t0 = time.perf_counter()
            o, r, d, _, info = envs[k].step(acts[t, k])
            step_s.append(time.perf_counter() - t0)
            assert np.array_equal(o, o2) and r == r2 and d == d2 and info == info2, (t, k)
        x = torch.tanh(x @ x) * 0.01  # torch work on the current stream between rounds
    torch.cuda.synchronize()
    mean_ms = 1e3 * float(np.mean(step_s[5:]))
    print(f"round-robin facade step: mean {mean_ms:.3f} ms, p99 {1e3 * np.percentile(step_s[5:], 99):.3f} ms")
    # the bit-exact checks above are the gate; the timing bound only catches the r04 failure mode (a kernel queued
    # behind another context's idle server: ~20 ms per step), loose enough for a slow or loaded box
    assert mean_ms < 5.0, mean_ms
    for e in envs + twins:
        e.close()


def test_blocked_caller_stream_times_out_without_wedging_other_facades(monkeypatch):
    """Every wait on the step server is bounded, every time.  With HK_STEP_HOST_WAIT_MS = 40 and the
    current stream occupied by self-ending work ten times that long (capped at 0.5 s), facade A's step cannot be
    served (its server is ordered after that stream): it fails with HK_E_DEVICE within a small multiple of the limit,
    and so do a second step and a reset of A.  Facade B then steps successfully on a stream of its own while A's
    stream is still busy.  B's step is what the code before this test could not do: after A's time-out A's server
    stayed recorded as running and as the device slot's owner, so B's hand-over called an unbounded
    hipStreamSynchronize on the server stream under the device lock and waited out A's stream.
    After a device synchronise A is usable again: reset brings it back, its next steps equal a twin on the
    launch-per-step path bit for bit, its step counter shows 0 or 1 steps from the withdrawn request (0: the
    abandoned server started after the quit word was posted and left without stepping; 1: a server took the request
    while it was being withdrawn, the case include/hockey.h documents), and both contexts close with HK_OK."""
    import time

    from hockey_amd.hockey_env import HockeyEnv

    limit_s, E_DEVICE = 0.040, -4
    bound_s = 5 * limit_s
    monkeypatch.setenv("HK_STEP_HOST_WAIT_MS", str(int(limit_s * 1e3)))
    monkeypatch.delenv("HK_STEP_HOST_SERVER", raising=False)
    monkeypatch.delenv("HK_STEP_HOST_STAGED", raising=False)
    a, b = HockeyEnv(), HockeyEnv()
    L = a._vec.L
    zero = np.zeros(8, np.float32)
    b.step(zero)  # both contexts have their buffers, and B's server holds the device's slot
    a.step(zero)
    a.reset(seed=5)  # stops A's server: its next step has to start one
    steps0 = int(a._vec.counters()[N.CNT_STEPS])

    def timed(call):
        t0 = time.perf_counter()
        rc = call()
        return rc, time.perf_counter() - t0

    def raw_step(env):
        act_p, _, out_p = env._host_ptrs
        return L.hk_step_host(env._vec._ctx, act_p, None, 0, out_p, env._vec._stream())

    torch.cuda._sleep(100_000)  # warm-up, then cycles per second from a short measured run
    torch.cuda.synchronize()
    probe = 2_000_000
    _, probe_s = timed(lambda: (torch.cuda._sleep(probe), torch.cuda.synchronize()))
    block_s = min(10 * limit_s, 0.5)
    torch.cuda._sleep(int(probe * block_s / probe_s))  # the current stream is busy for about block_s

    rc, dt = timed(lambda: raw_step(a))
    assert rc == E_DEVICE and b"wait limit" in L.hk_last_error() and dt < bound_s, (rc, dt, L.hk_last_error())
    rc, dt = timed(lambda: raw_step(a))
    assert rc == E_DEVICE and b"wait limit" in L.hk_last_error() and dt < bound_s, (rc, dt, L.hk_last_error())
    rc, dt = timed(lambda: L.hk_reset(a._vec._ctx, None, None, None, None, a._vec._stream()))
    assert rc == E_DEVICE and b"wait limit" in L.hk_last_error() and dt < bound_s, (rc, dt, L.hk_last_error())
    with torch.cuda.stream(torch.cuda.Stream()):
        rc, dt = timed(lambda: raw_step(b))
    still_blocked = not torch.cuda.current_stream().query()
    print(f"blocked stream: probe {probe_s * 1e3:.1f} ms, B's step rc {rc} in {dt * 1e3:.2f} ms, "
          f"A's stream still busy {still_blocked}")
    assert rc == 0 and dt < bound_s, (rc, dt, L.hk_last_error())
    assert still_blocked, "the filler ended before B stepped: the case was not exercised"

    torch.cuda.synchronize()
    extra = int(a._vec.counters()[N.CNT_STEPS]) - steps0
    assert extra in (0, 1), extra
    monkeypatch.setenv("HK_STEP_HOST_SERVER", "0")  # a context picks its step path at its first hk_step_host call
    twin = HockeyEnv()
    a.reset(one_starting=True, seed=9)  # explicit: a facade's own resets alternate the starting side
    twin.reset(one_starting=True, seed=9)
    rng = np.random.default_rng(9)
    for t in range(5):
        act = rng.uniform(-1, 1, 8).astype(np.float32)
        o, r, d, _, info = a.step(act)
        o2, r2, d2, _, info2 = twin.step(act)
        assert np.array_equal(o, o2) and r == r2 and d == d2 and info == info2, t
        assert np.array_equal(a._out_np, twin._out_np), t
    torch.cuda.synchronize()
    for env in (a, b, twin):
        assert L.hk_destroy(env._vec._ctx) == 0, L.hk_last_error()
        env._vec._ctx = None


def test_keep_mode_step_returns_an_independent_obs():
    """the float64 obs step() returns is the caller's; changing it in place leaves env._get_obs()
    alone (the reference builds a fresh array per call)."""
    from hockey_amd.hockey_env import HockeyEnv

    env = HockeyEnv()
    env.reset(seed=3)
    o, *_ = env.step(np.zeros(8, np.float32))
    keep = env._get_obs().copy()
    o *= 0.0
    assert np.array_equal(env._get_obs(), keep) and not np.array_equal(o, keep)
    env.close()


# ------------------------------------------------------------------------------------------------ behaviour
def test_stage3_actor_reproduces_recorded_win_rates(golden):
    """The reference's stage-3 best actor (pretrained/stage_3/models/td3_best.pt, extracted weights-only into
    tests/golden/stage3_actor.npz) under the reference's evaluation protocol (rl/utils/evaluator.py:10-35:
    Hockey-One-v0, reset seeds 42..141, greedy actions): win rates within 3 binomial standard errors of the
    recorded WR_strong / WR_weak (metrics.json eval 53).  The GPU arenas restate Box2D (parity unpinned per
    trajectory) and draw the opponent phase per arena: this is the behavioural pin."""
    from hockey_amd.evaluate import Actor, evaluate

    z = golden("stage3_actor.npz")
    actor = Actor().to("cuda:0")
    with torch.no_grad():
        for name, p in actor.named_parameters():
            p.copy_(torch.from_numpy(z[name.replace(".", "_")]))
    actor.eval()
    n = int(z["eval_episodes"])
    for weak, rec in ((False, float(z["wr_strong"])), (True, float(z["wr_weak"]))):
        r = evaluate(actor, episodes=n, seed=int(z["eval_seed"]), weak_opponent=weak)
        big = evaluate(actor, episodes=4000, seed=int(z["eval_seed"]), weak_opponent=weak)
        p = big["win"]
        se = np.sqrt(max(p * (1 - p), 0.01 * 0.99) / n)  # the recorded rate is itself a 100-episode estimate
        print(f"stage3 actor vs {'weak' if weak else 'strong'}: WR {r['win']:.3f} (100 eps), {p:.4f} (4000 eps), "
              f"recorded {rec}")
        assert abs(rec - p) <= 3 * se, (weak, rec, p, r)


@pytest.mark.gpu
def test_raw_stream_matches_public_current_stream():
    """vec_env._raw_stream (torch's private raw-stream accessor) equals the public current stream's handle, on the
    default stream and inside a torch.cuda.stream context."""
    from hockey_amd.vec_env import _raw_stream

    dev = torch.cuda.current_device()
    assert _raw_stream(dev) == torch.cuda.current_stream(dev).cuda_stream
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        assert _raw_stream(dev) == st.cuda_stream == torch.cuda.current_stream(dev).cuda_stream
    assert _raw_stream(dev) == torch.cuda.current_stream(dev).cuda_stream
