"""Exact arena snapshots, restore and fork on the GPU: hk_snapshot / hk_restore / hk_copy_arenas (the gfx950 copy
kernel of hk_arena_copy.hip) through VecHockeyEnv, HockeyEnv and Lookahead, against the oracle -- which is never
snapshotted: it runs every history uninterrupted.  Every comparison is at tolerance zero unless stated.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hockey_amd import _native as N  # noqa: E402
from arena_copy_cases import N_ARENAS, fork_follows_the_oracle, interrupted, lookahead_case, no_bad_index  # noqa: E402
from arena_copy_cases import scen, want  # noqa: E402,F401  (module-scoped fixtures: the scenarios, the oracle's run)
from scene_lockstep import DEV, STEP_FIELDS, GpuVec, require_gfx950, run_batch, scene_env  # noqa: E402
from vec_lockstep import first_mismatch  # noqa: E402

HK_E_INVALID = -1


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gfx950()


def _vec(n, **kw):
    """The VecHockeyEnv itself, for the tests of its torch-level calls."""
    from hockey_amd.vec_env import VecHockeyEnv

    kw.setdefault("policies", ("external", "external"))
    return VecHockeyEnv(n, device=DEV, **kw)


def _t(a):
    return torch.as_tensor(a, device=DEV)


def _zoo_env(scen):  # noqa: F811
    """GpuVec with the scenarios in place; its .env is the VecHockeyEnv."""
    return scene_env(GpuVec, scen["state"], scen["aux"])


@pytest.mark.parametrize("how", ["step", "rollout"])
def test_resume_from_snapshot_equals_uninterrupted_oracle(scen, want, how):  # noqa: F811
    """(5.1) snapshot -> every arena reset and stepped -> restore -> the oracle's uninterrupted trajectory."""
    ok = interrupted(_zoo_env(scen), scen, want, "hk_" + how, lambda g: g.env.snapshot(),
                     lambda g, s: g.env.restore(s))
    assert ok.all(), "arenas %s left the oracle's trajectory after restore" % np.nonzero(~ok)[0].tolist()


def test_resume_from_get_state_is_not_exact(scen, want):  # noqa: F811
    """The power of (5.1) on the device: get_state / set_state alone does not resume these scenarios."""
    ok = interrupted(_zoo_env(scen), scen, want, "hk_step", lambda g: g.get_state(), lambda g, s: g.set_state(*s))
    assert not ok.all()


@pytest.mark.parametrize("how", ["step", "rollout"])
def test_fork_to_other_indices_follows_the_oracle(oracle, how):
    """(5.3) arena_copy_cases.fork_follows_the_oracle with VecHockeyEnv.fork (hk_copy_arenas) as the fork."""
    fork_follows_the_oracle(oracle, GpuVec(128), "hk_" + how, lambda g, src, dst: g.env.fork(src, dst))


def test_same_index_resume_with_device_draws(oracle):
    """(6) strong-vs-strong fused bots, Philox phase increments, auto-reset; time limits of 12..28 steps so resets
    (device placement draws) fall before and after the snapshot at step 20.  Both continuations of 20 steps equal
    each other and the oracle's uninterrupted 40 steps: a restore to the same index continues the same streams."""
    n, seed = N_ARENAS, 4242
    mt = (12 + np.arange(n) % 17).astype(np.int32)
    ov = oracle.OracleVec(n, policies=("strong", "strong"), auto_reset=True, seed=seed)
    ov.reset(max_t=mt)
    wantrun = [ov.step(with_agent_two=True, final_obs=True) for _ in range(40)]
    dones = np.stack([w["done"] for w in wantrun])
    assert dones[:20].any() and dones[20:].any(), "resets occur on both sides of the snapshot"
    g = GpuVec(n, policies=("strong", "strong"), auto_reset=True, seed=seed)
    env = g.env
    mt_t = _t(mt)
    N.check(env.L.hk_reset(env._ctx, None, None, N.ptr(mt_t), None, env._stream()), "hk_reset")
    fields = STEP_FIELDS + ("final_obs",)

    def run(t0):
        out = []
        for t in range(t0, t0 + 20):
            got = vars(g.step(None, with_agent_two=True, final_obs=True))
            bad = first_mismatch(t, got, wantrun[t], fields=fields)
            assert bad is None, bad
            out.append(got)
        return out

    run(0)
    snap = env.snapshot()
    first = run(20)
    end_state = g.get_state()
    env.restore(snap)
    second = run(20)
    for a, b in zip(first, second):
        for f in fields:
            assert np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8)), f
    st, aux = g.get_state()
    assert np.array_equal(st.view(np.uint32), end_state[0].view(np.uint32)) and np.array_equal(aux, end_state[1])
    no_bad_index(g)
    g.close()
    ov.close()


def test_lift_one_arena_into_a_one_arena_context(scen):  # noqa: F811
    """(7) arena 77 of a 101-arena context, lifted into a one-arena context, steps like its source."""
    env = _zoo_env(scen)
    run_batch(env, scen["actions"][:2], "hk_step")
    one = GpuVec(1)
    one.env.fork([77], [0], source=env.env)
    rng = np.random.default_rng(77)
    for t in range(5):
        a = rng.uniform(-1, 1, (N_ARENAS, 8)).astype(np.float32)
        g = vars(env.step(a, with_agent_two=True))
        h = vars(one.step(a[77:78], with_agent_two=True))
        for f in STEP_FIELDS:
            assert np.array_equal(g[f][77:78].view(np.uint8), h[f].view(np.uint8)), (t, f)
    assert torch.equal(env.env.snapshot([77]).blob, one.env.snapshot().blob)
    (s0, x0), (s1, x1) = env.get_state(), one.get_state()
    assert np.array_equal(s0[77:78].view(np.uint32), s1.view(np.uint32)) and np.array_equal(x0[77:78], x1)
    no_bad_index(env, one)
    env.close()
    one.close()


def test_facade_snapshot_restore_around_the_step_server(scen):  # noqa: F811
    """(7) HockeyEnv.snapshot / restore between hk_step_host steps: the resident server is stopped for the copy and
    restarted by the next step, and the continuation repeats bit for bit.  Then the facade takes arena 77 of a batch."""
    from hockey_amd.hockey_env import HockeyEnv

    h = HockeyEnv()
    h.reset(seed=11)
    rng = np.random.default_rng(5)
    acts = rng.uniform(-1, 1, (12, 8))
    for t in range(4):
        h.step(acts[t])
    snap = h.snapshot()

    def cont():
        out = []
        for t in range(4, 12):
            o, r, d, _, info = h.step(acts[t])
            out.append((o.tobytes(), r, d, tuple(sorted(info.items())), h.obs_agent_two().tobytes()))
        return out

    first = cont()
    h.restore(snap)
    assert h.time == 4
    assert cont() == first
    env = _zoo_env(scen)
    run_batch(env, scen["actions"][:2], "hk_step")
    h.restore(env.env.snapshot([77]))
    a = scen["actions"][2]
    g = vars(env.step(a, with_agent_two=True))
    o, r, d, _, info = h.step(a[77])
    assert np.array_equal(o, g["obs"][77].astype(np.float64)) and np.float32(r) == g["reward"][77]
    assert bool(d) == bool(g["done"][77])
    with pytest.raises(ValueError):
        h.restore(env.env.snapshot([1, 2]))
    h.close()
    env.close()
    # the fused opponent's phase travels with the arena, and its host mirror follows a restore
    from hockey_amd.hockey_env import HockeyEnv_BasicOpponent

    hb = HockeyEnv_BasicOpponent()
    hb.reset(seed=3)
    for t in range(3):
        hb.step(acts[t][:4])
    snap, phase = hb.snapshot(), hb.opponent.phase
    for t in range(3, 5):
        hb.step(acts[t][:4])
    assert hb.opponent.phase != phase
    hb.restore(snap)
    assert hb.opponent.phase == phase and hb.time == 3
    hb.close()


def test_copy_between_keep_modes_is_invalid():
    a, b = _vec(4, keep_mode=True), _vec(4, keep_mode=False)
    before = b.snapshot().blob.clone()
    rc = a.L.hk_copy_arenas(b._ctx, None, a._ctx, None, 4, a._stream())
    assert rc == HK_E_INVALID and b"keep_mode" in a.L.hk_last_error()
    with pytest.raises(N.HockeyNativeError):
        b.fork([0], [1], source=a)
    with pytest.raises(N.HockeyNativeError):
        b.restore(a.snapshot())
    assert torch.equal(b.snapshot().blob, before)
    with pytest.raises(ValueError, match="duplicate"):
        a.fork([0, 1], [2, 2])
    with pytest.raises(ValueError, match="also a source"):
        a.fork([0, 1], [1, 2])
    with pytest.raises(ValueError, match="out of range"):
        a.fork([0], [4])
    no_bad_index(a, b)
    a.close()
    b.close()


def test_out_of_range_entries_are_counted_on_the_device(scen):  # noqa: F811
    """With assume_valid the kernel's own check stands: bad entries copy nothing and are counted, exactly."""
    env = _zoo_env(scen).env
    dst = _vec(130)
    before = dst.snapshot().blob.clone()
    idx = torch.arange(130, device=DEV)
    src = idx.clone()  # sources 101..129 do not exist: 29 bad entries, spread over three workgroups
    dst.fork(src, idx, source=env, assume_valid=True)
    assert dst.counters()[N.CNT_BAD_INDEX] == 29 and env.counters()[N.CNT_BAD_INDEX] == 0
    assert torch.equal(dst.snapshot(list(range(N_ARENAS))).blob, env.snapshot().blob)
    keep = list(range(N_ARENAS, 130))
    fresh = _vec(130)
    assert torch.equal(dst.snapshot(keep).blob, fresh.snapshot(keep).blob)
    assert before.numel() == dst.snapshot().blob.numel()
    for e in (env, dst, fresh):
        e.close()


def test_fork_replays_from_a_graph(scen):  # noqa: F811
    """(8) a fork recorded in a torch.cuda.graph (a single branch) and replayed gives the eager call's arenas."""
    zoo = _zoo_env(scen)
    run_batch(zoo, scen["actions"][:2], "hk_step")
    env, dst = zoo.env, _vec(128)
    g = torch.Generator().manual_seed(3)
    d_idx = torch.randperm(128, generator=g)[:90].to(DEV)
    s_idx = torch.randint(0, N_ARENAS, (90,), generator=g).to(DEV)
    dst.fork(s_idx, d_idx, source=env)  # eager, checked
    eager = dst.snapshot(d_idx).blob.clone()
    dst.reset()
    assert not torch.equal(dst.snapshot(d_idx).blob, eager)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dst.fork(s_idx, d_idx, source=env, assume_valid=True)
    dst.reset()
    graph.replay()
    assert torch.equal(dst.snapshot(d_idx).blob, eager)
    no_bad_index(env, dst)
    env.close()
    dst.close()


def test_lookahead_against_an_oracle_batch(oracle):
    """(9) M = 5 sources, K = 8 branches, H = 6 steps, player 2 a fused weak bot with given phase increments, against
    the oracle batch of arena_copy_cases.lookahead_case (40 arenas with duplicated histories).  Source 1 scores
    inside the horizon: the kernel repeats the sticky -10, and it enters each return once."""
    from hockey_amd.lookahead import Lookahead

    c = lookahead_case(oracle)
    M, K, H, hist, pol = c["M"], c["K"], c["H"], c["hist"], c["policies"]
    env = _vec(c["n_live"], policies=pol)
    env.reset_params(c["params"], max_t=c["max_t"])
    env.opponent_phase(c["phase"])
    for t in range(hist):
        env.step(_t(c["h_act"][t]), opp_inc=_t(c["h_inc"][t]))
    live_before = env.snapshot().blob.clone()
    st_before = [x.clone() for x in env.get_state()]

    gamma = 0.97
    la = Lookahead(env, branches=K, horizon=H, gamma=gamma, max_sources=M, policies=pol)
    out = la.evaluate(c["src"], c["acts"], opp_inc=c["incs"])
    rew, done = out.rewards.cpu().numpy(), out.dones.cpu().numpy()
    w_rew, w_done, w_win = c["rewards"], c["dones"], c["winner"]
    assert rew.shape == (H, M, K) and done.shape == (H, M, K) and out.winner.shape == (M, K)
    assert np.array_equal(rew.reshape(H, -1).view(np.uint32), w_rew.view(np.uint32))
    assert np.array_equal(done.reshape(H, -1), w_done)
    assert np.array_equal(out.winner.cpu().numpy().reshape(-1), w_win)
    # returns: the float64 sum of the float32 rewards up to and including the first done step, within the bound
    # of H float32 additions
    ret = out.returns.cpu().numpy().astype(np.float64).reshape(-1)
    r64 = w_rew.astype(np.float64)
    for b in range(M * K):
        t_end = int(np.argmax(w_done[:, b])) if w_done[:, b].any() else H - 1
        terms = r64[:t_end + 1, b] * gamma ** np.arange(t_end + 1)
        bound = H * 2.0 ** -23 * np.abs(terms).sum()
        print("branch %d: return %.9g reference %.9g bound %.3g" % (b, ret[b], terms.sum(), bound))
        assert abs(ret[b] - terms.sum()) <= bound, b
    # the scoring source: done inside the horizon with steps to spare, the sticky -10 repeated by the kernel but
    # counted once
    sc = slice(K, 2 * K)
    t0 = np.argmax(w_done[:, sc], axis=0)
    assert w_done[:, sc].any(0).all() and (t0 <= H - 2).all() and (w_win[sc] == -1).all()
    assert (w_rew[-1, sc] < -9).all() and (w_rew[t0, np.arange(K) + K] < -9).all()
    naive = (r64[:, sc] * (gamma ** np.arange(H))[:, None]).sum(0)
    assert (ret[sc] - naive > 8).all(), "a repeated terminal reward was counted"
    assert (ret[sc] < -10 * gamma ** (H - 1)).all() and (ret[sc] > -11).all()
    # the live env is untouched
    st, aux = env.get_state()
    assert torch.equal(st.view(torch.int32), st_before[0].view(torch.int32)) and torch.equal(aux, st_before[1])
    assert torch.equal(env.snapshot().blob, live_before)
    assert env.counters()[N.CNT_STEPS] == hist * c["n_live"]
    no_bad_index(env, la.ws)
    la.close()
    env.close()
