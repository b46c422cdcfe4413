"""One lockstep harness for the step kernel's scene batches and games.  TEST INFRASTRUCTURE ONLY.

A scene batch (wave_zoo, toi_lean_zoo, wave_list_scenes, sleep_scenes, physics_scenes, physics_scenes2,
arena_copy_cases) or a game is driven through an IMPLEMENTATION and compared bit for bit with the oracle.  An
implementation has hostcheck.HostVec's call shapes, numpy in and numpy out:

    set_state(state, aux=None, mask=None)   reset_params(params, mask=None, max_t=None)   reset()
    step(actions, with_agent_two=..., debug=..., ...) -> namespace of numpy fields
    get_state() -> (state, aux)             counters()            close()
    paths: the launches it has ("hk_step"; "hk_rollout" where rollout(actions[K, n, 8], ...) exists)

HostVec (the kernel source's host build) is one, GpuVec (VecHockeyEnv on the MI355X) and OracleWorlds (a list of
OracleWorld: the oracle's debug rows and wrong variants) are the others.  Everything that drives one of them
through a batch and says where it left the oracle is here once; the test files hold the batches and what they expect.
"""
from types import SimpleNamespace

import numpy as np

from hockey_amd import _native as N
from hockey_amd.placement import np_random, placement
from vec_lockstep import FIELDS, first_mismatch

STEP_FIELDS = FIELDS[:7]  # the seven step outputs: obs, obs2, reward, reward2, done, info, info2
WORLD_FIELDS = STEP_FIELDS[:6]  # what an OracleWorld answers per step: all of them but info2
DEV = "cuda:0"


def require_gfx950():
    import torch

    assert torch.cuda.is_available(), "GPU tests need the MI355X (gfx950)"
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


# ------------------------------------------------------------------------------------------------ implementations
class GpuVec:
    """VecHockeyEnv on the GPU behind HostVec's call shapes.  `env` is the VecHockeyEnv, for the calls only it has
    (snapshot, restore, fork)."""

    paths = ("hk_step", "hk_rollout")

    def __init__(self, n, keep_mode=True, mode=0, auto_reset=False, vel_ref=False, policies=("external", "external"),
                 seed=0, arena_offset=0, diag_flags=0):
        import torch
        from hockey_amd.vec_env import VecHockeyEnv

        self.torch, self.n = torch, n
        self.env = VecHockeyEnv(n, keep_mode=keep_mode, mode=mode, device=DEV, policies=policies,
                                auto_reset=auto_reset, seed=seed, vel_ref_semantics=vel_ref,
                                arena_offset=arena_offset, diag_flags=diag_flags)
        self._dbg = None

    def _dev(self, a):
        """A device tensor of a's own copy: the batches' arrays are read-only and may be strided views."""
        return None if a is None else self.torch.as_tensor(np.array(a), device=DEV)

    @staticmethod
    def _np(res, t=None):
        have = {f: getattr(res, f) for f in res.__slots__ if getattr(res, f) is not None}
        return {f: (v if t is None else v[t]).cpu().numpy() for f, v in have.items()}

    def close(self):
        self.env.close()

    def reset(self):
        self.env.reset()

    def reset_params(self, params, mask=None, max_t=None):
        self.env.reset_params(self._dev(np.asarray(params, np.float32)), self._dev(mask), self._dev(max_t))

    def set_state(self, state, aux=None, mask=None):
        self.env.set_state(self._dev(state), self._dev(aux), self._dev(mask))

    def step(self, actions=None, debug=False, opp_inc=None, policy2=None, **kw):
        if debug and self._dbg is None:
            self._dbg = self.torch.zeros((self.n, N.DEBUG_DIM), dtype=self.torch.float32, device=DEV)
        res = self.env.step(self._dev(actions), opp_inc=self._dev(opp_inc), policy2=self._dev(policy2),
                            debug=self._dbg if debug else None, **kw)
        out = SimpleNamespace(**self._np(res))
        if debug:
            out.debug = self._dbg.cpu().numpy()
        return out

    def rollout(self, actions=None, n_steps=None, **kw):
        """One hk_rollout of len(actions) steps (n_steps where no player is external); the per-step dicts."""
        k = len(actions) if n_steps is None else n_steps
        res = self.env.rollout(k, actions=self._dev(actions), **kw)
        return [self._np(res, t) for t in range(k)]

    def get_state(self):
        st, aux = self.env.get_state()
        return st.cpu().numpy(), aux.cpu().numpy()

    def counters(self):
        return np.asarray(self.env.counters())

    def opponent_phase(self, new=None):
        return self.env.opponent_phase(self._dev(new)).cpu().numpy()


class OracleWorlds:
    """n OracleWorld arenas behind the same call shapes: the side that has debug rows and the wrong variants
    (oracle.set_variant is read when a world is created and at every step)."""

    paths = ("hk_step",)

    def __init__(self, oracle, n, keep_mode=True, mode=0):
        self.n = n
        self.ws = [oracle.OracleWorld(keep_mode, mode) for _ in range(n)]
        self.toi_events = 0

    def close(self):
        self.ws = []

    def reset_params(self, params, mask=None, max_t=None):
        for i, w in enumerate(self.ws):
            if mask is None or mask[i]:
                w.reset(params[i], max_t if np.ndim(max_t) == 0 else max_t[i])

    def set_state(self, state, aux=None, mask=None):
        for i, w in enumerate(self.ws):
            if mask is None or mask[i]:
                w.set_raw(state[i], w.get_raw()[1] if aux is None else aux[i])

    def observe(self):
        return np.stack([w.obs() for w in self.ws]), np.stack([w.obs_two() for w in self.ws])

    def step(self, actions, with_agent_two=False, debug=False):
        rows = []
        for w, a in zip(self.ws, actions):
            o, r, d, info, dbg = w.step(a)
            self.toi_events += w.stats()[1]
            row = [o, np.float32(r), np.uint8(d), info.astype(np.float32), dbg]
            if with_agent_two:
                row += [w.obs_two(), np.float32(w.info_two()[1])]
            rows.append(row)
        names = ("obs", "reward", "done", "info", "debug") + (("obs2", "reward2") if with_agent_two else ())
        return SimpleNamespace(**{f: np.stack([row[j] for row in rows]) for j, f in enumerate(names)})

    def get_state(self):
        raw = [w.get_raw() for w in self.ws]
        return np.stack([r[0] for r in raw]), np.stack([r[1] for r in raw])


def scene_env(make, state, aux, **kw):
    """make(n, **kw) with the rows of a scene batch put in place."""
    env = make(len(state), **kw)
    env.set_state(state, aux)
    return env


# ------------------------------------------------------------------------------------------------ the oracle's answer
def oracle_run(oracle, state, aux, actions, keep_mode=True, every_step_state=False, patch=None):
    """OracleVec through actions [K, n, 8] from (state, aux): {"steps": the K per-step output dicts, "state": the
    final (state, aux), "counters"}, all frozen read-only.  every_step_state: also "states" [K, n, 18] and "auxs"
    [K, n, 5] after every step.  patch(k, state) -> None or (state, mask): a masked set_state before step k; "patched"
    then maps k to the states before and after it."""
    ov = oracle.OracleVec(len(state), keep_mode=keep_mode, policies=("external", "external"), auto_reset=False)
    ov.set_state(state, aux)
    out = {"steps": [], "states": [], "auxs": [], "patched": {}}
    for k, a in enumerate(actions):
        before = ov.get_state()[0] if patch else None
        p = patch(k, before) if patch else None
        if p is not None:
            ov.set_state(p[0], None, p[1])
            out["patched"][k] = (before, ov.get_state()[0])
        out["steps"].append(ov.step(a, with_agent_two=True))
        if every_step_state:
            st, ax = ov.get_state()
            out["states"].append(st)
            out["auxs"].append(ax)
    out.update(state=ov.get_state(), counters=ov.counters())
    if every_step_state:
        out.update(states=np.stack(out["states"]), auxs=np.stack(out["auxs"]))
    ov.close()
    _freeze(out)
    return out


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _freeze(v)


# ------------------------------------------------------------------------------------------------ comparisons
def _rows(x, rows):
    return x if rows is None else x[rows]


def _arena(row, rows):
    return int(row) if rows is None else int(rows[row])


def check_step(t, got, want_t, how, rows=None, describe=None, fields=STEP_FIELDS):
    """Step t's outputs of a context that holds the batch's arenas `rows` (in that order; None: all of them) against
    the oracle's.  A failure names the batch's arena."""
    got = got if isinstance(got, dict) else vars(got)
    bad = first_mismatch(t, got, {f: _rows(want_t[f], rows) for f in fields}, fields=fields)
    if bad:
        ctx = ""
        if "arena" in bad:
            bad["row"], bad["arena"] = bad["arena"], _arena(bad["arena"], rows)
            ctx = "\n%s" % describe(bad["arena"], t) if describe else ""
        raise AssertionError("%s: step %d, arena %s: %s%s" % (how, t, bad.get("arena", "-"), bad, ctx))


def check_end(env, want, how, rows=None, describe=None, toi=None, large=None):
    """The context's final state words and aux rows against the oracle's, and the counters: 0 to 4 when the context
    holds the whole batch, no overflow, the TOI counter against the labels toi [n, K] of the rows held, the
    large-island counter against `large` (an int or a predicate)."""
    last = len(want["steps"]) - 1
    st, aux = env.get_state()
    ost, oaux = (_rows(x, rows) for x in want["state"])
    for what, g, w in (("state", st.view(np.uint32), ost.view(np.uint32)), ("aux row", aux, oaux)):
        ok = (g == w).all(1)
        if not ok.all():
            row = int(np.nonzero(~ok)[0][0])
            i = _arena(row, rows)
            raise AssertionError("%s: final %s (after step %d) of arena %d (row %d) differs\n%s\n%s%s" % (
                how, what, last, i, row, g[row], w[row], "\n%s" % describe(i, last) if describe else ""))
    c = np.asarray(env.counters()).astype(np.int64)
    assert c[N.CNT_OVERFLOW] == 0, (how, "overflow counter", c[N.CNT_OVERFLOW])
    if toi is not None:
        assert c[N.CNT_TOI] == _rows(toi, rows).sum(), (how, "TOI counter", c[N.CNT_TOI], _rows(toi, rows).sum())
    if large is not None:
        n = int(c[N.CNT_LARGE_ISLANDS])
        assert large(n) if callable(large) else n == large, (how, "large-island counter", n, large)
    if rows is None or len(rows) == len(want["state"][0]):  # the whole batch: every counter the oracle keeps
        assert np.array_equal(c[:5], want["counters"][:5]), (how, "counters", c[:8], want["counters"][:5])


def same_bits(got, want, what, label=None, first=0, ref="the oracle's"):
    """[K, n, ...] stacks: 4-byte words as uint32, everything else in its own dtype."""
    g, w = (a.view(np.uint32) if a.dtype.itemsize == 4 else a for a in (np.asarray(got), np.asarray(want)))
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    same = (g == w).reshape(g.shape[0], g.shape[1], -1).all(-1)
    if not same.all():
        k, i = (int(x[0]) for x in np.nonzero(~same))
        raise AssertionError("%s: step %d, arena %d%s: differs from %s\n%s\n%s" % (
            what, k + first, i, "" if label is None else " (%s)" % label[i], ref, got[k][i], want[k][i]))


def wave_permutation(n, seed=64):
    """The lanes of every wave of n arenas permuted (fixed seed): every arena keeps its wave."""
    rng = np.random.default_rng(seed)
    perm = np.concatenate([w0 + rng.permutation(min(64, n - w0)) for w0 in range(0, n, 64)])
    assert np.array_equal(np.sort(perm), np.arange(n)) and (perm // 64 == np.arange(n) // 64).all()
    return perm


def run_batch(env, actions, path):
    """actions [K, n, 8] through K hk_step launches or one hk_rollout; the K output dicts."""
    assert path in env.paths, (path, env.paths)
    if path == "hk_step":
        return [vars(env.step(a, with_agent_two=True)) for a in actions]
    return env.rollout(actions, with_agent_two=True)


def check_run(env, actions, path, want, how, rows=None, describe=None, **end):
    """run_batch, check_step on every step, check_end(**end); closes env.  actions: the batch's [K, n, 8]."""
    for t, got in enumerate(run_batch(env, actions if rows is None else actions[:, rows], path)):
        check_step(t, got, want["steps"][t], how, rows, describe)
    check_end(env, want, how, rows, describe, **end)
    env.close()


# ------------------------------------------------------------------------------------------------ games
def world_lockstep(make, oracle, mode, n, steps, seed, **env_kw):
    """make(n, keep_mode=, mode=, ...) against one OracleWorld per arena: PCG64 placements, U(-1, 1) joint actions,
    strong-vs-strong BasicOpponent actions on the even arenas (contacts, shots, goals).  Returns the first mismatch,
    or the oracle's TOI events and the implementation's counters."""
    env = make(n, keep_mode=True, mode=mode, **env_kw)
    params = np.zeros((n, 6), np.float32)
    for i in range(n):
        rng, _ = np_random(seed * 100_000 + i)
        params[i], max_t = placement(mode, bool(i % 2), rng)
    env.reset_params(params)
    ws = OracleWorlds(oracle, n, True, mode)
    ws.reset_params(params, max_t=max_t)
    rng = np.random.default_rng(seed)
    phases = rng.uniform(0, np.pi, (n, 2))
    obs, obs2 = (o.astype(np.float64) for o in ws.observe())
    for t in range(steps):
        acts = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        for i in range(0, n, 2):
            a1, phases[i, 0] = oracle.basic_opponent(0, 1, phases[i, 0], 0.1, obs[i])
            a2, phases[i, 1] = oracle.basic_opponent(0, 1, phases[i, 1], 0.1, obs2[i])
            acts[i] = np.concatenate([a1, a2]).astype(np.float32)
        got, want = vars(env.step(acts, with_agent_two=True)), vars(ws.step(acts, with_agent_two=True))
        bad = first_mismatch(t, got, want, fields=WORLD_FIELDS)
        if bad:
            return bad
        obs, obs2 = want["obs"].astype(np.float64), want["obs2"].astype(np.float64)
    assert np.array_equal(env.get_state()[0], ws.get_state()[0])
    out = {"n_toi": ws.toi_events, "counters": env.counters()}
    env.close()
    return out


def batched_lockstep(make, oracle, n, steps, mode, policies, seed, external=False, offset=0, mix=False, keep_mode=True,
                 vel_ref=False, diag_flags=0):
    """make(...) against the oracle's batched context on the hk_step contract: fused policies with Philox increments
    (opp_inc NULL), device auto-reset with episode counters.  external: U(-1.2, 1.2) joint actions (clipped in
    both).  mix: player 2's policy drawn per arena and step from {external, weak, strong} (hk_step_io.policy2).
    An implementation with hk_rollout takes the second half of the steps in one rollout (policy2 is hk_step's alone:
    a mixed run stays on hk_step).  Returns the first mismatch, or the counters."""
    kw = dict(keep_mode=keep_mode, mode=mode, policies=policies, auto_reset=True, seed=seed, arena_offset=offset,
              vel_ref=vel_ref)
    env, ov = make(n, diag_flags=diag_flags, **kw), oracle.OracleVec(n, **kw)
    rng = np.random.default_rng(seed)
    acts, p2 = [None] * steps, [None] * steps
    for t in range(steps):  # one stream: each step's actions, then its policy draw
        if external:
            acts[t] = rng.uniform(-1.2, 1.2, (n, 8)).astype(np.float32)
        if mix:
            p2[t] = rng.choice(np.array([0, 2, 3], np.uint8), n)
    half = steps // 2 if "hk_rollout" in env.paths and not mix else steps
    for t in range(half):
        got = vars(env.step(acts[t], with_agent_two=True, record_actions=True, final_obs=True, policy2=p2[t]))
        bad = first_mismatch(t, got, ov.step(acts[t], with_agent_two=True, final_obs=True, policy2=p2[t]))
        if bad:
            return bad
    if half < steps:
        ro = env.rollout(np.stack(acts[half:]) if external else None, n_steps=steps - half, with_agent_two=True,
                         record_actions=True, final_obs=True)
        for t in range(half, steps):
            bad = first_mismatch(t, ro[t - half], ov.step(acts[t], with_agent_two=True, final_obs=True))
            if bad:
                return bad
    st, aux = env.get_state()
    ost, oaux = ov.get_state()
    assert np.array_equal(st, ost) and np.array_equal(aux, oaux)
    if hasattr(env, "opponent_phase"):
        assert np.array_equal(env.opponent_phase(), ov.phase())
    c, oc = np.asarray(env.counters()).astype(np.int64), ov.counters()
    assert np.array_equal(c[:5], oc[:5]), (c[:7], oc[:7])  # steps, episodes, goals p1 / p2, TOI events
    env.close()
    ov.close()
    return {"counters": c}
