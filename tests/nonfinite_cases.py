"""Scenarios that feed values which are not finite numbers into the step (include/hockey.h, "Non-finite values").

Test infrastructure only.  tests/test_nonfinite.py runs them on the kernel source's host build and the oracle,
tests/test_gpu_nonfinite.py runs the action and increment scenarios on gfx950; tests/sanitize/sanitize_main.cpp
restates them in C++ for the ASan/UBSan build.

Action and increment scenarios: external values, sanitised where the step fetches them.  The state stays finite by
contract, so they are ordinary bit-for-bit parity runs, plus a twin run that is fed what the contract says the
value acts as.

State-borne scenarios: non-finite state through set_state or reset params.  Not sanitised: the affected arenas'
values are unspecified, the step terminates, no other arena changes, a masked reset restores the arena.  They run
on the CPU only, in a child process (``python nonfinite_cases.py NAME``) under the caller's time limit.
"""
import os
import sys

import numpy as np

CLEAN, AFFECTED = 10, 60  # clean steps, then steps that carry the value
STEPS = CLEAN + AFFECTED
MODES = (0, 1, 2)


def lanes(n):
    """The affected arenas: first lane, an odd one, both sides of the first wave boundary, the last arena
    (128 arenas: 0, 5, 63, 64, 127; 100 arenas: the last lane of a partial wave)."""
    return [0, 5, 63, 64, n - 1]


# float32 bit patterns of the action values, and what each must act as (None: itself).  +-3e38 clip like +-Inf, so
# their twin is +-1 as well.  The payload NaN is a signalling one: fraction MSB clear.
ACTION_VALUES = {
    "nan": (0x7FC00000, 0.0),
    "nan_signbit": (0xFFC00000, 0.0),
    "nan_payload": (0x7FA12345, 0.0),
    "+inf": (0x7F800000, 1.0),
    "-inf": (0xFF800000, -1.0),
    "+3e38": (int(np.float32(3e38).view(np.uint32)), 1.0),
    "-3e38": (int(np.float32(-3e38).view(np.uint32)), -1.0),
    "denormal_1e-45": (0x00000001, None),
    "-0.0": (0x80000000, None),
}
# float64 bit patterns of the phase-increment values; every one acts as 0
INC_VALUES = {
    "nan": 0x7FF8000000000000,
    "nan_signbit_payload": 0xFFF4000000012345,
    "+inf": 0x7FF0000000000000,
    "-inf": 0xFFF0000000000000,
}
# policy settings: context policies, whether io.actions is given, whether player 2's policy is drawn per step
ACTION_KINDS = {
    "ext_ext": (("external", "external"), True, False),
    "ext_strong": (("external", "strong"), True, False),
    "mix": (("external", "external"), True, True),
}
INC_KINDS = {
    "strong_weak": (("strong", "weak"), False, False),
    "ext_strong": (("external", "strong"), True, False),
    "mix": (("external", "external"), True, True),
}
# Component placement.  Arenas are independent, so one batch runs five placements at once: affected arena j carries
# the value in component (c0 + j) % 8.  c0 = 0 covers components 0..4 and c0 = 3 covers 3..7: each of the 8 in turn.
C0S = (0, 3)


def _is_nan32(bits):
    return (bits & 0x7F800000) == 0x7F800000 and (bits & 0x007FFFFF) != 0


class Inputs:
    """One scenario's per-step inputs: the run that carries the value (``acts`` / ``inc``), its twin
    (``twin_acts`` / ``twin_inc``; None = the scenario has no substitution) and the expected HK_CNT_BAD_ACTION."""

    def __init__(self, n, policies, mode, seed):
        self.n, self.policies, self.mode, self.seed = n, policies, mode, seed
        self.acts = self.twin_acts = self.inc = self.twin_inc = self.p2 = None
        self.count = 0
        self.twin_fields_differ = ()  # output fields the twin may differ in by construction


def _base(n, kinds, kind, mode, seed, with_inc):
    policies, ext, mix = kinds[kind]
    x = Inputs(n, policies, mode, seed)
    rng = np.random.default_rng(seed)
    if ext:
        x.acts = rng.uniform(-1.2, 1.2, (STEPS, n, 8)).astype(np.float32)
    if mix:
        x.p2 = rng.choice(np.array([0, 2, 3], np.uint8), (STEPS, n))
    if with_inc:
        x.inc = rng.uniform(0.0, 0.2, (STEPS, n, 2))
    return x


def action_inputs(n, kind, mode, value, c0, seed=0):
    bits, acts_as = ACTION_VALUES[value]
    x = _base(n, ACTION_KINDS, kind, mode, 1000 + seed, False)
    clean = x.acts
    x.acts = clean.copy()
    if acts_as is not None:
        x.twin_acts = clean.copy()
    for j, a in enumerate(lanes(n)):
        c = (c0 + j) % 8
        x.acts.view(np.uint32)[CLEAN:, a, c] = bits
        if acts_as is not None:
            x.twin_acts[CLEAN:, a, c] = acts_as
    if _is_nan32(bits):
        x.count = len(lanes(n)) * AFFECTED
    elif acts_as is not None:
        x.twin_fields_differ = ("actions",)  # actions_out reports the value before the clip: Inf against 1
    return x


def inc_inputs(n, kind, mode, value, seed=0):
    x = _base(n, INC_KINDS, kind, mode, 2000 + seed, True)
    clean = x.inc
    x.inc = clean.copy()
    x.twin_inc = clean.copy()
    for j, a in enumerate(lanes(n)):
        x.inc.view(np.uint64)[CLEAN:, a, j % 2] = INC_VALUES[value]
        x.twin_inc[CLEAN:, a, j % 2] = 0.0
    x.count = len(lanes(n)) * AFFECTED  # counted whether or not a bot reads that increment in that step
    return x


def twin_of(x):
    """The twin run's inputs: the contract's substitutions, no counted arena-step."""
    t = Inputs(x.n, x.policies, x.mode, x.seed)
    t.acts = x.acts if x.twin_acts is None else x.twin_acts
    t.inc = x.inc if x.twin_inc is None else x.twin_inc
    t.p2 = x.p2
    return t


def run_steps(env, x, step):
    """Step ``env`` through the scenario; step(env, actions, opp_inc, policy2) -> dict of numpy outputs (copies)."""
    out = []
    for t in range(STEPS):
        out.append(step(env, None if x.acts is None else x.acts[t], None if x.inc is None else x.inc[t],
                        None if x.p2 is None else x.p2[t]))
    return out


def host_step(env, a, inc, p2):
    r = vars(env.step(a, with_agent_two=True, opp_inc=inc, record_actions=True, final_obs=True, policy2=p2))
    return r


def oracle_step(ov, a, inc, p2):
    return ov.step(a, inc, with_agent_two=True, final_obs=True, policy2=p2)


# ------------------------------------------------------------------------------------------------ state-borne
INF = float("inf")
# state18 = p1 {x, y, angle, vx, vy, w}, p2 {...}, puck {...}; params6 = p2x, p2y, puckx, pucky, puck_fx, puck_fy
STATE_CASES = {
    "p1_x_+inf": ("state", {0: INF}),
    "puck_y_-inf": ("state", {13: -INF}),
    "p2_xy_inf": ("state", {6: INF, 7: -INF}),
    "p1_angle_+inf": ("state", {2: INF}),
    "puck_vx_+inf": ("state", {15: INF}),
    "p1_vx_-inf": ("state", {3: -INF}),
    "p2_w_+inf": ("state", {11: INF}),
    "puck_v_3e38": ("state", {15: 3e38, 16: 3e38}),
    "p2_v_-3e38": ("state", {9: -3e38, 10: 3e38}),
    "all_v_3e38": ("state", {3: 3e38, 4: -3e38, 5: 3e38, 9: 3e38, 15: -3e38}),
    "param_puckx_nan": ("params", {2: float("nan")}),
    "param_p2y_+inf": ("params", {1: INF}),
    "param_force_-inf": ("params", {4: -INF}),
    "param_force_nan": ("params", {4: float("nan"), 5: float("nan")}),
    "clean": ("state", {}),
}


def _same(got, want, rows, fields):
    for f in fields:
        g = np.asarray(got[f]).reshape(len(want[f]), -1)[rows]
        w = np.asarray(want[f]).reshape(len(want[f]), -1)[rows]
        if g.tobytes() != w.tobytes():
            bad = [int(r) for r, gg, ww in zip(rows, g, w) if gg.tobytes() != ww.tobytes()]
            return f"{f}: arenas {bad[:8]}"
    return None


def run_state_case(name, mode=0, n=128, seed=7):
    """Returns None, or a description of the first violation.  The host build (`h`), a clean twin of it (`c`) and
    the oracle (`o`) step the same external actions; after CLEAN steps `h` and `o` take the non-finite values in the
    affected arenas.  Unaffected arenas: h == c == o at every step.  After a masked reset of the affected arenas
    from finite params the whole batch: h == o for AFFECTED more steps."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import oracle as O
    from hostcheck import HostVec
    from hockey_amd.placement import np_random, placement

    how, poke = STATE_CASES[name]
    kw = dict(keep_mode=True, mode=mode, policies=("external", "external"), auto_reset=False, seed=seed)
    h, c, o = HostVec(n, **kw), HostVec(n, **kw), O.OracleVec(n, **kw)
    params = np.zeros((n, 6), np.float32)
    for i in range(n):
        rng, _ = np_random(seed * 1000 + i)
        params[i], _ = placement(mode, bool(i % 2), rng)
    for e in (h, c):
        e.reset_params(params)
    o.reset(params=params)
    hit = np.zeros(n, np.uint8)
    hit[lanes(n)] = 1
    rest = np.nonzero(hit == 0)[0]
    everyone = np.arange(n)
    fields = ("obs", "obs2", "reward", "reward2", "done", "info", "info2", "final_obs")
    rng = np.random.default_rng(seed)

    def step_all(t, rows, with_twin):
        a = rng.uniform(-1.2, 1.2, (n, 8)).astype(np.float32)
        got, want = host_step(h, a, None, None), oracle_step(o, a, None, None)
        bad = _same(got, want, rows, fields)
        if bad:
            return f"step {t}: host build vs oracle: {bad}"
        if with_twin:
            bad = _same(got, host_step(c, a, None, None), rows, fields)
            if bad:
                return f"step {t}: host build vs its clean twin: {bad}"
        hs, ha = h.get_state()
        os_, oa = o.get_state()
        if hs[rows].tobytes() != os_[rows].tobytes() or ha[rows].tobytes() != oa[rows].tobytes():
            return f"step {t}: state, host build vs oracle"
        if with_twin:
            cs, ca = c.get_state()
            if hs[rows].tobytes() != cs[rows].tobytes() or ha[rows].tobytes() != ca[rows].tobytes():
                return f"step {t}: state, host build vs its clean twin"
        return None

    for t in range(CLEAN):
        bad = step_all(t, everyone, True)
        if bad:
            return bad
    if how == "state":
        st, _ = h.get_state()
        for k, v in poke.items():
            st[:, k] = v
        h.set_state(st, None, hit)
        o.set_state(st, None, hit)
    else:
        p = params.copy()
        for k, v in poke.items():
            p[:, k] = v
        h.reset_params(p, hit)
        o.reset(hit, p)
        c.reset_params(params, hit)  # the twin's affected arenas are not compared; its others must not notice
    for t in range(CLEAN, STEPS):
        bad = step_all(t, rest, True)
        if bad:
            return bad
    h.reset_params(params, hit)
    o.reset(hit, params)
    for t in range(STEPS, STEPS + AFFECTED):
        bad = step_all(t, everyone, False)
        if bad:
            return f"after the masked reset: {bad}"
    return None


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "hockey-env_amd"))
    bad = run_state_case(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    print(bad or "ok")
    sys.exit(1 if bad else 0)
