"""Values that are not finite numbers, on gfx950 (include/hockey.h "Non-finite values"; the CPU side is
tests/test_nonfinite.py, which passes before these run).

Step kernel: the action and increment scenarios of tests/nonfinite_cases.py through hk_step and hk_rollout, at 128
arenas (two full waves) and 100 (a partial wave), against the oracle bit for bit, HK_CNT_BAD_ACTION included.  The
state stays finite by contract, so these are ordinary parity runs.  The state-borne scenarios are NOT run here: their
termination evidence comes from the host build, which steps one lane at a time, not from the wave-cooperative drains.

hkl_act / hkl_value: a row that holds NaN, +-Inf or 3e38 changes no other row's bits -- at the first and the last row
of a 64-row tile and at the last row of a partial tile, whose spare lanes recompute it -- and is itself written, with
actions that are NaN or lie in [-1, 1].  Policy ids outside [0, K) leave their rows unwritten.

hkl_sample / hkl_sample_group: a fill word of 0 or -1 gives slot 0 for every sample (out-of-contract device values are
clamped, never addressed); the noise is learner_ref.sample_noise within learner_ref.bound, as for any fill level.
The sampler is launched alone: it does not address the ring.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import learner_ref as R  # noqa: E402
import nonfinite_cases as C  # noqa: E402
import value_ref as V  # noqa: E402
from hockey_amd import _native as N  # noqa: E402
from hockey_amd import learner_hip as LH  # noqa: E402
from scene_lockstep import require_gfx950  # noqa: E402
from vec_lockstep import FIELDS, first_mismatch  # noqa: E402

DEV = "cuda:0"
PREFILL = 0x7FC00BAD  # a NaN no kernel computes: a float that still holds it was not written
POISON = (float("nan"), float("inf"), float("-inf"), 3e38)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gfx950()


# ---------------------------------------------------------------------------------------------------- step kernel
_OUT = (("obs", 18, torch.float32), ("obs2", 18, torch.float32), ("reward", 0, torch.float32),
        ("reward2", 0, torch.float32), ("done", 0, torch.uint8), ("info", 4, torch.float32),
        ("info2", 4, torch.float32), ("actions", 8, torch.float32), ("final_obs", 18, torch.float32))


def _env(x):
    from hockey_amd.vec_env import VecHockeyEnv
    return VecHockeyEnv(x.n, keep_mode=True, mode=x.mode, device=DEV, policies=x.policies, auto_reset=True,
                        seed=x.seed)


def _dev(a):
    return None if a is None else torch.as_tensor(a, device=DEV)


def _per_step(stacked):
    host = {k: v.cpu().numpy() for k, v in stacked.items()}
    return [{k: v[t] for k, v in host.items()} for t in range(C.STEPS)]


def _by_step(env, x):
    """STEPS hk_step launches; the outputs stay on the device until the end."""
    acts, inc, p2 = _dev(x.acts), _dev(x.inc), _dev(x.p2)
    keep = {k: [] for k, _, _ in _OUT}
    for t in range(C.STEPS):
        r = env.step(None if acts is None else acts[t], with_agent_two=True, opp_inc=None if inc is None else inc[t],
                     record_actions=True, final_obs=True, policy2=None if p2 is None else p2[t])
        for k in keep:
            keep[k].append(getattr(r, k).clone())
    return _per_step({k: torch.stack(v) for k, v in keep.items()})


def _by_rollout(env, x):
    """One hk_rollout launch of STEPS steps with every input and output array."""
    acts, inc, p2 = _dev(x.acts), _dev(x.inc), _dev(x.p2)
    out = {k: torch.empty((C.STEPS, x.n) + ((w,) if w else ()), dtype=dt, device=DEV) for k, w, dt in _OUT}
    io = N.StepIO()
    io.actions = None if acts is None else acts.data_ptr()
    io.opp_inc = None if inc is None else inc.data_ptr()
    io.policy2 = None if p2 is None else p2.data_ptr()
    for k in out:
        setattr(io, "actions_out" if k == "actions" else k, out[k].data_ptr())
    env.rollout_raw(C.STEPS, io)
    return _per_step(out)


def _gpu_vs_oracle(oracle, x):
    ov = oracle.OracleVec(x.n, keep_mode=True, mode=x.mode, policies=x.policies, auto_reset=True, seed=x.seed)
    want = C.run_steps(ov, x, C.oracle_step)
    ost, oaux = ov.get_state()
    oc = ov.counters()
    ov.close()
    assert oc[N.CNT_BAD_ACTION] == x.count
    for path, run in (("hk_step", _by_step), ("hk_rollout", _by_rollout)):
        env = _env(x)
        got = run(env, x)
        for t in range(C.STEPS):
            bad = first_mismatch(t, got[t], want[t], fields=FIELDS)
            assert bad is None, (path, bad)
        st, aux = env.get_state()
        st, aux = st.cpu().numpy(), aux.cpu().numpy()
        assert np.array_equal(st.view(np.uint32), ost.view(np.uint32)) and np.array_equal(aux, oaux), path
        assert np.isfinite(st).all(), path
        c = env.counters()
        assert np.array_equal(c[:5], oc[:5]), (path, c, oc)
        assert c[N.CNT_BAD_ACTION] == x.count, (path, c, x.count)
        assert c[N.CNT_OVERFLOW] == 0 and c[N.CNT_BAD_POLICY] == 0, (path, c)
        env.close()


@pytest.mark.parametrize("kind", list(C.ACTION_KINDS))
@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("n", [128, 100])
def test_step_kernel_action_values(oracle, n, mode, kind):
    """Every action value, in each of the 8 components, at lanes 0, 5, 63, 64 and the last arena: hk_step and
    hk_rollout equal the oracle on every output, the final state and the counters."""
    for c0 in C.C0S:
        for value in C.ACTION_VALUES:
            _gpu_vs_oracle(oracle, C.action_inputs(n, kind, mode, value, c0, seed=mode))


@pytest.mark.parametrize("kind", list(C.INC_KINDS))
@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("n", [128, 100])
def test_step_kernel_phase_increment_values(oracle, n, mode, kind):
    for value in C.INC_VALUES:
        _gpu_vs_oracle(oracle, C.inc_inputs(n, kind, mode, value, seed=mode))


# ---------------------------------------------------------------------------------------------------- hkl_act
def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _prefilled(*shape):
    return torch.full(shape, PREFILL, dtype=torch.int32, device=DEV).view(torch.float32)


def _tile_rows(n):
    """First and last row of every 64-row tile of n rows, the last row of the partial tile included."""
    return sorted({r for r in range(n) if r % 64 in (0, 63)} | {n - 1})


def _poisoned(t, rows, value, cols):
    """A copy of t [n, k] with `value` in row rows[i], column (5 i + 1) % cols."""
    p = t.clone()
    for i, r in enumerate(rows):
        p[r, (5 * i + 1) % cols] = value
    return p


@functools.lru_cache(maxsize=None)
def _bank(K=3):
    from hockey_amd.policy_bank import PolicyBank

    g = torch.Generator().manual_seed(5 + K)
    bank = PolicyBank(K, DEV)
    for _ in range(K):
        bank.add(R._net(g, 18, 4))
    return bank


def _act(bank, obs, pol):
    out = _prefilled(obs.shape[0], 8)
    bank.act(obs, pol, out=out, out_col=0, backend="hip")
    torch.cuda.synchronize()
    return out


def _assert_isolated(clean, got, poisoned_rows, acting, width=4):
    """Rows outside poisoned_rows: the clean call's bits.  Poisoned acting rows: written, NaN or in [-1, 1]."""
    n = clean.shape[0]
    rest = torch.ones(n, dtype=torch.bool)
    rest[poisoned_rows] = False
    assert torch.equal(_bits(got)[rest], _bits(clean)[rest]), "a poisoned row changed another row"
    for r in poisoned_rows:
        if acting[r]:
            assert (_bits(got)[r, :width] != PREFILL).all(), f"poisoned row {r} was not written"
            v = got[r, :width].cpu()
            assert bool((torch.isnan(v) | (v.abs() <= 1.0)).all()), (r, v)


def test_act_row_isolation():
    """n = 200, K = 3.  Without a policy array the tiles are rows 64 b .. 64 b + 63: rows 0 / 64 / 128 / 192 open a
    tile, 63 / 127 / 191 close one, 199 closes the partial tile.  With one, a tile holds 64 rows of one policy's
    group in an order the scatter's atomics decide, so the known positions are made by group size: slot 1's group is
    the single row 77 (the last row of a partial tile, recomputed by 63 spare lanes), slot 0's is exactly one full
    tile, and slot 2's 135 rows end in a partial tile; row 77, two rows of slot 0's tile and the tile-edge rows are
    poisoned."""
    n, K = 200, 3
    bank = _bank(K)
    obs = (torch.randn(n, 18, generator=torch.Generator().manual_seed(77)) * 1.5).to(DEV)
    edge = _tile_rows(n)
    assert edge == [0, 63, 64, 127, 128, 191, 192, 199]
    pol = torch.full((n,), 2, dtype=torch.int32)
    pol[torch.arange(0, 192, 3)] = 0
    pol[77] = 1
    assert int((pol == 0).sum()) == 64 and int((pol == 1).sum()) == 1
    everyone = torch.ones(n, dtype=torch.bool)
    for policy, rows in ((None, edge), (pol.to(DEV), sorted(set(edge) | {77, 3, 6}))):
        clean = _act(bank, obs, policy)
        assert (_bits(clean)[:, :4] != PREFILL).all() and (_bits(clean)[:, 4:] == PREFILL).all()
        assert torch.isfinite(clean[:, :4]).all()
        for value in POISON:
            _assert_isolated(clean, _act(bank, _poisoned(obs, rows, value, 18), policy), rows, everyone)


def test_act_out_of_range_policy_ids_are_not_addressed():
    """Policy ids K, 2^31 - 1, -2 and -2^31 leave their rows unwritten (-1 is the documented "does not act"); the
    other rows are the bits of a call in which those rows are at -1."""
    n, K = 200, 3
    bank = _bank(K)
    obs = (torch.randn(n, 18, generator=torch.Generator().manual_seed(78)) * 1.5).to(DEV)
    pol = (torch.arange(n, dtype=torch.int32) % K)
    base = pol.clone()
    odd = {0: K, 63: 2 ** 31 - 1, 64: -2, 199: -2 ** 31, 100: K, 101: -2}
    for r, k in odd.items():
        pol[r], base[r] = k, -1
    got, want = _act(bank, obs, pol.to(DEV)), _act(bank, obs, base.to(DEV))
    assert torch.equal(_bits(got), _bits(want))
    assert (_bits(got)[list(odd)] == PREFILL).all(), "a row with an id outside [0, K) was written"
    acting = torch.ones(n, dtype=torch.bool)
    acting[list(odd)] = False
    assert (_bits(got)[acting][:, :4] != PREFILL).all() and (_bits(got)[:, 4:] == PREFILL).all()


# ---------------------------------------------------------------------------------------------------- hkl_value
@functools.lru_cache(maxsize=None)
def _vf():
    from hockey_amd.value import ValueFn

    nets = V.value_nets(21, 1.5)
    return ValueFn((nets["actor"], V.critic_state(nets, (-1.0,) * 4, (2.0,) * 4)), DEV)


def _value(obs, act):
    """One hkl_value call into prefilled buffers: [n, 7] = q1, q2, qmin and (V mode) the actor's action."""
    vf, n = _vf(), obs.shape[0]
    q = _prefilled(3, n)
    a = _prefilled(n, 4)
    io = LH.ValueIO()
    io.n_rows = n
    io.actor, io.q[0], io.q[1] = vf.actor.net(), vf.critics[0].net(), vf.critics[1].net()
    io.obs, io.obs_ld = obs.data_ptr(), obs.stride(0)
    if act is not None:
        io.act, io.act_ld = act.data_ptr(), act.stride(0)
    else:
        io.act_out, io.act_out_ld = a.data_ptr(), 4
    for c in range(4):
        io.act_low[c], io.act_range[c] = vf._low[c], vf._range[c]
    io.q1, io.q2, io.qmin = q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr()
    rc = LH.lib().hkl_value(ctypes.byref(io), ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, LH.lib().hkl_last_error()
    torch.cuda.synchronize()
    return torch.cat([q.t(), a], dim=1)


@pytest.mark.parametrize("mode", ["Q", "V"])
@pytest.mark.parametrize("n", [65, 200])
def test_value_row_isolation(n, mode):
    """The tile-edge rows (n = 65: rows 0 and 63 of the full tile, row 64 alone in the partial one) hold NaN, +-Inf
    or 3e38 in the observation, and in Q mode in the action: every other row's q1 / q2 / qmin (and V mode's action)
    are the clean call's bits, and every poisoned row's outputs were written."""
    g = torch.Generator().manual_seed(100 + n)
    obs = (torch.randn(n, 18, generator=g) * 1.5).to(DEV)
    act = (torch.rand(n, 4, generator=g) * 2 - 1).to(DEV) if mode == "Q" else None
    rows = _tile_rows(n)
    clean = _value(obs, act)
    width = 3 if mode == "Q" else 7
    assert (_bits(clean)[:, :width] != PREFILL).all() and torch.isfinite(clean[:, :width]).all()
    assert (_bits(clean)[:, width:] == PREFILL).all()
    rest = torch.ones(n, dtype=torch.bool)
    rest[rows] = False
    for value in POISON:
        runs = [_value(_poisoned(obs, rows, value, 18), act)]
        if mode == "Q":
            runs.append(_value(obs, _poisoned(act, rows, value, 4)))
            runs.append(_value(_poisoned(obs, rows[::2], value, 18), _poisoned(act, rows[1::2], value, 4)))
        for got in runs:
            assert torch.equal(_bits(got)[rest], _bits(clean)[rest]), (value, "a poisoned row changed another row")
            assert (_bits(got)[rows][:, :width] != PREFILL).all(), (value, "a poisoned row was not written")
            assert (_bits(got)[:, width:] == PREFILL).all()
            if mode == "V":
                a = got[rows][:, 3:7].cpu()
                assert bool((torch.isnan(a) | (a.abs() <= 1.0)).all()), (value, a)


# ---------------------------------------------------------------------------------------------------- hkl_sample
def _sample_io(B, seed, size, ctr):
    t = {"counter": torch.tensor([ctr], dtype=torch.int64, device=DEV),
         "size": torch.tensor([size], dtype=torch.int64, device=DEV),
         "idx": torch.full((B,), -7, dtype=torch.int64, device=DEV), "noise": _prefilled(B, 4)}
    io = LH.SampleIO()
    io.batch, io.seed, io.scale, io.clip = B, seed, 0.2, 0.5
    for k, v in t.items():
        setattr(io, k, v.data_ptr())
    return io, t


def _assert_sampled(t, B, seed, ctr):
    assert bool((t["idx"] == 0).all()), t["idx"].cpu().unique()
    noise = t["noise"].cpu()
    n64, n32 = R.sample_noise(seed, B, ctr, 0.2, 0.5), R.sample_noise(seed, B, ctr, 0.2, 0.5, np.float32)
    err, eager = R.rel_err(noise, torch.from_numpy(n64)), R.rel_err(torch.from_numpy(n32), torch.from_numpy(n64))
    assert err <= R.bound(eager), (err, eager)
    assert float(noise.abs().max()) <= 0.5
    assert int(t["counter"]) == ctr


@pytest.mark.parametrize("size", [0, -1])
def test_sample_on_an_empty_ring_gives_slot_zero(size):
    """*size == 0 (nothing pushed yet) and -1 (out of contract): every slot is 0.  Before the clamp sample_slot
    returned size - 1 in uint64, slot -1 (-2), which the critic step would have addressed."""
    B, seed, ctr = 768, 0x1234ABCD, 5
    st = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    io, t = _sample_io(B, seed, size, ctr)
    LH._check(LH.lib().hkl_sample(ctypes.byref(io), st), "hkl_sample")
    torch.cuda.synchronize()
    _assert_sampled(t, B, seed, ctr)
    # the grouped launch: member 0 on a ring with 1000 slots filled, member 1 on the empty one
    (io0, t0), (io1, t1) = _sample_io(B, seed + 1, 1000, ctr), _sample_io(B, seed, size, ctr)
    host = (LH.SampleIO * 2)(io0, io1)
    dev = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
    LH._check(LH.lib().hkl_sample_group(host, ctypes.c_void_p(dev.data_ptr()), 2, st), "hkl_sample_group")
    torch.cuda.synchronize()
    _assert_sampled(t1, B, seed, ctr)
    assert np.array_equal(t0["idx"].cpu().numpy(), R.sample_slots(seed + 1, B, ctr, 1000))
