"""Twin-critic inference (hockey_amd/value.py, hkl_value of include/hockey_learner.h) and what is built on it --
Lookahead's value bootstrap and the shooting planner's candidates -- on the CPU: the binding, the torch reference
backend against TD3's own modules and against the float64 restatement (tests/value_ref.py), bootstrap and
shooting_candidates.  tests/test_gpu_value.py holds the kernel itself to the float64 restatement."""
import ctypes
import os

import numpy as np
import pytest
import torch

import learner_ref as R
import value_ref as V
from hockey_amd import learner_hip as LH
from hockey_amd.lookahead import bootstrap
from hockey_amd.planner import shooting_candidates
from hockey_amd.value import ValueFn

IDENT = ((-1.0,) * 4, (2.0,) * 4)
AFFINE = (R.ACT_AFFINE_LOW, R.ACT_AFFINE_RANGE)


def _agent(seed=3, affine=False):
    from hockey_amd.td3 import TD3

    agent = TD3(device="cpu", seed=seed)
    if affine:
        with torch.no_grad():
            agent.critic.action_low.copy_(torch.tensor(AFFINE[0]))
            agent.critic.action_range.copy_(torch.tensor(AFFINE[1]))
            agent.critic.action_high.copy_(agent.critic.action_low + agent.critic.action_range)
    return agent


def _rows(n, affine, seed=0):
    g = torch.Generator().manual_seed(100 + n + seed)
    low, rng = (torch.tensor(t) for t in (AFFINE if affine else IDENT))
    return torch.randn(n, 18, generator=g) * 1.5, low + rng * torch.rand(n, 4, generator=g)


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_library_exports_hkl_value_and_the_struct_sizes_agree():
    """The cross-compiled libhockey_learner.so exports hkl_value, hkl_value_io as ctypes lays it out has the size the
    library compiled, and bad arguments are refused on the host with a text, before anything touches a device."""
    assert os.path.exists(LH.LIB_PATH), "build() compiles libhockey_learner.so"
    L = ctypes.CDLL(LH.LIB_PATH)
    assert hasattr(L, "hkl_value") and "hkl_value" in LH.EXPORTS and "hkl_value_io_size" in LH.EXPORTS
    assert L.hkl_value_io_size() == ctypes.sizeof(LH.ValueIO)
    L.hkl_value.argtypes = [ctypes.POINTER(LH.ValueIO), ctypes.c_void_p]
    L.hkl_last_error.restype = ctypes.c_char_p
    net = LH.Net(8, 8, 8, 8, 8, 8, 8, 22, 1)

    def io(**kw):
        x = LH.ValueIO(n_rows=0, obs=8, obs_ld=18, act=8, act_ld=4, qmin=8)
        x.actor, x.q[0], x.q[1] = LH.Net(8, 8, 8, 8, 8, 8, 8, 18, 4), net, net
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    assert L.hkl_value(ctypes.byref(io()), None) == 0  # zero rows: nothing to do, nothing launched
    assert L.hkl_value(ctypes.byref(io(act=None, act_out=8, act_out_ld=4, qmin=None)), None) == 0
    no_w2 = io()
    no_w2.q[1].w2 = None
    no_pack = io(act=None)
    no_pack.actor.pack = None
    for bad in (io(n_rows=-1), io(obs_ld=17), io(act_ld=3), io(act_out=8, act_out_ld=4), io(obs=None),
                io(act=None, act_out=8, act_out_ld=3), io(qmin=None), no_w2, no_pack):
        assert L.hkl_value(ctypes.byref(bad), None) == 1
        assert L.hkl_last_error().startswith(b"hkl_value: ")
    no_pack.act = 8  # Q mode does not read the actor
    assert L.hkl_value(ctypes.byref(no_pack), None) == 0


def test_lazy_exports():
    import hockey_amd

    from hockey_amd.planner import ShootingPlanner

    assert hockey_amd.ValueFn is ValueFn and hockey_amd.ShootingPlanner is ShootingPlanner


@pytest.mark.parametrize("affine", (False, True))
@pytest.mark.parametrize("n", (1, 65))
def test_torch_backend_equals_the_agents_modules(n, affine):
    """ValueFn(backend="torch") on the CPU is TD3's own actor / critic modules bit for bit: q, qmin, v and v's action,
    on contiguous rows and on strided views (obs as [:, :18] of 24 columns, act as act8[:, :4])."""
    agent = _agent(affine=affine)
    vf = ValueFn(agent, device="cpu")
    obs, act = _rows(n, affine)
    with torch.no_grad():
        w1, w2 = agent.critic(obs, act)
        a = agent.actor(obs)
        wv = torch.minimum(*agent.critic(obs, a))
    obs24, act8 = torch.full((n, 24), 9.0), torch.full((n, 8), 9.0)
    obs24[:, :18], act8[:, :4] = obs, act
    for o, c in ((obs, act), (obs24[:, :18], act8[:, :4]), (obs24, act8)):
        q1, q2 = vf.q(o, c, backend="torch")
        assert q1.shape == (n,) and torch.equal(_bits(q1), _bits(w1)) and torch.equal(_bits(q2), _bits(w2))
        assert torch.equal(_bits(vf.qmin(o, c, backend="torch")), _bits(torch.minimum(w1, w2)))
        v, va = vf.v(o, backend="torch", return_action=True)
        assert torch.equal(_bits(v), _bits(wv)) and torch.equal(_bits(va), _bits(a))
        assert torch.equal(_bits(vf.v(o, backend="torch")), _bits(wv))
    assert torch.equal(_bits(vf.v(obs)), _bits(wv))  # "auto" on the CPU is the torch path


@pytest.mark.parametrize("affine", (False, True))
@pytest.mark.parametrize("n", (1, 65))
def test_torch_backend_within_its_own_fp32_error_of_the_float64_restatement(n, affine):
    """The torch path against value_ref.value_reference in float64 (the restatement the GPU tests use): within
    learner_ref.bound of the restatement's own float32 error, for networks from learner_ref._net given as an
    (actor, twin_q) pair of state dicts."""
    low, rng = AFFINE if affine else IDENT
    nets = V.value_nets(21)
    vf = ValueFn((nets["actor"], V.critic_state(nets, low, rng)), device="cpu")
    obs, act = _rows(n, affine, seed=1)
    for a in (act, None):
        ref64 = V.value_reference(nets, obs, a, low, rng)
        ref32 = V.value_reference(nets, obs, a, low, rng, dtype=torch.float32)
        if a is None:
            qmin, a_out = vf.v(obs, backend="torch", return_action=True)
            got = {"qmin": qmin, "a": a_out}
        else:
            q1, q2 = vf.q(obs, a, backend="torch")
            got = {"q1": q1, "q2": q2, "qmin": vf.qmin(obs, a, backend="torch")}
        for k, t in got.items():
            err, bound = R.rel_err(t, ref64[k]), R.bound(R.rel_err(ref32[k], ref64[k]))
            assert err <= bound, (k, err, bound)


def test_refresh_picks_up_changed_weights_and_sources():
    """The ValueFn holds copies: training the agent on does not move its values until refresh(); refresh(source)
    switches to a checkpoint dict, which gives the values of the agent it was taken from."""
    agent = _agent()
    vf = ValueFn(agent, device="cpu")
    obs, act = _rows(7, False)
    before = vf.qmin(obs, act, backend="torch")
    ck = agent.checkpoint()
    with torch.no_grad():
        for p in list(agent.critic.parameters()) + list(agent.actor.parameters()):
            p.mul_(1.25)
    assert torch.equal(vf.qmin(obs, act, backend="torch"), before)
    vf.refresh()
    with torch.no_grad():
        want = torch.minimum(*agent.critic(obs, act))
        want_v = torch.minimum(*agent.critic(obs, agent.actor(obs)))
    assert not torch.equal(want, before) and torch.equal(vf.qmin(obs, act, backend="torch"), want)
    assert torch.equal(vf.v(obs, backend="torch"), want_v)
    vf.refresh(ck)
    assert torch.equal(vf.qmin(obs, act, backend="torch"), before)
    with pytest.raises(ValueError):
        vf.refresh({"policy": ck["policy"]})
    with pytest.raises(ValueError):
        ValueFn((torch.nn.Linear(18, 4), agent.critic), device="cpu")


def test_bad_shapes_and_dtypes_raise():
    vf = ValueFn(_agent(), device="cpu")
    obs, act = _rows(5, False)
    for o, a in ((obs[:, :17], act), (obs.double(), act), (obs, act[:, :3]), (obs, act.double()), (obs, act[:4]),
                 (obs[0], act), (obs, act.reshape(5, 2, 2)), (obs.numpy(), act)):
        with pytest.raises(ValueError):
            vf.q(o, a, backend="torch")
        with pytest.raises(ValueError):
            vf.qmin(o, a, backend="torch")
    for o in (obs[:, :17], obs.double(), obs[0]):
        with pytest.raises(ValueError):
            vf.v(o, backend="torch")
    with pytest.raises(ValueError):
        vf.v(obs, backend="cuda")
    # a column stride is made contiguous, not refused
    wide = torch.zeros(5, 36)
    wide[:, ::2] = obs
    assert torch.equal(vf.v(wide[:, ::2], backend="torch"), vf.v(obs, backend="torch"))


def test_bootstrap_against_a_plain_loop():
    """H = 4, M = 2, K = 3: branches done at step 0, done at the last step, never done, and a done branch whose
    value is NaN; the result is the float64 loop's, rounded once."""
    H, M, K, gamma = 4, 2, 3, 0.95
    dones = torch.zeros((H, M, K), dtype=torch.uint8)
    dones[:, 0, 0] = 1          # done at step 0 (sticky)
    dones[H - 1, 0, 1] = 1      # done at the last step
    dones[1:, 1, 2] = 1         # done inside, its value NaN
    g = torch.Generator().manual_seed(8)
    returns = torch.randn(M, K, generator=g) * 3
    values = torch.randn(M, K, generator=g) * 7
    values[1, 2] = float("nan")
    got = bootstrap(returns, dones, values, gamma)
    assert got.dtype == torch.float32 and got.shape == (M, K)
    want = np.zeros((M, K), np.float32)
    for m in range(M):
        for k in range(K):
            ended = any(int(dones[t, m, k]) for t in range(H))
            x = float(returns[m, k])
            if not ended:
                x = x + gamma ** H * float(values[m, k])
            want[m, k] = np.float32(x)
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    assert torch.isfinite(got).all()
    kept = torch.tensor([[True, True, False], [False, False, True]])
    assert torch.equal(got[kept], returns[kept]) and not torch.equal(got[~kept], returns[~kept])


def test_shooting_candidates():
    """Branch 0 is the base at every step, every entry lies in [-1, 1], the same seed gives the same tensor (another
    seed another), sigma = 0 gives the base everywhere."""
    M, K, H = 3, 5, 4
    base = torch.tensor([[0.9, -0.95, 0.0, 1.0], [-1.0, 0.2, 0.5, -0.5], [0.1, 0.1, -0.1, 0.99]])
    gen = lambda s: torch.Generator().manual_seed(s)  # noqa: E731
    c = shooting_candidates(base, K, H, 0.5, gen(1))
    assert c.shape == (H, M, K, 4) and c.dtype == torch.float32
    assert torch.equal(c[:, :, 0], base.expand(H, M, 4))
    assert float(c.min()) >= -1.0 and float(c.max()) <= 1.0
    assert (c == 1.0).any() and (c == -1.0).any()  # the clamp acted
    assert not torch.equal(c[:, :, 1], base.expand(H, M, 4)) and not torch.equal(c[0], c[1])
    assert torch.equal(c, shooting_candidates(base, K, H, 0.5, gen(1)))
    assert not torch.equal(c, shooting_candidates(base, K, H, 0.5, gen(2)))
    assert torch.equal(shooting_candidates(base, K, H, 0.0, gen(1)), base[None, :, None, :].expand(H, M, K, 4))
    with pytest.raises(ValueError):
        shooting_candidates(base[:, :3], K, H, 0.5)
