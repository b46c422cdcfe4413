"""hkl_explore (include/hockey_explore.h, csrc/hkl_explore.h) on the GPU, through hockey_amd.explore.Explorer.

Every output and every scratch buffer the call may write is filled with NaN bits first and compared as int32, so a
float that should not have been written, or was not, shows.  The actor's part is hkl_act's (bit for bit); everything
after it is held exactly to the law in numpy (hockey_amd.explore.law, the torch backend's body) and to the
independent restatement tests/explore_ref.py, given hkl_act's actions and, for the normals, the kernel's own z_out,
which in turn is held to the float64 Box-Muller under learner_ref.bound.

The shapes are the smallest that can go wrong: rows_per_member 1, 20, 63, 64, 65, 70 with 1 and 3 members (partly
filled 64-row tiles, tiles that span members, groups reordered by the scatter) and 64 members of 3 rows.

This file captures no graph and takes no stream from torch's pool (tests/test_gpu_facade.py's blocked-stream test runs
after it and depends on the streams handed out before): the graph and training tests are in
tests/test_gpu_population_explore.py.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import explore_ref as XR  # noqa: E402
import learner_ref as R  # noqa: E402
from hockey_amd import explore as X  # noqa: E402
from hockey_amd.policy_bank import PolicyBank  # noqa: E402
from hockey_amd.td3 import Actor  # noqa: E402

DEV = "cuda:0"
SHAPES = [(n, S) for n in (1, 20, 63, 64, 65, 70) for S in (1, 3)] + [(3, 64)]
KINDS = ("gaussian", "ornstein-uhlenbeck", "uniform", "external", "none")
_banks = {}


def bank(S, same=False):
    """S slots of different actors (same: one actor in every slot), built once per S."""
    key = (S, same)
    if key not in _banks:
        torch.manual_seed(100 + S)
        b = PolicyBank(S, DEV)
        first = Actor()
        b.replace_many(range(S), [first if same else Actor() for _ in range(S)])
        _banks[key] = b
    return _banks[key]


def observations(N, seed):
    return torch.randn(N, 18, generator=torch.Generator().manual_seed(seed)).to(DEV)


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def nan_fill(ex, width=8):
    """Fresh NaN-filled out; the explorer's z / scale refilled with NaN (x is state: the caller decides)."""
    ex.z.fill_(float("nan"))
    ex.scale.fill_(float("nan"))
    return torch.full((ex.N, width), float("nan"), device=DEV)


def members_for(S, kinds, start=(0,), anneal=("linear", "exp", "none")):
    """Package members and their reference twins: member m takes kinds[m % ..], start[m % ..], anneal[m % ..]."""
    pk, rf = [], []
    for m in range(S):
        kw = dict(seed=(1 << 40) * (m % 3) + 17 * m + 5, start_steps=start[m % len(start)], max_total_steps=400 + 50 * m,
                  init_scale=0.3 - 0.001 * m, min_scale=0.05, anneal=anneal[m % len(anneal)],
                  noise=kinds[m % len(kinds)], theta=0.15 + 0.01 * (m % 4), dt=1.0 if m % 2 == 0 else 0.5)
        pk.append(X.Member(**kw))
        rf.append(XR.member(**kw))
    return pk, rf


@pytest.mark.parametrize("n,S", SHAPES)
def test_noise_none_equals_hkl_act_bit_for_bit(n, S):
    """noise "none", start_steps 0: columns [2, 6) of a NaN-filled out equal hkl_act's on the same inputs, every other
    column and the OU state keep their NaN bits, z_out is 0 and the counters advance."""
    b = bank(S)
    pk, _ = members_for(S, ("none",))
    ex = X.Explorer(b, pk, n, backend="hip", keep_draws=True)
    obs = observations(S * n, 3)
    ex.x.fill_(float("nan"))
    out = ex.explore(obs, nan_fill(ex), 2)
    want = b.act(obs, ex.policy, backend="hip")
    torch.cuda.synchronize()
    assert np.array_equal(bits(out[:, 2:6]), bits(want)) and torch.isfinite(want).all()
    assert torch.isnan(out[:, :2]).all() and torch.isnan(out[:, 6:]).all() and torch.isnan(ex.x).all()
    assert not bits(ex.z).any()
    assert ex.total.tolist() == [n] * S and ex.calls.tolist() == [1] * S


def _sequence(n, S, kinds, start):
    """5 calls with a varying count (all arenas in calls 0 and 3, one member at count 0 in call 2) against the law in
    numpy and explore_ref, given hkl_act's actions and the kernel's z_out.  Returns what the calls covered."""
    b = bank(S)
    pk, rf = members_for(S, kinds, start)
    ex = X.Explorer(b, pk, n, backend="hip", keep_draws=True)
    N = S * n
    g = torch.Generator().manual_seed(7 * n + S)
    total, calls = np.zeros(S, np.int64), np.zeros(S, np.int64)
    x = np.zeros((N, 4), np.float32)
    seen = {"random": 0, "noisy": 0, "all_random_ou": 0, "clamped": 0, "count0": 0}
    for c in range(5):
        obs = observations(N, 50 + c)
        block = torch.randn(N, 4, 3, generator=g).to(DEV)  # the external noise: a strided view of a [N, 4, 3] block
        ext = block[:, :, c % 3]
        count = torch.randint(1, n + 1, (S,), generator=g).to(torch.int32)
        if c in (0, 3):
            count[:] = n
        if c == 2:
            count[S // 2] = 0
        a = b.act(obs, ex.policy, backend="hip")
        out = ex.explore(obs, nan_fill(ex, 4), 0, count=count.to(DEV), ext=ext)
        torch.cuda.synchronize()
        z = ex.z.cpu().numpy()
        for name, ref in (("law", X.law(pk, n, total, calls, count.numpy(), a.cpu().numpy(), x, ext.cpu().numpy(), z)),
                          ("explore_ref", XR.call(rf, n, total, calls, count.numpy(), a.cpu().numpy(), x,
                                                  ext.cpu().numpy(), z))):
            assert same_bits(out.cpu().numpy(), ref["out"]), (name, c)
            assert same_bits(ex.x.cpu().numpy(), ref["x"]), (name, c)
            assert np.array_equal(ex.total.cpu().numpy(), ref["total"]), (name, c)
            assert np.array_equal(ex.calls.cpu().numpy(), ref["calls"]), (name, c)
            got_s = ex.scale.cpu().numpy()
            for m, mem in enumerate(pk):  # none / linear: exact; exp: the float64 pow may sit on a rounding boundary
                if mem.anneal == "exp":
                    assert abs(float(got_s[m]) - float(ref["scale"][m])) <= np.spacing(ref["scale"][m]), (name, c, m)
                else:
                    assert got_s[m].view(np.int32) == ref["scale"][m].view(np.int32), (name, c, m)
        # z_out: the uniform draws exactly; the normals under the float32 Box-Muller's own error; 0 elsewhere
        for m, mem in enumerate(rf):
            rows = slice(m * n, (m + 1) * n)
            t0, t1, all_random, mask = XR.phase(total[m], int(count[m]), n, mem["start_steps"])
            if all_random or mem["noise"] in ("none", "external"):
                assert not z[rows].view(np.int32).any(), (c, m)
                seen["all_random_ou"] += all_random and mem["noise"] == "ornstein-uhlenbeck"
                continue
            w = XR.words(mem["seed"], XR.KEY_NOISE, n, int(calls[m]))
            if mem["noise"] == "uniform":
                assert same_bits(z[rows], XR.uniform_pm1(w).astype(np.float32)), (c, m)
            else:
                ref64 = XR.normals(w)
                assert R.rel_err(z[rows], ref64) <= R.bound(R.rel_err(XR.normals(w, np.float32), ref64)), (c, m)
        seen["random"] += int(ref["random"].sum())
        seen["noisy"] += int((~ref["random"]).sum())
        seen["clamped"] += int((np.abs(ref["out"]) == 1).sum())
        seen["count0"] += int((count == 0).sum())
        total, calls, x = ref["total"], ref["calls"], ref["x"]
    return seen


@pytest.mark.parametrize("n,S", SHAPES)
def test_five_calls_equal_the_law_exactly(n, S):
    """Members cycling through all five noise modes, three anneal modes and three start_steps (0; inside the first
    call's rows; past two calls): actions, OU state, scale, counters and draws over 5 consecutive calls."""
    starts = (0, n // 2 + 2, 2 * n + 2)
    if S == 1:  # one member: every mode in turn, its first call wholly inside the random phase
        seen = [_sequence(n, 1, (k,), (n + 2,)) for k in KINDS]
        assert sum(s["all_random_ou"] for s in seen) >= 1
        seen = {k: sum(s[k] for s in seen) for k in seen[0]}
    else:
        seen = _sequence(n, S, KINDS, starts)
    assert seen["random"] > 0 and seen["noisy"] > 0 and seen["count0"] >= 1


@pytest.mark.parametrize("n", [20, 65])
def test_member_of_a_mixed_call_equals_its_own_call(n):
    """Composition: member j of a 3-member call (gaussian / OU / uniform, different seeds, start_steps and schedules)
    equals a single-member call for j on j's observation rows, bit for bit in out, x, z_out and scale_out, over 3
    calls; j's draws do not depend on where j stands."""
    b3 = bank(3)
    kinds = ("gaussian", "ornstein-uhlenbeck", "uniform")
    pk, _ = members_for(3, kinds, start=(0, n // 2, 0))
    pop = X.Explorer(b3, pk, n, backend="hip", keep_draws=True)
    solos = []
    for j in range(3):
        b1 = PolicyBank(1, DEV)
        b1.replace(0, b3.state_dict(j))
        solos.append(X.Explorer(b1, [pk[j]], n, backend="hip", keep_draws=True))
    for c in range(3):
        obs = observations(3 * n, 80 + c)
        count = torch.tensor([n, max(n - 3 * c, 1), n - 1], dtype=torch.int32, device=DEV)
        out = pop.explore(obs, nan_fill(pop, 4), 0, count=count)
        for j, solo in enumerate(solos):
            rows = slice(j * n, (j + 1) * n)
            own = solo.explore(obs[rows].clone(), nan_fill(solo, 4), 0, count=count[j:j + 1].clone())
            torch.cuda.synchronize()
            assert np.array_equal(bits(out[rows]), bits(own)), (c, j)
            assert np.array_equal(bits(pop.x[rows]), bits(solo.x)) and np.array_equal(bits(pop.z[rows]), bits(solo.z))
            assert np.array_equal(bits(pop.scale[j:j + 1]), bits(solo.scale))
            assert pop.total[j] == solo.total[0] and pop.calls[j] == solo.calls[0] == c + 1
    assert pop.x[n:2 * n].abs().sum() > 0


def test_permuting_rows_between_slots_of_equal_weights_changes_nothing():
    """Three slots hold one actor; the rows' policy ids are permuted among them (so the grouping's order and the tiles
    differ): out, x and z_out keep their bits.  A row's draw is keyed by its identity, not its position in order."""
    n, S = 70, 3
    b = bank(S, same=True)
    pk, _ = members_for(S, ("ornstein-uhlenbeck", "gaussian", "uniform"), start=(0, 40, 0))
    base = (torch.arange(S * n) // n).to(torch.int32)
    perm = base[torch.randperm(S * n, generator=torch.Generator().manual_seed(3))]
    obs = observations(S * n, 9)
    res = []
    for policy in (base, perm):
        ex = X.Explorer(b, pk, n, backend="hip", keep_draws=True, policy=policy.to(DEV))
        outs = []
        for c in range(2):
            outs.append(bits(ex.explore(obs, nan_fill(ex, 4), 0)).copy())
        torch.cuda.synchronize()
        res.append((outs, bits(ex.x), bits(ex.z)))
    assert not np.array_equal(base.numpy(), perm.numpy())
    for a, p in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, p)
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])


def test_non_finite_observation_rows_are_contained():
    """One NaN and one Inf observation row (+Inf and -Inf in two columns; in different members, OU and gaussian, past
    the random phase): their four actions are non-finite, every other row's actions and OU state, and all counters, equal a clean run's."""
    n, S = 20, 3
    b = bank(S)
    pk, _ = members_for(S, ("ornstein-uhlenbeck", "gaussian", "ornstein-uhlenbeck"))
    clean_obs = observations(S * n, 21)
    bad_obs = clean_obs.clone()
    bad_obs[5, 3] = float("nan")
    bad_obs[47, 0], bad_obs[47, 1] = float("inf"), float("-inf")  # Inf - Inf in half the hidden units: NaN actions
    runs = []
    for obs in (clean_obs, bad_obs):
        ex = X.Explorer(b, pk, n, backend="hip", keep_draws=True)
        out = None
        for c in range(2):
            out = ex.explore(obs, nan_fill(ex, 4), 0)
        torch.cuda.synchronize()
        runs.append((out.cpu(), ex.x.cpu(), ex.total.cpu(), ex.calls.cpu(), ex.scale.cpu()))
    (o0, x0, t0, c0, s0), (o1, x1, t1, c1, s1) = runs
    good = torch.ones(S * n, dtype=torch.bool)
    good[5] = good[47] = False
    assert not torch.isfinite(o1[5]).any() and not torch.isfinite(o1[47]).any()
    assert torch.isfinite(o1[good]).all() and np.array_equal(bits(o1[good]), bits(o0[good]))
    assert np.array_equal(bits(x1[good]), bits(x0[good])) and torch.isfinite(x1[good]).all()
    assert torch.equal(t0, t1) and torch.equal(c0, c1) and np.array_equal(bits(s0), bits(s1))


def test_out_of_contract_device_values_are_clamped():
    """A negative total or count and a count above n are clamped (include/hockey_explore.h): the call equals the one
    with the clamped values."""
    n, S = 20, 3
    b = bank(S)
    pk, _ = members_for(S, ("gaussian", "uniform", "ornstein-uhlenbeck"), start=(0, 10, 0))
    obs = observations(S * n, 31)
    res = []
    for total, count in (([-5, 3, 7], [-2, n + 9, 4]), ([0, 3, 7], [0, n, 4])):
        ex = X.Explorer(b, pk, n, backend="hip", keep_draws=True)
        ex.total.copy_(torch.tensor(total))
        out = ex.explore(obs, nan_fill(ex, 4), 0, count=torch.tensor(count, dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        res.append((bits(out), bits(ex.x), ex.total.tolist(), ex.calls.tolist()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert res[0][2] == res[1][2] == [0, 3 + n, 11] and res[0][3] == [1, 1, 1]
