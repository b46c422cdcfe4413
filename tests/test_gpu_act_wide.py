"""hkl_act_wide (csrc/hk_learner.hip) through PolicyBank capacities above 64, on the GPU.

The wide acting kernel runs hkl_act's acting tile (one __device__ body), so every comparison here is bitwise
(torch.equal over the whole output buffer, sentinels included): against narrow banks through hkl_act, never against a
tolerance.  hkl_act's own accuracy against a float64 forward is tests/test_gpu_policy_bank.py's subject.

The graph-replay test of the wide path is test_wide_bank_graph_replay in tests/test_gpu_population_selfplay.py: a
capture takes a stream from torch's pool, and tests/test_gpu_facade.py's blocked-stream test, which runs between the
two files, depends on which pooled streams the process has handed out before it.  This file takes none.
"""
import functools

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import learner_ref as R  # noqa: E402
from hockey_amd.policy_bank import PolicyBank  # noqa: E402

DEV = "cuda:0"
SENTINEL = -7.5
INT32_MIN = -2 ** 31


@functools.lru_cache(maxsize=None)
def _nets(K, seed=18):
    g = torch.Generator().manual_seed(seed + K)
    return tuple(R._net(g, 18, 4) for _ in range(K))


def _obs(n, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    return (torch.rand((n, 18), generator=g) * 2 - 1).to(DEV)


def _out(n):
    return torch.full((n, 8), SENTINEL, device=DEV)


@functools.lru_cache(maxsize=None)
def _bank130():
    nets = _nets(130)
    wide = PolicyBank(130, DEV, wide=True)
    wide.replace_many(range(130), nets)
    narrow = []
    for c in range(3):  # slots [64 c, 64 c + 64) of the 130: the last bank holds 2, so that K and K + 5 miss it too
        chunk = nets[64 * c:64 * c + 64]
        b = PolicyBank(len(chunk), DEV)
        b.replace_many(range(len(chunk)), chunk)
        narrow.append(b)
    return wide, narrow


def _narrow_expected(narrow, obs, policy):
    """hkl_act over slots [64 c, 64 c + 64) with policy - 64 c: an id outside a chunk is outside that bank's range
    and does not act there (hkl_act's own guard).  The shift is taken in int64 and an id that would leave int32
    (INT32_MIN - 64) is non-acting anyway, so negative ids become -1."""
    exp = _out(obs.shape[0])
    for c, b in enumerate(narrow):
        p = policy.to(torch.int64) - 64 * c
        p = torch.where(p >= 0, p, torch.full_like(p, -1)).to(torch.int32)
        b.act(obs, p, out=exp, out_col=4, backend="hip")
    return exp


def _policy130(n=1000):
    """Rows per policy: 0 (policy 7), 1 (policy 3), 63 (policy 64), 64 (policy 129), 65 (policy 63), 200 > 128
    (policy 100); ids -1, K, K + 5 and INT32_MIN sprinkled in; the rest spread over the other policies.  Shuffled."""
    ids = [3] + [64] * 63 + [129] * 64 + [63] * 65 + [100] * 200 + [-1] * 5 + [130] * 3 + [135] * 3 + [INT32_MIN] * 3
    others = [k for k in range(130) if k not in (7, 3, 64, 129, 63, 100)]
    i = 0
    while len(ids) < n:
        ids.append(others[i % len(others)])
        i += 1
    p = torch.tensor(ids, dtype=torch.int64)
    p = p[torch.randperm(n, generator=torch.Generator().manual_seed(4))]
    counts = torch.bincount(p[(p >= 0) & (p < 130)], minlength=130)
    assert counts[7] == 0 and counts[3] == 1 and counts[64] == 63 and counts[129] == 64 and counts[63] == 65
    assert counts[100] > 128
    return p.to(torch.int32).to(DEV)


def test_wide_bank_is_hkl_act_bit_for_bit():
    wide, narrow = _bank130()
    n = 1000
    obs, policy = _obs(n), _policy130(n)
    got = wide.act(obs, policy, out=_out(n), out_col=4, backend="hip")
    exp = _narrow_expected(narrow, obs, policy)
    assert torch.equal(got, exp)
    acting = (policy >= 0) & (policy < 130)
    assert torch.all(got[acting][:, 4:] != SENTINEL) and torch.all(got[~acting] == SENTINEL)
    assert torch.all(got[:, :4] == SENTINEL)


@pytest.mark.parametrize("case", ["one_policy", "all_minus_one", "n1", "n65"])
def test_wide_bank_extremes(case):
    wide, narrow = _bank130()
    if case == "one_policy":
        n, policy = 1000, torch.full((1000,), 77, dtype=torch.int32, device=DEV)
    elif case == "all_minus_one":
        n, policy = 1000, torch.full((1000,), -1, dtype=torch.int32, device=DEV)
    elif case == "n1":
        n, policy = 1, torch.tensor([129], dtype=torch.int32, device=DEV)
    else:
        n, policy = 65, (torch.arange(65, dtype=torch.int32, device=DEV) * 2) % 130
    obs = _obs(n, seed=len(case))
    got = wide.act(obs, policy, out=_out(n), out_col=4, backend="hip")
    assert torch.equal(got, _narrow_expected(narrow, obs, policy))
    if case == "all_minus_one":
        assert torch.all(got == SENTINEL)
    else:
        assert torch.all(got[:, 4:] != SENTINEL)


def test_wide_bank_every_row_its_own_policy():
    """1 000 rows on 1 000 distinct policies of a K = 1 024 bank whose slots copy 4 weight sets (slot k holds set
    k % 4): equal to a 4-slot bank through hkl_act with policy % 4."""
    nets = _nets(4)
    wide = PolicyBank(1024, DEV, wide=True)
    wide.replace_many(range(1024), [nets[k % 4] for k in range(1024)])
    small = PolicyBank(4, DEV)
    small.replace_many(range(4), nets)
    n = 1000
    policy = torch.randperm(1024, generator=torch.Generator().manual_seed(9))[:n].to(torch.int32).to(DEV)
    obs = _obs(n, seed=3)
    got = wide.act(obs, policy, out=_out(n), out_col=4, backend="hip")
    exp = small.act(obs, policy % 4, out=_out(n), out_col=4, backend="hip")
    assert torch.equal(got, exp) and torch.all(got[:, 4:] != SENTINEL)


def test_wide_bank_no_rows():
    wide, _ = _bank130()
    buf = _out(4)
    out = wide.act(_obs(4)[:0], torch.zeros(4, dtype=torch.int32, device=DEV)[:0], out=buf[:0], out_col=4,
                   backend="hip")
    torch.cuda.synchronize()
    assert out.shape == (0, 8) and torch.all(buf == SENTINEL)


def test_wide_bank_at_the_capacity_limit():
    """Capacity 4 096 with slots 0, 63, 64 and 4 095 holding one weight set, rows on exactly those: PolicyBank(1)."""
    net = _nets(1)[0]
    wide = PolicyBank(4096, DEV, wide=True)
    wide.replace_many([0, 63, 64, 4095], [net] * 4)
    one = PolicyBank(1, DEV)
    one.replace(0, net)
    n = 300
    policy = torch.tensor([0, 63, 64, 4095], dtype=torch.int32).repeat(n // 4).to(DEV)
    obs = _obs(n, seed=6)
    got = wide.act(obs, policy, out=_out(n), out_col=4, backend="hip")
    exp = one.act(obs, torch.zeros(n, dtype=torch.int32, device=DEV), out=_out(n), out_col=4, backend="hip")
    assert torch.equal(got, exp) and torch.all(got[:, 4:] != SENTINEL)


def test_narrow_bank_is_left_alone():
    """A PolicyBank(40) call (hkl_act) gives the bytes the same 40 actors give through a wide bank."""
    nets = _nets(130)[:40]
    small = PolicyBank(40, DEV)
    small.replace_many(range(40), nets)
    wide = PolicyBank(200, DEV, wide=True)
    wide.replace_many(range(40), nets)
    n = 777
    g = torch.Generator().manual_seed(2)
    policy = torch.randint(-1, 40, (n,), generator=g, dtype=torch.int32).to(DEV)
    obs = _obs(n, seed=8)
    a = small.act(obs, policy, out=_out(n), out_col=4, backend="hip")
    b = wide.act(obs, policy, out=_out(n), out_col=4, backend="hip")
    assert torch.equal(a, b) and torch.all(a[policy >= 0][:, 4:] != SENTINEL)
