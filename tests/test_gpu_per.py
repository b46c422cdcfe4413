"""The device-side prioritized replay sampler (hkl_per_* of include/hockey_learner.h, csrc/hk_learner.hip;
hockey_amd.td3.DevicePrioritizedRing) against the numpy float64 reference of tests/per_ref.py, which
tests/test_per_ref.py pins to PrioritizedRing on the CPU.

With BLK = hkl_per_block(): capacities 1, BLK - 1, BLK, BLK + 1 and 3 BLK + 17, each full, filled to mid-block and to
a block edge; batches 1, 257 and 768 (a longer list of draws is fed as one batch of each small size and batches of 768).
The raw-ABI tests hold only a weights array and the sampler's own state, no transition columns.

* exact sampling: weights k 2^-10 whose total is a power of two make every float64 partial sum exact in any order, so
  the slots must equal the reference's, every one, for u = 0, the largest double below 1, every cdf[j] / T, its
  predecessor and 64 random values; the block sums must equal numpy's bit for bit;
* general weights: lognormal float32 weights, with and without 30 % of the slots at 1e8, the first slots NaN, +-inf,
  -1, 0, 1e-9, 1e-6: per_ref.check_general's rule with eps = 2 size 2^-53 T, at most 1 of 4096 draws in the band;
* device RNG: with u == NULL the slots are the reference's for the uniforms of learner_ref's Philox, and the noise is
  hkl_sample's bit for bit;
* write-back: numpy's w[idx] = clip(td) bit for bit under heavy duplication, then an exact-sampling pass that a stale
  block sum would fail; pushes that wrap, before and after the ring is full, interleaved with updates: w bit for bit
  the CPU PrioritizedRing's and exact sampling after every step; three marked slots past 2^24;
* the fused learner on a DevicePrioritizedRing against the fused learner on a PrioritizedRing (same slots and noise),
  graph replay against eager launches bit for bit on the learner's own Philox stream, and a short train() run.

Importance weights.  err = max|iw - iw_64| / max|iw_64| against per_ref.importance, bound learner_ref.bound:
err <= max(4 err_fp32_eager, 4 * 2^-24) with err_fp32_eager the error of torch's float32 evaluation of the same
expressions on the GPU (learner_hip.py's eager branch).  Measured on an MI355X (the kernel evaluates in float64 and
rounds once):

    batch  err       err_fp32_eager  err / bound
    1      0.00e+00  0.00e+00        0.00
    257    2.94e-08  7.18e-08        0.10
    768    2.98e-08  9.98e-08        0.07
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import learner_ref as R  # noqa: E402
import per_ref as P  # noqa: E402
from hockey_amd import learner_hip as LH  # noqa: E402
from hockey_amd.td3 import TD3, DevicePrioritizedRing, Learner, PrioritizedRing, TD3Config, train  # noqa: E402
from test_gpu_learner import LOSS_RTOL, PARAM_ATOL  # noqa: E402

DEV = "cuda:0"
BATCHES = (1, 257, 768)
SEED = 0x5EED5EED1234


def capacities():
    return P.capacities(LH.lib().hkl_per_block())


def fills(cap):
    return P.fills(cap, LH.lib().hkl_per_block())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


class Raw:
    """The sampler's state around a bare weights array, driven through the C ABI."""

    def __init__(self, w, size):
        self.L = LH.lib()
        self.blk = self.L.hkl_per_block()
        self.cap, self.size, self.pos = len(w), int(size), int(size) % len(w)
        nblk = -(-self.cap // self.blk)
        self.w = torch.from_numpy(np.asarray(w, np.float32)).to(DEV)
        self.size_t = torch.tensor(self.size, dtype=torch.int64, device=DEV)
        self.bsum = torch.full((nblk,), float("nan"), dtype=torch.float64, device=DEV)
        self.bpre = torch.full((nblk,), float("nan"), dtype=torch.float64, device=DEV)
        self.bmax = torch.full((nblk,), float("nan"), dtype=torch.float32, device=DEV)
        self.last = torch.zeros(self.cap, dtype=torch.int32, device=DEV)
        self.bown = torch.zeros(nblk, dtype=torch.int32, device=DEV)
        p = LH._p
        self.per = LH.Per(self.cap, p(self.w), p(self.size_t), p(self.bsum), p(self.bmax), p(self.bpre), p(self.last),
                          p(self.bown))
        self.refresh()

    def refresh(self, lo=0, n=None):
        LH._check(self.L.hkl_per_refresh(self.per, lo, self.cap - lo if n is None else n, _st()), "hkl_per_refresh")

    def push(self, n):
        after = min(self.size + n, self.cap)
        LH._check(self.L.hkl_per_push(self.per, self.pos, n, after, _st()), "hkl_per_push")
        self.pos, self.size = (self.pos + n) % self.cap, after
        self.size_t.fill_(after)

    def sample(self, batch, u=None, ctr=None, beta=0.15, noise=False, iw=True):
        """(idx, iw, noise) as numpy arrays; every output starts as NaN / -1."""
        idx = torch.full((batch,), -1, dtype=torch.int64, device=DEV)
        iw_t = torch.full((batch,), float("nan"), device=DEV) if iw else None
        nz = torch.full((batch, 4), float("nan"), device=DEV) if noise else None
        u_t = None if u is None else torch.from_numpy(np.ascontiguousarray(u, np.float64)).to(DEV)
        c_t = None if ctr is None else torch.tensor(ctr, dtype=torch.int64, device=DEV)
        p = LH._p
        io = LH.PerSampleIO(self.per, batch, SEED, p(c_t), p(u_t), p(idx), p(nz), 0.2, 0.3, p(iw_t), beta)
        LH._check(self.L.hkl_per_sample(io, _st()), "hkl_per_sample")
        torch.cuda.synchronize()
        return idx.cpu().numpy(), None if iw_t is None else iw_t.cpu().numpy(), None if nz is None else nz.cpu().numpy()

    def draws(self, u):
        """The slots of a list of uniforms of any length, fed as batches of 1, 257 and then 768 (padded with 0.5)."""
        u = np.asarray(u, np.float64)
        sizes = [1, 257] + [768] * max(0, -(-(len(u) - 258) // 768))
        pad = np.concatenate([u, np.full(sum(sizes) - len(u), 0.5)])
        out, o = [], 0
        for b in sizes:
            out.append(self.sample(b, pad[o:o + b], iw=False)[0])
            o += b
        return np.concatenate(out)[:len(u)]

    def update(self, idx, td):
        i = torch.from_numpy(np.ascontiguousarray(idx, np.int64)).to(DEV)
        t = torch.from_numpy(np.ascontiguousarray(td, np.float32)).to(DEV)
        io = LH.PerUpdateIO(self.per, len(idx), LH._p(i), LH._p(t))
        LH._check(self.L.hkl_per_update(io, _st()), "hkl_per_update")
        torch.cuda.synchronize()

    def check_state(self):
        """Block sums / maxima equal numpy's over the current weights (exact-sum weights: bit for bit) and the
        scratch words are back at zero."""
        w = self.w.cpu().numpy()
        p = P.sanitised(w, self.size)
        nblk = len(self.bsum)
        want = np.array([p[b * self.blk:(b + 1) * self.blk].sum() for b in range(nblk)])
        assert np.array_equal(self.bsum.cpu().numpy().view(np.uint64), want.view(np.uint64))
        wmax = np.array([w[b * self.blk:(b + 1) * self.blk].max() for b in range(nblk)])
        assert np.array_equal(self.bmax.cpu().numpy(), wmax)
        assert int(self.last.abs().max()) == 0 and int(self.bown.abs().max()) == 0


def _assert_exact(raw, seed, limit=None):
    w = raw.w.cpu().numpy()
    u = P.exact_draws(w, raw.size, seed, limit=limit)
    got, want = raw.draws(u), P.sample(w, raw.size, u)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (raw.cap, raw.size, bad[:8], u[bad[:8]], got[bad[:8]], want[bad[:8]])


# ------------------------------------------------------------------------------------------------------ sampling
@pytest.mark.parametrize("ci", range(5))
def test_exact_sampling_equals_reference_at_every_capacity_and_fill(ci):
    cap = capacities()[ci]
    for size in fills(cap):
        raw = Raw(P.dyadic_weights(size, 100 + ci, cap), size)
        raw.check_state()
        _assert_exact(raw, 7)


@pytest.mark.parametrize("regime", ["a", "b"])
def test_general_weights_within_the_summation_bound(regime):
    cap = capacities()[4]
    for size in (cap, fills(cap)[0]):
        w = np.full(cap, 1e8, np.float32)
        w[:size] = P.general_weights(size, regime, 11)
        raw = Raw(w, size)
        u = np.random.default_rng(12 + size).random(4096)
        idx = raw.draws(u)
        band = P.check_general(w, size, u, idx)
        print(f"general weights regime {regime} size {size}: draws in the excluded band {band}")
        assert band <= 1


def _philox_u(batch, ctr):
    r = R.philox4x32_10(np.uint64(SEED), R._sample_counters(batch, ctr)).astype(np.uint64)
    return (((r[:, 0] << np.uint64(32)) | r[:, 1]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


@pytest.mark.parametrize("batch", BATCHES)
def test_device_rng_draws_the_reference_slots_and_hkl_sample_noise(batch):
    cap = capacities()[4]
    size = fills(cap)[0]
    w = P.dyadic_weights(size, 21, cap)
    raw = Raw(w, size)
    for ctr in (0, (1 << 33) + 5):
        idx, _, noise = raw.sample(batch, ctr=ctr, noise=True, iw=False)
        assert np.array_equal(idx, P.sample(w, size, _philox_u(batch, ctr))), ctr
        i2 = torch.full((batch,), -1, dtype=torch.int64, device=DEV)
        n2 = torch.full((batch, 4), float("nan"), device=DEV)
        c_t = torch.tensor(ctr, dtype=torch.int64, device=DEV)
        sio = LH.SampleIO(batch, SEED, LH._p(c_t), LH._p(raw.size_t), LH._p(i2), LH._p(n2), 0.2, 0.3)
        LH._check(raw.L.hkl_sample(sio, _st()), "hkl_sample")
        torch.cuda.synchronize()
        assert np.array_equal(noise.view(np.uint32), n2.cpu().numpy().view(np.uint32)), ctr


@pytest.mark.parametrize("batch", BATCHES)
def test_importance_weights_within_the_fp32_bound(batch):
    cap = capacities()[4]
    size = fills(cap)[0]
    w = np.full(cap, 1e8, np.float32)
    w[:size] = P.general_weights(size, "a", 31)
    w[:7] = 1.0  # a NaN raw weight in the batch makes every importance weight NaN, in torch's expressions too
    raw = Raw(w, size)
    beta = 0.15
    idx, iw, _ = raw.sample(batch, u=np.random.default_rng(32).random(batch), beta=beta)
    ref = P.importance(w, idx, size, beta)
    wb = raw.w[torch.from_numpy(idx).to(DEV)]  # learner_hip.py's eager expressions, float32 on the GPU
    e = (1.0 / ((wb / wb.sum()) * raw.size_t)) ** beta
    e = (e / e.max()).cpu().numpy()
    err, err32 = R.rel_err(iw, ref), R.rel_err(e, ref)
    print(f"importance weights batch {batch}: err {err:.3e} err_fp32_eager {err32:.3e} err/bound {err / R.bound(err32):.2f}")
    assert err <= R.bound(err32), (err, err32)
    idx_t, again = torch.from_numpy(idx).to(DEV), torch.full((batch,), float("nan"), device=DEV)
    io = LH.PerSampleIO(raw.per, batch, 0, None, None, LH._p(idx_t), None, 0.0, 0.0, LH._p(again), beta)
    LH._check(raw.L.hkl_per_weights(io, _st()), "hkl_per_weights")
    torch.cuda.synchronize()
    assert np.array_equal(again.cpu().numpy().view(np.uint32), iw.view(np.uint32))  # the same kernel, the same bits


# ------------------------------------------------------------------------------------------------------ write-back
def test_write_back_last_occurrence_wins_and_block_sums_follow():
    cap = capacities()[4]
    w = P.dyadic_weights(cap, 41)
    raw = Raw(w, cap)
    rng = np.random.default_rng(42)
    hot = np.array([0, raw.blk - 1, raw.blk, 2 * raw.blk + 5, cap - 1])
    idx = np.concatenate([rng.choice(hot, 150), rng.choice(cap, 106, replace=False)])
    rng.shuffle(idx)
    td = np.exp(rng.normal(0, 3, 256)).astype(np.float32)
    td[::5] = np.float32(1e-7) * rng.random(52).astype(np.float32)  # below the floor
    td[1::5] = np.float32(1e6) * (1 + rng.random(51).astype(np.float32))  # above the ceiling
    raw.update(idx, td)
    want = P.write_back(w.copy(), idx, td)
    assert np.array_equal(raw.w.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert (want == 1e6).any() and (want == np.float32(1e-6)).any()
    assert int(raw.last.abs().max()) == 0 and int(raw.bown.abs().max()) == 0
    # dyadic values back into the same slots, the last one chosen so that the total is a power of two again
    k = rng.integers(1, 4096, 256).astype(np.int64)
    final = want.copy()
    final[idx] = (k * 2.0 ** -10).astype(np.float32)  # numpy's own last-wins
    rest = int(round(float(np.delete(final.astype(np.float64), idx[-1]).sum() * 1024)))
    k[-1] = (1 << rest.bit_length()) - rest
    assert 1 <= k[-1] < 1 << 24
    td2 = (k * 2.0 ** -10).astype(np.float32)
    raw.update(idx, td2)
    final = P.write_back(want.copy(), idx, td2)
    assert np.array_equal(raw.w.cpu().numpy().view(np.uint32), final.view(np.uint32))
    total = float(final.astype(np.float64).sum())
    assert np.log2(total) == int(np.log2(total))
    raw.check_state()
    _assert_exact(raw, 43)


def test_pushes_that_wrap_interleaved_with_updates_equal_cpu_ring():
    cap = capacities()[4]
    raw = Raw(np.full(cap, 1e8, np.float32), 0)
    ring = PrioritizedRing(cap, device="cpu")
    rng = np.random.default_rng(51)
    z = lambda n, *s: torch.zeros((n,) + s)  # noqa: E731
    # 2200 slots filled; a push that fills the ring and wraps; pushes on the full ring, the last one wrapping again
    for step, n in enumerate([700, 1500, 900, 400, 2900, 1]):
        ring.push(z(n, 18), z(n, 4), z(n), z(n, 18), z(n))
        raw.push(n)
        assert (raw.size, raw.pos) == (ring.size, ring.pos)
        assert np.array_equal(raw.w.cpu().numpy().view(np.uint32), ring.w.numpy().view(np.uint32)), step
        raw.check_state()
        _assert_exact(raw, 60 + step, limit=300)
        idx = rng.integers(0, raw.size, 257)
        idx[:30] = idx[30]
        td = (rng.integers(1, 1 << 16, 257) * 2.0 ** -10).astype(np.float32)  # dyadic: every sum stays exact
        td[7] = np.float32(3e5)  # the largest weight, which the next push spreads
        ring.last = torch.from_numpy(idx)
        ring.update_priorities(torch.from_numpy(td))
        raw.update(idx, td)
        assert np.array_equal(raw.w.cpu().numpy().view(np.uint32), ring.w.numpy().view(np.uint32)), step
        raw.check_state()
        _assert_exact(raw, 70 + step, limit=300)
    assert ring.size == cap


def test_marked_slots_past_2_to_24_are_reached():
    blk = LH.lib().hkl_per_block()
    cap = 2 ** 24 + blk + 3
    w = np.full(cap, 2.0 ** -10, np.float32)
    marked = np.array([2 ** 24 + 1, 2 ** 24 + blk - 1, cap - 1])
    w[marked] = 2.0 ** -4
    raw = Raw(w, cap)
    cdf = np.cumsum(w.astype(np.float64))
    T = cdf[-1]
    lo, hi = cdf[marked - 1], cdf[marked]
    inside = np.concatenate([(lo + (hi - lo) * f) / T for f in (0.25, 0.5, 0.75)])
    edges = np.concatenate([lo / T, np.nextafter(lo / T, 0), hi[:-1] / T, np.nextafter(hi / T, 0)])
    u = np.concatenate([inside, edges])
    got = raw.draws(u)
    want = np.minimum(np.searchsorted(cdf, u * T, side="right"), cap - 1)
    assert np.array_equal(got, want)
    assert np.array_equal(got[:9], np.tile(marked, 3))


# ------------------------------------------------------------------------------------------------------ the ring class
def _filled(ring, cap, seed):
    g = torch.Generator().manual_seed(seed)
    cols = (torch.randn(cap, 18, generator=g), torch.rand(cap, 4, generator=g) * 2 - 1, torch.randn(cap, generator=g),
            torch.randn(cap, 18, generator=g), (torch.rand(cap, generator=g) < 0.1).float())
    ring.push(*(t.to(DEV) for t in cols))
    return ring


def test_device_ring_samples_and_writes_back_like_prioritized_ring():
    cap = capacities()[4]
    w = torch.from_numpy(P.dyadic_weights(cap, 81)).to(DEV)
    a, b = _filled(PrioritizedRing(cap, device=DEV), cap, 1), _filled(DevicePrioritizedRing(cap, device=DEV), cap, 1)
    assert torch.equal(a.w, b.w)
    a.w.copy_(w)
    b.w.copy_(w)
    b.refresh()
    for batch in BATCHES:
        torch.manual_seed(batch)
        sa = a.sample(batch)
        torch.manual_seed(batch)
        sb = b.sample(batch)
        assert torch.equal(a.last, b.last)
        for x, y in zip(sa[:5], sb[:5]):
            assert torch.equal(x, y)
        # against torch's float32 chain (four roundings, a pow, the maximum's own error): 8 x 2^-24 of the top weight 1
        assert R.rel_err(sb[5], sa[5].double()) <= 8 * 2.0 ** -24
        td = torch.rand(batch, device=DEV) * 4
        a.update_priorities(td)
        b.update_priorities(td)
        assert torch.equal(a.w, b.w)


# ------------------------------------------------------------------------------------------------------ the learner
def test_fused_learner_on_device_ring_matches_fused_learner_on_prioritized_ring():
    from hockey_amd.learner_hip import FusedLearner

    cfg = TD3Config(prioritized_replay=True)
    cap, B = 20_000, 1024
    out = []
    for cls in (PrioritizedRing, DevicePrioritizedRing):
        ring = _filled(cls(cap, device=DEV, beta=cfg.beta), cap, 2)
        w0 = P.general_weights(cap, "b", 91)
        w0[:7] = 1.0
        ring.w.copy_(torch.from_numpy(w0))
        if cls is DevicePrioritizedRing:
            ring.refresh()
        agent = TD3(cfg, device=DEV, seed=3)
        fl = FusedLearner(agent, ring, B)
        acc = torch.zeros(4, dtype=torch.float64, device=DEV)
        fl.set_loss_accumulator(acc)
        g = torch.Generator().manual_seed(4)
        for k in range(6):
            idx = torch.randint(0, cap, (B,), generator=g)
            idx[:50] = idx[50]
            fl.update(k % 2 == 1, idx=idx.to(DEV), noise=(torch.randn(B, 4, generator=g) * 0.2).to(DEV))
        torch.cuda.synchronize()
        params = torch.cat([p.detach().flatten() for m in (agent.actor, agent.critic, agent.target_actor,
                                                           agent.target_critic) for p in m.parameters()])
        out.append((acc.cpu(), params, ring.w.clone()))
    (acc_a, par_a, w_a), (acc_b, par_b, w_b) = out
    for j in (0, 1):  # mean critic / actor loss over the updates
        la, lb = float(acc_a[j] / acc_a[j + 2]), float(acc_b[j] / acc_b[j + 2])
        assert abs(la - lb) <= LOSS_RTOL * max(1.0, abs(la)), (j, la, lb)
    assert float((par_a - par_b).abs().max()) <= PARAM_ATOL
    assert float(((w_a - w_b).abs() / w_a.abs().clamp_min(1.0)).max()) <= 1e-4
    assert int((w_b != torch.from_numpy(w0).to(DEV)).sum()) > 4000  # the priorities were written back


def test_device_per_graph_replay_equals_eager_bit_for_bit():
    """After test_fused_graph_replay_equals_fused_eager: Learner's captured update pairs against the same updates
    launched one by one, here on distinct ring entries with the slots, noise and importance weights drawn from the
    learner's Philox stream and the priorities written back every update."""
    res = []
    for graphs in (False, True):
        cfg = TD3Config(prioritized_replay=True)
        agent = TD3(cfg, device=DEV, seed=0)
        ring = _filled(DevicePrioritizedRing(4096, device=DEV, beta=cfg.beta), 4096, 5)
        lr = Learner(agent, ring, 512, graphs=graphs, warm_pairs=1, fused=True)
        for _ in range(3):
            lr.run(8)
        assert agent.train_step == 24 and (lr.graph is not None) == graphs
        torch.cuda.synchronize()
        assert int(lr.fused.sample_counter) == 24
        res.append((torch.cat([p.detach().flatten() for m in (agent.actor, agent.critic, agent.target_actor,
                                                              agent.target_critic) for p in m.parameters()]),
                    ring.w.clone(), ring._bsum.clone()))
    assert torch.equal(res[0][0], res[1][0]), (res[0][0] - res[1][0]).abs().max()
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    assert int((res[0][1] != 1e8).sum()) > 0


def test_train_with_the_device_per_sampler():
    from hockey_amd import _native as N
    from hockey_amd.constants import Mode
    from hockey_amd.vec_env import VecHockeyEnv

    env = VecHockeyEnv(64, mode=Mode.NORMAL, device=DEV, policies=("external", "external"), auto_reset=False, seed=0)
    agent, stats = train(n_arenas=64, rounds=2, per_sampler="device", env=env, device=DEV,
                         cfg=TD3Config(prioritized_replay=True, max_steps=40, start_steps=0, batch_size=256))
    ring = agent._fused_learner.ring
    assert isinstance(ring, DevicePrioritizedRing) and stats["updates"] > 0
    cnt = env.counters()
    env.close()
    assert int(cnt[N.CNT_OVERFLOW]) == 0
    assert bool(torch.isfinite(ring.w).all())
    assert int((ring.w != 1e8).sum()) > 0
