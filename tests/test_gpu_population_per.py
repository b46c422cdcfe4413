"""Prioritized replay in a population on the GPU: the grouped hkl_per_* kernels (include/hockey_learner.h,
csrc/hk_learner.hip), hockey_amd.population.PopulationPrioritizedRing and the PopulationLearner / train_population
built on them.

The grouped calls promise member m the single call's results bit for bit, whatever the other members are.  Every
comparison here is therefore bitwise equality against single-member twins -- the hkl_per_* calls on a
DevicePrioritizedRing, and FusedLearner on one -- which tests/test_gpu_per.py already holds to the float64 reference
of tests/per_ref.py; the push test compares the weights with per_ref.RefRing as well.  Floating-point tensors are
compared through their bit patterns, so NaN weights (per_ref.general_weights puts one in slot 0) count as equal.

Shapes: capacity 3 * 1024 + 17 (a ragged last block, and a member stride that is no multiple of the float4 the
kernels read) with S = 3 members filled to mid-block, to a block edge and completely; S = 64 at capacity 1025 and
S = 1 at capacity 1, the ends of the member range.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import per_ref as P  # noqa: E402
from hockey_amd import learner_hip as LH  # noqa: E402
from hockey_amd.population import PopulationLearner, PopulationPrioritizedRing, train_population  # noqa: E402
from hockey_amd.td3 import TD3, DevicePrioritizedRing, ReplayRing, TD3Config  # noqa: E402
from test_gpu_population import _cfg, _state, _transitions  # noqa: E402

DEV = "cuda:0"
BATCHES = (1, 257, 768)
BETAS = (0.15, 0.6, -0.3)
_INT = {4: torch.int32, 8: torch.int64}


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _same(a, b):
    """Bitwise equality (NaNs with equal bits included)."""
    if a.dtype.is_floating_point:
        a, b = a.contiguous().view(_INT[a.element_size()]), b.contiguous().view(_INT[b.element_size()])
    return a.shape == b.shape and torch.equal(a, b)


def _dev_array(arr):
    """(device copy of a ctypes array, its address): what a grouped call takes as ``dev``."""
    t = torch.frombuffer(bytearray(arr), dtype=torch.uint8).to(DEV)
    return t, ctypes.c_void_p(t.data_ptr())


def _assert_rings(pop, twins, what, columns=False):
    """Member j's weights, block sums / maxima and fill level equal twin j's; the scratch words are back at zero."""
    torch.cuda.synchronize()
    for j, tw in enumerate(twins):
        m = pop.member(j)
        if not m.prioritized:
            continue
        for k in ("w", "_bsum", "_bmax", "size_t") + (("s", "a", "r", "s2", "d") if columns else ()):
            assert _same(getattr(m, k), getattr(tw, k)), (what, "member", j, k)
    assert int(pop.last.abs().max()) == 0 and int(pop.bown.abs().max()) == 0, what


# ------------------------------------------------------------------------------------------------ sample / update
def _weighted(S, cap):
    """A PopulationPrioritizedRing and S DevicePrioritizedRing twins holding the same weights and fill levels:
    per_ref.general_weights regimes a, b, a, ... (NaN, +-inf, -1, 0, 1e-9, 1e-6 in the first slots; b with 30 % of the
    slots at 1e8) over fill levels mid-block, block edge, full, ..."""
    blk = LH.lib().hkl_per_block()
    fills = P.fills(cap, blk)
    betas = [BETAS[j % 3] for j in range(S)]
    pop = PopulationPrioritizedRing(S, cap, beta=betas, device=DEV)
    twins = []
    for j in range(S):
        size = fills[j % len(fills)]
        w = np.full(cap, 1e8, np.float32)
        w[:size] = P.general_weights(size, "ab"[j % 2], 11 + j)
        wt = torch.from_numpy(w).to(DEV)
        tw = DevicePrioritizedRing(cap, device=DEV, beta=betas[j])
        tw.w.copy_(wt)
        tw.size, tw.pos = size, size % cap
        tw.size_t.fill_(size)
        tw.refresh()
        twins.append(tw)
        pop.member(j).w.copy_(wt)
        pop.size_t[j] = size
        pop.pos_t[j] = size % cap
    pop.refresh()
    return pop, twins, betas


@pytest.mark.parametrize("S,cap", [(3, 3 * 1024 + 17), (64, 1025), (1, 1)])
def test_grouped_sample_weights_and_update_equal_the_single_calls(S, cap):
    """At batches 1, 257 and 768, once from given uniforms and once from Philox (per-member seeds and counters), with
    per-member beta 0.15 / 0.6 / -0.3, noise scale and clip: idx, noise, iw and bpre of hkl_per_sample_group equal
    hkl_per_sample's per member, hkl_per_weights_group equals hkl_per_weights, and after hkl_per_update_group on slots
    with duplicates w, bsum and bmax equal hkl_per_update's while last / bown are all zero.  In the given-uniforms pass
    member 1 has no noise and member 2 no iw (the optional outputs stay optional per member)."""
    L, p = LH.lib(), LH._p
    pop, twins, betas = _weighted(S, cap)
    _assert_rings(pop, twins, "refresh")
    rng = np.random.default_rng(5)
    for batch in BATCHES:
        for philox in (False, True):
            out, ios, keep = [], {"g": [], "t": []}, []
            for j in range(S):
                u = None if philox else torch.from_numpy(rng.random(batch)).to(DEV)
                ctr = torch.tensor((j * 7 + 3) << (30 * (j % 2)), dtype=torch.int64, device=DEV)  # some past 2^32
                keep += [u, ctr]
                sides = {}
                for side, per in (("g", pop.pers[j]), ("t", twins[j].per)):
                    idx = torch.full((batch,), -1, dtype=torch.int64, device=DEV)
                    noise = torch.full((batch, 4), float("nan"), device=DEV)
                    iw = torch.full((batch,), float("nan"), device=DEV)
                    with_noise, with_iw = philox or j != 1, philox or j != 2
                    ios[side].append(LH.PerSampleIO(per, batch, 0x5EED0000 + 977 * j, p(ctr), p(u), p(idx),
                                                    p(noise) if with_noise else None, 0.2 + 0.05 * (j % 3),
                                                    0.3 + 0.1 * (j % 2), p(iw) if with_iw else None, betas[j]))
                    sides[side] = {"idx": idx, "noise": noise, "iw": iw}
                out.append(sides)
            host = (LH.PerSampleIO * S)(*ios["g"])
            dev_t, dev = _dev_array(host)
            LH._check(L.hkl_per_sample_group(host, dev, S, _st()), "hkl_per_sample_group")
            for io in ios["t"]:
                LH._check(L.hkl_per_sample(io, _st()), "hkl_per_sample")
            torch.cuda.synchronize()
            for j in range(S):
                for k in ("idx", "noise", "iw"):
                    assert _same(out[j]["g"][k], out[j]["t"][k]), (batch, philox, "member", j, k)
                assert _same(pop.member(j)._bpre, twins[j]._bpre), (batch, philox, "member", j, "bpre")
                assert int(out[j]["g"]["idx"].min()) >= 0
            # the importance weights alone, every member with iw, into fresh buffers
            again = {s: [torch.full((batch,), float("nan"), device=DEV) for _ in range(S)] for s in "gt"}
            for side in "gt":
                for j in range(S):
                    ios[side][j].iw = p(again[side][j])
            host = (LH.PerSampleIO * S)(*ios["g"])
            dev_t, dev = _dev_array(host)
            LH._check(L.hkl_per_weights_group(host, dev, S, _st()), "hkl_per_weights_group")
            for io in ios["t"]:
                LH._check(L.hkl_per_weights(io, _st()), "hkl_per_weights")
            torch.cuda.synchronize()
            for j in range(S):
                assert _same(again["g"][j], again["t"][j]), (batch, philox, "member", j, "weights alone")
            # the write-back on slots with duplicates, TD errors below the floor and above the ceiling included
            ups = {"g": [], "t": []}
            for j in range(S):
                idx = out[j]["t"]["idx"].clone()
                idx[:batch // 3] = idx[batch // 3]
                td = np.exp(rng.normal(0, 4, batch)).astype(np.float32)
                td[::5] = np.float32(1e-8)
                td[1::7] = np.float32(3e6)
                td_t = torch.from_numpy(td).to(DEV)
                keep += [idx, td_t]
                ups["g"].append(LH.PerUpdateIO(pop.pers[j], batch, p(idx), p(td_t)))
                ups["t"].append(LH.PerUpdateIO(twins[j].per, batch, p(idx), p(td_t)))
            host = (LH.PerUpdateIO * S)(*ups["g"])
            dev_t, dev = _dev_array(host)
            LH._check(L.hkl_per_update_group(host, dev, S, _st()), "hkl_per_update_group")
            for io in ups["t"]:
                LH._check(L.hkl_per_update(io, _st()), "hkl_per_update")
            _assert_rings(pop, twins, ("update", batch, philox))
    if S > 1:  # the members really are different rings
        assert not _same(pop.member(0).w, pop.member(1).w)


# ------------------------------------------------------------------------------------------------ push
def test_ragged_pushes_interleaved_with_updates_equal_single_rings_and_the_reference():
    """S = 3 at capacity 3 * 1024 + 17.  Per-member row counts of a push: 0, 1, exactly max_n (the only member with
    rows), 1500 (more than a block), counts that wrap the ring, and one push of the whole capacity into a full ring
    (every block, head and tail).  After each push a grouped priority write-back with duplicates.  After every step
    each member's w, bsum, bmax, fill level, write position and ring columns equal a DevicePrioritizedRing fed the same
    rows in the same order, and w equals per_ref.RefRing in numpy.  init_weight is 1 here, below the written-back
    priorities, so that every push spreads a maximum that differs per member and per step (at the default 1e8 the
    unseen slots' weight would be the maximum throughout)."""
    S, cap = 3, 3 * 1024 + 17
    L, p = LH.lib(), LH._p
    pop = PopulationPrioritizedRing(S, cap, init_weight=1.0, device=DEV)
    twins = [DevicePrioritizedRing(cap, device=DEV, init_weight=1.0) for _ in range(S)]
    refs = [P.RefRing(cap, init_weight=1.0) for _ in range(S)]
    _assert_rings(pop, twins, "initial")
    g = torch.Generator().manual_seed(3)
    rng = np.random.default_rng(4)
    steps = [(0, 1, 700), (0, 1500, 0), (1, 0, 1500), (1500, 1, 800), (1400, 1588, 1), (300, 5, 1500), (0, cap, 0),
             (1, 1, 1)]
    for step, counts in enumerate(steps):
        n = sum(counts)
        member = torch.cat([torch.full((c,), j, dtype=torch.int64) for j, c in enumerate(counts)])
        member = member[torch.randperm(n, generator=g)]  # interleaved; a member's rows keep their relative order
        cols = [torch.randn(n, 18, generator=g), torch.rand(n, 4, generator=g) * 2 - 1, torch.randn(n, generator=g),
                torch.randn(n, 18, generator=g), (torch.rand(n, generator=g) < 0.1).float()]
        pop.push(member.to(DEV), *[c.to(DEV) for c in cols])
        for j in range(S):
            if counts[j]:
                rows = member == j
                twins[j].push(*[c[rows].to(DEV) for c in cols])
                refs[j].push(counts[j])
        _assert_rings(pop, twins, ("push", step), columns=True)
        assert pop.pos_t.cpu().tolist() == [tw.pos for tw in twins] == [r.pos for r in refs], step
        assert pop.size_t.cpu().tolist() == [r.size for r in refs], step
        for j in range(S):
            assert np.array_equal(pop.member(j).w.cpu().numpy().view(np.uint32), refs[j].w.view(np.uint32)), (step, j)
        # priorities of 257 slots per member, 30 of them one slot; one large value that the next push spreads
        ups, keep = [], []
        for j in range(S):
            idx = rng.integers(0, max(refs[j].size, 1), 257)  # slot 0 of a member that is still empty
            idx[:30] = idx[30]
            td = np.exp(rng.normal(0, 3, 257)).astype(np.float32)
            td[7] = np.float32(2e5 + 1000 * step + j)
            idx_t, td_t = torch.from_numpy(idx).to(DEV), torch.from_numpy(td).to(DEV)
            keep += [idx_t, td_t]
            ups.append(LH.PerUpdateIO(pop.pers[j], 257, p(idx_t), p(td_t)))
            twins[j].last = idx_t
            twins[j].update_priorities(td_t)
            refs[j].update(idx, td)
        host = (LH.PerUpdateIO * S)(*ups)
        dev_t, dev = _dev_array(host)
        LH._check(L.hkl_per_update_group(host, dev, S, _st()), "hkl_per_update_group")
        _assert_rings(pop, twins, ("update", step))
        for j in range(S):
            assert np.array_equal(pop.member(j).w.cpu().numpy().view(np.uint32), refs[j].w.view(np.uint32)), (step, j)
    assert [r.size for r in refs] == [cap] * S  # every member filled up and wrapped


# ------------------------------------------------------------------------------------------------ learner
def _build(S, batch, cap, fill, prioritized=None):
    """(PopulationLearner on a PopulationPrioritizedRing, twin FusedLearners on a DevicePrioritizedRing each, or on a
    ReplayRing for a uniform member): same seeds (so the same initial weights), same ring contents, per-member beta."""
    from hockey_amd.learner_hip import FusedLearner

    prioritized = [True] * S if prioritized is None else prioritized
    betas = [BETAS[j % 3] for j in range(S)]
    pop = PopulationPrioritizedRing(S, cap, prioritized=prioritized, beta=betas, device=DEV)
    twins = []
    for j in range(S):
        data = _transitions(j, fill)
        pop.push(torch.full((fill,), j, dtype=torch.int64, device=DEV), *data)
        ring = DevicePrioritizedRing(cap, device=DEV, beta=betas[j]) if prioritized[j] else ReplayRing(cap, device=DEV)
        ring.push(*data)
        twins.append(FusedLearner(TD3(_cfg(j, batch), device=DEV, seed=40 + j), ring, batch, rng="device"))
    agents = [TD3(_cfg(j, batch), device=DEV, seed=40 + j) for j in range(S)]
    pl = PopulationLearner(agents, [pop.member(j) for j in range(S)], batch, warm_pairs=1)
    return pop, pl, twins


def _assert_learners(pop, pl, twins, what):
    torch.cuda.synchronize()
    for j, (a, b) in enumerate(zip(pl.members, twins)):
        sa, sb = _state(a), _state(b)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (what, "member", j, k)
        assert (a.iw is None) == (b.iw is None) == (not pop.member(j).prioritized)
        if a.iw is not None:
            assert torch.equal(a.iw, b.iw), (what, "member", j, "iw")
    _assert_rings(pop, [f.ring for f in twins], what)


def _push_some(pop, twins, seed):
    """One ragged push into every member (40 + 13 j rows, interleaved), and the same rows into the twins' rings."""
    S = len(twins)
    g = torch.Generator().manual_seed(seed)
    member = torch.cat([torch.full((40 + 13 * j,), j, dtype=torch.int64) for j in range(S)])
    member = member[torch.randperm(member.numel(), generator=g)]
    data = _transitions(99, member.numel())
    pop.push(member.to(DEV), *data)
    for j, f in enumerate(twins):
        rows = (member == j).to(DEV)
        f.ring.push(*[c[rows] for c in data])


@pytest.mark.parametrize("S,batch,updates,mixed", [(3, 256, 4, False), (3, 512, 4, False), (3, 256, 4, True),
                                                   (64, 256, 2, False)])
def test_grouped_prioritized_updates_equal_single_updates_bit_for_bit(S, batch, updates, mixed):
    """S = 3 all prioritized at B = 256 and 512, S = 3 mixed (prioritized, uniform, prioritized), four updates (actor
    off, on, off, on); S = 64 all prioritized, two updates.  After every update everything in test_gpu_population's
    _state, the importance weights and the rings' w, bsum and bmax equal the twins'."""
    big = S <= 3
    pop, pl, twins = _build(S, batch, 2048 if big else 512, 1500 if big else 300,
                            [True, False, True] if mixed else None)
    assert (pl.n_per, pl.n_uniform) == ((2, 1) if mixed else (S, 0))
    _assert_learners(pop, pl, twins, "initial")
    for u in range(updates):
        pl.update(u % 2 == 1)
        for f in twins:
            f.update(u % 2 == 1)
        _assert_learners(pop, pl, twins, f"update {u}")
    w = pop.member(0).w[:int(pop.size_t[0])]
    assert int((w != 1e8).sum()) > 0  # priorities were written back
    if S > 1:
        assert not torch.equal(pl.members[0].idx, pl.members[S - 1].idx)


def test_population_graph_replay_sees_pushed_priorities():
    """run(4) (a warm-up pair, then the pair captured and replayed), one ragged push into every member, run(2) (a
    further replay) against six eager twin updates with the same push at the same place."""
    pop, pl, twins = _build(3, 256, 2048, 1500, [True, False, True])
    pl.run(4)
    assert pl.graph is not None and pl.train_step == 4
    for u in range(4):
        for f in twins:
            f.update(u % 2 == 1)
    _assert_learners(pop, pl, twins, "graph replay")
    _push_some(pop, twins, 17)
    _assert_rings(pop, [f.ring for f in twins], "push", columns=True)
    pl.run(2)
    for u in range(2):
        for f in twins:
            f.update(u % 2 == 1)
    _assert_learners(pop, pl, twins, "replay after the push")
    # the replay drew from the pushed slots' priorities: the push moved the fill level, which the draws clamp to
    assert int(pop.size_t[0]) == 1540


def _copy(arr):
    return type(arr).from_buffer_copy(arr)


def test_refused_grouped_per_calls_launch_nothing():
    """Bad n_members, a null dev, a member with a null pointer, unequal cap / batch, and for the push max_n of 0 and
    a null pos: HKL_E_INVALID with the call's name in the message.  Nothing was launched: the population that made
    the bad calls stays bit-equal to twins that never saw them."""
    pop, pl, twins = _build(3, 256, 2048, 1500)
    L, h, d, S, st = pl.L, pl.host, pl.dptr, 3, _st()
    pers, pers_dev = pop.pers, ctypes.c_void_p(pop._pers_dev.data_ptr())
    args = pop._push_args.data_ptr()
    bad = []

    def refused(name, rc, member=None):
        msg = L.hkl_last_error().decode()
        if rc != 1 or not msg.startswith(name) or (member is not None and f"member {member}" not in msg):
            bad.append((name, rc, msg))

    calls = {"hkl_per_sample_group": ("psio", lambda a, dv, n: L.hkl_per_sample_group(a, dv, n, st)),
             "hkl_per_weights_group": ("psio", lambda a, dv, n: L.hkl_per_weights_group(a, dv, n, st)),
             "hkl_per_update_group": ("puio", lambda a, dv, n: L.hkl_per_update_group(a, dv, n, st))}
    for name, (key, fn) in calls.items():
        for n in (0, 65):
            refused(name, fn(h[key], d[key], n))
        refused(name, fn(h[key], None, S))
        c = _copy(h[key])
        c[1].per.bsum = None
        refused(name, fn(c, d[key], S), 1)
        c = _copy(h[key])
        c[2].per.cap = 4096
        refused(name, fn(c, d[key], S), 2)
        c = _copy(h[key])
        c[1].batch = 512
        refused(name, fn(c, d[key], S), 1)
    c = _copy(pers)
    c[2].cap = 4096
    for name, fn in (("hkl_per_refresh_group", lambda a, dv, n: L.hkl_per_refresh_group(a, dv, n, st)),
                     ("hkl_per_push_group", lambda a, dv, n: L.hkl_per_push_group(a, dv, args, args + 24, args + 48,
                                                                                  8, n, st))):
        for n in (0, 65):
            refused(name, fn(pers, pers_dev, n))
        refused(name, fn(pers, None, S))
        refused(name, fn(c, pers_dev, S), 2)
    refused("hkl_per_push_group", L.hkl_per_push_group(pers, pers_dev, args, args + 24, args + 48, 0, S, st))
    refused("hkl_per_push_group", L.hkl_per_push_group(pers, pers_dev, None, args + 24, args + 48, 8, S, st))
    assert not bad, bad
    for u in range(2):
        pl.update(u % 2 == 1)
        for f in twins:
            f.update(u % 2 == 1)
    _assert_learners(pop, pl, twins, "after the refused calls")


# ------------------------------------------------------------------------------------------------ training
def test_train_population_with_prioritized_members_on_the_gpu():
    """test_gpu_population's train_population shape -- 3 members, 4 arenas each, max_steps 30, batch 256, start_steps
    0, 4 updates per round, 3 rounds (the guard skips two), episode_end="done" -- with members prioritized / uniform /
    prioritized.  The bookkeeping is that test's for every member, the uniform one included; the prioritized members'
    rings hold written-back priorities inside [1e-6, 1e6]; all parameters are finite and have moved."""
    noises = ("gaussian", "ornstein-uhlenbeck", "pink")
    members = [(TD3Config(batch_size=256, max_steps=30, start_steps=0, noise_mode=nm, use_self_play=False,
                          curriculum_name="stage1", lr_q=4e-4 * (j + 1), prioritized_replay=j != 1,
                          beta=0.15 + 0.2 * j), 7 + j) for j, nm in enumerate(noises)]
    rows = []
    agents, st = train_population(members, n_arenas=4, rounds=3, device=DEV, updates_per_round=4, episode_end="done",
                                  on_step=lambda m, ar, *rest: rows.append(torch.stack([m, ar])))
    torch.cuda.synchronize()
    rows = torch.cat(rows, 1).cpu()
    assert torch.equal(rows[1] // 4, rows[0])
    for j, ag in enumerate(agents):
        stored = int((rows[0] == j).sum())
        assert st[j]["replay_size"] == st[j]["env_steps"] == ag.total_steps == stored > 256
        assert st[j]["skipped_rounds"] == 2 and st[j]["updates"] == 4 and ag.train_step == 4
        ring = ag._fused_learner.ring
        assert ring.prioritized == (j != 1)
        if ring.prioritized:
            assert ring.beta == members[j][0].beta
            w = ring.w[:stored]
            moved = w[w != 1e8]
            assert moved.numel() > 0 and bool(((moved >= 1e-6) & (moved <= 1e6)).all()), j
            assert bool((ring.w[stored:] == 1e8).all())  # unfilled slots keep init_weight
        init = TD3(members[j][0], device=DEV, seed=members[j][1])
        for net in ("actor", "critic", "target_actor", "target_critic"):
            assert all(torch.isfinite(p).all() for p in getattr(ag, net).parameters()), (j, net)
        assert not torch.equal(ag.actor.fc2.weight, init.actor.fc2.weight), j
