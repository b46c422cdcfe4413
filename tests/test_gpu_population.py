"""The grouped learner kernels (include/hockey_learner.h hkl_*_group, csrc/hk_learner.hip) and hockey_amd.population on
the GPU.  The grouped form promises member m the single call's results bit for bit, whatever the other members are:
every comparison here is torch.equal against plain FusedLearners fed the same rings, seeds and weights."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hockey_amd.population import PopulationLearner, PopulationRing, train_population  # noqa: E402
from hockey_amd.td3 import TD3, ReplayRing, TD3Config  # noqa: E402

DEV = "cuda:0"


def _cfg(j, batch):
    """Members that differ in everything the grouped kernels read per member."""
    return TD3Config(batch_size=batch, lr_q=4e-4 * (1 + 0.5 * (j % 5)), lr_pol=4e-4 / (1 + (j % 3)),
                     gamma=0.99 - 0.01 * (j % 4), tau_actor=0.005 * (1 + j % 2), tau_critic=0.005 * (1 + j % 3),
                     wd_q=1e-4 if j % 3 == 1 else 0.0, target_action_noise_scale=0.2 + 0.05 * (j % 2))


def _transitions(j, n):
    g = torch.Generator().manual_seed(1000 + j)
    return [t.to(DEV) for t in (torch.randn(n, 18, generator=g), torch.rand(n, 4, generator=g) * 2 - 1,
                                torch.randn(n, generator=g), torch.randn(n, 18, generator=g),
                                (torch.rand(n, generator=g) < 0.1).float())]


def _build(S, batch, cap, fill):
    """(PopulationLearner on a PopulationRing, twin FusedLearners on ReplayRings): same seeds (so the same initial
    weights), same ring contents."""
    from hockey_amd.learner_hip import FusedLearner

    pop = PopulationRing(S, cap, device=DEV)
    twins = []
    for j in range(S):
        data = _transitions(j, fill)
        pop.push(torch.full((fill,), j, dtype=torch.int64, device=DEV), *data)
        ring = ReplayRing(cap, device=DEV)
        ring.push(*data)
        twins.append(FusedLearner(TD3(_cfg(j, batch), device=DEV, seed=40 + j), ring, batch, rng="device"))
    agents = [TD3(_cfg(j, batch), device=DEV, seed=40 + j) for j in range(S)]
    pl = PopulationLearner(agents, [pop.member(j) for j in range(S)], batch, warm_pairs=1)
    return pl, twins


def _state(f):
    """Everything an update writes that a later update or the caller reads."""
    out = {"flat_" + k: v for k, v in f.flat.items()}
    out.update({"m_" + k: v for k, v in f.m.items()})
    out.update({"v_" + k: v for k, v in f.v.items()})
    out.update({"step_" + k: v for k, v in f.step.items()})
    out.update({"pack_" + k: nb.pack for k, nb in f.nets.items()})
    out.update(sample_counter=f.sample_counter, idx=f.idx, td=f.buf["td"], noise=f.buf["noise"], acc=f._acc)
    return out


def _assert_equal(pl, twins, what):
    torch.cuda.synchronize()
    for j, (a, b) in enumerate(zip(pl.members, twins)):
        sa, sb = _state(a), _state(b)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (what, "member", j, k)


@pytest.mark.parametrize("S,batch,updates", [(3, 256, 4), (3, 512, 4), (1, 256, 2), (64, 256, 2)])
def test_grouped_updates_equal_single_updates_bit_for_bit(S, batch, updates):
    """S = 3 (odd: a member / grid mix-up shows) at B = 256 and 512 (hkl_wgrad's 512-sample split-K chunks), four
    updates (actor off, on, off, on); S = 1 and 64, the ends of the member range, two updates.  Every parameter,
    target parameter, Adam moment, pack, step and sample counter, idx, td and loss accumulator is torch.equal."""
    big = S <= 3
    pl, twins = _build(S, batch, 2048 if big else 512, 1500 if big else 300)
    _assert_equal(pl, twins, "initial")
    for u in range(updates):
        pl.update(u % 2 == 1)
        for f in twins:
            f.update(u % 2 == 1)
        _assert_equal(pl, twins, f"update {u}")
    assert int(twins[0].step["critic"]) == updates and int(pl.members[-1].step["actor"]) == updates // 2
    losses = pl.take_losses()
    assert len(losses) == S and all(cl is not None and al is not None for cl, al in losses)
    if S > 1:  # the members really are different learners
        assert not torch.equal(pl.members[0].flat["critic"], pl.members[1].flat["critic"])
        assert not torch.equal(pl.members[0].idx, pl.members[1].idx)


def test_population_graph_replay_equals_eager_grouped_updates():
    """run(4) -- one warm-up pair, then the pair captured and replayed -- against four eager grouped updates."""
    pl, twins = _build(3, 256, 2048, 1500)
    pl.run(4)
    assert pl.graph is not None and pl.train_step == 4 and all(ag.train_step == 4 for ag in pl.agents)
    for u in range(4):
        for f in twins:
            f.update(u % 2 == 1)
    _assert_equal(pl, twins, "graph replay")
    pl.run(2)  # a further replay of the captured graph
    for u in range(2):
        for f in twins:
            f.update(u % 2 == 1)
    _assert_equal(pl, twins, "second replay")


def _copy(arr):
    return type(arr).from_buffer_copy(arr)


def test_group_calls_reject_bad_arguments_and_launch_nothing():
    """n_members of 0 or 65, unequal batches, a batch that is no multiple of 256, a null dev and a member with a null
    required pointer: HKL_E_INVALID with a message from every grouped call that has the argument.  Nothing was
    launched: the learner that made the bad calls stays bit-equal to twins that never saw them."""
    pl, twins = _build(3, 256, 2048, 1500)
    L, h, d, S = pl.L, pl.host, pl.dptr, 3
    st = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    simple = {"hkl_sample_group": ("sio", "idx"), "hkl_critic_step_group": ("cio", "x0"),
              "hkl_actor_step_group": ("aio", "dz2"), "hkl_adam_group": ("adam_c1", "step")}
    bad = []

    def refused(name, rc):
        msg = L.hkl_last_error().decode()
        if rc != 1 or not msg.startswith(name) or len(msg) <= len(name) + 2:
            bad.append((name, rc, msg))

    for name, (key, ptr) in simple.items():
        fn = getattr(L, name)
        for n in (0, 65):
            refused(name, fn(h[key], d[key], n, st))
        refused(name, fn(h[key], None, S, st))
        c = _copy(h[key])
        setattr(c[1], ptr, None)
        refused(name, fn(c, d[key], S, st))
        assert "member 1" in L.hkl_last_error().decode()
        if hasattr(c[0], "batch"):
            c = _copy(h[key])
            c[2].batch = 512
            refused(name, fn(c, d[key], S, st))
            assert "member 2" in L.hkl_last_error().decode()
            c = _copy(h[key])
            for io in c:
                io.batch = 320
            refused(name, fn(c, d[key], S, st))
    c = _copy(h["adam_c1"])  # adam: a member whose segment shape differs
    c[1].seg[0].rows += 1
    refused("hkl_adam_group", L.hkl_adam_group(c, d["adam_c1"], S, st))
    # pack
    for n in (0, 65):
        refused("hkl_pack_group", L.hkl_pack_group(h["pack_a"], d["pack_a"], 4, n, st))
    refused("hkl_pack_group", L.hkl_pack_group(h["pack_a"], None, 4, S, st))
    c = _copy(h["pack_a"])
    c[2].net[3].w2 = None
    refused("hkl_pack_group", L.hkl_pack_group(c, d["pack_a"], 4, S, st))
    # wgrad pair: the batch is one argument for all members
    wg = lambda w, wd, n_, nd, batch, n: L.hkl_wgrad_pair_group(w, wd, 2, n_, nd, 2, batch, n, st)  # noqa: E731
    for n in (0, 65):
        refused("hkl_wgrad_pair_group", wg(h["c256"], d["c256"], h["c32"], d["c32"], 256, n))
    refused("hkl_wgrad_pair_group", wg(h["c256"], d["c256"], h["c32"], d["c32"], 320, S))
    refused("hkl_wgrad_pair_group", wg(h["c256"], None, h["c32"], d["c32"], 256, S))
    refused("hkl_wgrad_pair_group", wg(h["c256"], d["c256"], h["c32"], None, 256, S))
    c = _copy(h["c32"])
    c[5].slab = None  # member 2's second narrow job
    refused("hkl_wgrad_pair_group", wg(h["c256"], d["c256"], c, d["c32"], 256, S))
    assert "member 2" in L.hkl_last_error().decode()
    assert not bad, bad
    for u in range(2):
        pl.update(u % 2 == 1)
        for f in twins:
            f.update(u % 2 == 1)
    _assert_equal(pl, twins, "after the refused calls")


def test_train_population_on_the_gpu():
    """S = 3 (gaussian / ornstein-uhlenbeck / pink), 4 arenas each, max_steps 30, batch 256, start_steps 0, 4 updates
    per round, episode_end="done".  Two such rounds store at most 2 x 4 x 30 = 240 transitions per member, which the
    documented guard (updates start once every member's total_steps exceeds the batch of 256) does not pass, so the
    run has a third round: the first two are skipped by the guard, the third updates."""
    noises = ("gaussian", "ornstein-uhlenbeck", "pink")
    members = [(TD3Config(batch_size=256, max_steps=30, start_steps=0, noise_mode=nm, use_self_play=False,
                          curriculum_name="stage1", lr_q=4e-4 * (j + 1)), 7 + j) for j, nm in enumerate(noises)]
    rows = []
    agents, st = train_population(members, n_arenas=4, rounds=3, device=DEV, updates_per_round=4, episode_end="done",
                                  on_step=lambda m, ar, *rest: rows.append(torch.stack([m, ar])))
    torch.cuda.synchronize()
    rows = torch.cat(rows, 1).cpu()
    assert torch.equal(rows[1] // 4, rows[0])  # member j's stored transitions come from arenas [4 j, 4 j + 4)
    for j, ag in enumerate(agents):
        stored = int((rows[0] == j).sum())
        assert st[j]["replay_size"] == st[j]["env_steps"] == ag.total_steps == stored > 256
        assert st[j]["skipped_rounds"] == 2 and st[j]["updates"] == 4 and ag.train_step == 4
        init = TD3(members[j][0], device=DEV, seed=members[j][1])
        for net in ("actor", "critic", "target_actor", "target_critic"):
            assert all(torch.isfinite(p).all() for p in getattr(ag, net).parameters()), (j, net)
        assert not torch.equal(ag.actor.fc2.weight, init.actor.fc2.weight), j
        for k in range(j):
            assert not torch.equal(ag.actor.fc2.weight, agents[k].actor.fc2.weight), (j, k)
