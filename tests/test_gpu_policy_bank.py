"""hkl_act (csrc/hk_learner.hip) through hockey_amd.policy_bank.PolicyBank on the GPU, and what is built on it:
OpponentMix(sampling="arena").select and evaluate.tournament.

Tolerance (learner_ref's rule, nothing fitted to the kernel).  For the rows a call writes,
err = max|out - out64| / max|out64| against a float64 forward on the CPU (tanh of learner_ref._mlp); the same
expression evaluated by torch in float32 on the GPU gives err_fp32_eager, and the bound is
learner_ref.bound(err_fp32_eager) = max(4 err_fp32_eager, 4 * 2^-24).  Output buffers are filled with NaN before a
call and compared as int32 afterwards, so a float the kernel should not have written is seen if it was, and one it
should have written is seen if it was not; the scratch buffers are poisoned before the call.

Measured on an MI355X (err and bound per case; the shapes cases gave the same figures at out_col 0 and 4; the
tournament row is the worst err / bound over the 502 per-step comparisons of part 7b, whose rows are the 36 to 60
acting arenas of one step under the checkpoint actors' large weights):

    case                                   err      bound    err / bound
    shapes n=1 K=1                         4.36e-07 1.03e-06 0.42
    shapes n=1 K=3                         7.03e-07 4.37e-06 0.16
    shapes n=1 K=40                        1.81e-07 6.90e-07 0.26
    shapes n=63 K=1                        5.06e-07 2.55e-06 0.20
    shapes n=63 K=3                        4.24e-07 1.73e-06 0.25
    shapes n=63 K=40                       4.24e-07 1.66e-06 0.26
    shapes n=64 K=1                        6.20e-07 1.84e-06 0.34
    shapes n=64 K=3                        3.92e-07 2.79e-06 0.14
    shapes n=64 K=40                       6.54e-07 1.86e-06 0.35
    shapes n=65 K=1                        5.14e-07 1.94e-06 0.26
    shapes n=65 K=3                        4.31e-07 1.61e-06 0.27
    shapes n=65 K=40                       4.19e-07 1.72e-06 0.24
    shapes n=200 K=1                       3.93e-07 2.46e-06 0.16
    shapes n=200 K=3                       4.83e-07 2.07e-06 0.23
    shapes n=200 K=40                      5.01e-07 2.38e-06 0.21
    shapes n=1000 K=1                      5.38e-07 2.10e-06 0.26
    shapes n=1000 K=3                      5.88e-07 1.98e-06 0.30
    shapes n=1000 K=40                     6.47e-07 1.77e-06 0.36
    replace n=200 K=3                      4.74e-07 1.70e-06 0.28
    checkpoints n=3280 K=12                1.61e-05 5.54e-05 0.29
    select n=4096 K=3                      6.61e-07 2.09e-06 0.32
    tournament steps=251 (worst step)      1.44e-05 1.53e-05 0.94

No case missed the bound.  Part 7a compares winners exactly, and torch's float32 GEMM picks its kernel by the row
count (on the MI355X a row's forward in a batch of 4 differed from the same row in a batch of 60 by up to 2.7e-6,
which changed 6 of the 15 pairs' games), so the reference loop evaluates its forwards at the tournament's row count
(_reference_winners).
"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import learner_ref as R  # noqa: E402
from hockey_amd.evaluate import Actor, reset_params, tournament, tournament_pairs  # noqa: E402
from hockey_amd.policy_bank import PolicyBank  # noqa: E402

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROWS, KS = (1, 63, 64, 65, 200, 1000), (1, 3, 40)
NAN_BITS = 0x7FC00000


# ---------------------------------------------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def _nets(K, seed=5):
    g = torch.Generator().manual_seed(seed + K)
    return tuple(R._net(g, 18, 4) for _ in range(K))


@functools.lru_cache(maxsize=None)
def _checkpoint_nets():
    with np.load(os.path.join(GOLDEN, "checkpoint_actors.npz"), allow_pickle=False) as z:
        return tuple({p: torch.from_numpy(z[f"{k}/{p.replace('.', '_')}"].copy()) for p in R.PARAMS} for k in range(12))


def _bank(nets, capacity=None):
    bank = PolicyBank(capacity or len(nets), DEV)
    for sd in nets:
        bank.add(sd)
    return bank


def _forward(nets, obs, policy, dtype, device):
    """[n, 4]: row i = tanh(mlp(obs_i)) of net policy[i] in ``dtype`` on ``device`` (rows at -1: 0)."""
    x = obs.detach().to(device=device, dtype=dtype)
    pol = policy.to(device)
    out = torch.zeros((x.shape[0], 4), dtype=dtype, device=device)
    for k, sd in enumerate(nets):
        rows = torch.nonzero(pol == k).squeeze(1)
        if rows.numel():
            p = {name: sd[name].to(device=device, dtype=dtype) for name in R.PARAMS}
            out[rows] = torch.tanh(R._mlp(p, x[rows]))
    return out


def _errors(got, nets, obs, policy):
    """(err, bound) of the written rows ``got`` [n, 4] (rows with policy >= 0)."""
    rows = (policy >= 0).cpu()
    ref64 = _forward(nets, obs, policy, torch.float64, "cpu")[rows]
    eager = _forward(nets, obs, policy, torch.float32, DEV).cpu()[rows]
    return R.rel_err(got.cpu()[rows], ref64), R.bound(R.rel_err(eager, ref64))


def _assign(n, K, seed=0):
    """Policies of n rows over K slots.  K >= 3 keeps slots 1 and (K > 3) K - 1 empty; from 200 rows on slot 0 gets
    exactly 64 rows and slot 2 at least 130; K = 1 fills slot 0 (exactly 64 rows at n = 64); rows at -1 from 65 rows
    on."""
    g = torch.Generator().manual_seed(1000 * K + n + seed)
    if K == 1:
        pol = torch.zeros(n, dtype=torch.int32)
        if n >= 65:
            pol[::7] = -1
        return pol
    usable = torch.tensor([k for k in range(K) if k not in (1, K - 1 if K > 3 else 1)], dtype=torch.int32)
    if n < 200:
        pool = torch.cat([usable, torch.tensor([-1], dtype=torch.int32)]) if n >= 65 else usable
        pol = pool[torch.randint(0, len(pool), (n,), generator=g)]
        pol[0] = 2
        return pol
    pol = torch.full((n,), -1, dtype=torch.int32)
    perm = torch.randperm(n, generator=g)
    pol[perm[:64]] = 0
    pol[perm[64:194]] = 2
    rest = perm[194 + (6 if n == 200 else 50):]
    others = usable[usable != 0]
    pol[rest] = others[torch.randint(0, len(others), (len(rest),), generator=g)]
    return pol


def _obs(n, seed=0, scale=1.5):
    return (torch.randn(n, 18, generator=torch.Generator().manual_seed(77 + n + seed)) * scale).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _poison(bank, n):
    """Scratch buffers of the n-row call, filled with junk before the call."""
    bank._scratch[n] = tuple(torch.full((m,), v, dtype=torch.int32, device=DEV)
                             for m, v in ((max(n, 1), -559038737), (65, 0x7F7F7F7F), (65, -1)))


def _act_checked(bank, nets, obs, policy, out_col=0):
    """One hip call into a NaN-filled [n, 8] buffer with poisoned scratch: asserts that exactly the acting rows'
    four floats were written; returns (their [n, 4] block, err, bound)."""
    n = obs.shape[0]
    out = torch.full((n, 8), float("nan"), device=DEV)
    _poison(bank, n)
    bank.act(obs, None if policy is None else policy.to(DEV), out=out, out_col=out_col, backend="hip")
    pol = torch.zeros(n, dtype=torch.int32) if policy is None else policy
    written = torch.zeros((n, 8), dtype=torch.bool)
    written[:, out_col:out_col + 4] = (pol >= 0).unsqueeze(1)
    bits = _bits(out).cpu()
    assert torch.all(bits[~written] == NAN_BITS), "a float outside the acting rows' four columns was written"
    got = out[:, out_col:out_col + 4]
    assert torch.isfinite(got.cpu()[pol >= 0]).all(), "an acting row was not written"
    err, bound = _errors(got, nets, obs, pol)
    return got, err, bound


# ---------------------------------------------------------------------------------------------------- 1. shapes
def test_assignments_cover_the_listed_conditions():
    """The parametrised cases below include empty slots, a slot with exactly 64 rows, a slot with more than 128
    rows and rows at -1; n = 1, 63, 64, 65 straddle one 64-row workgroup."""
    for K in (3, 40):
        for n in (200, 1000):
            c = torch.bincount(_assign(n, K)[_assign(n, K) >= 0].long(), minlength=K)
            assert c[0] == 64 and c[2] > 128 and c[1] == 0 and (_assign(n, K) == -1).any(), (K, n)
    assert (torch.bincount(_assign(1000, 40).long() + 1, minlength=41)[1:] == 0).sum() == 2
    assert int((_assign(64, 1) == 0).sum()) == 64 and (_assign(200, 1) == -1).any() and (_assign(200, 1) == 0).sum() > 128
    for n in ROWS:
        for K in KS:
            pol = _assign(n, K)
            assert pol.shape == (n,) and (pol >= 0).any() and pol.max() < K and pol.min() >= -1


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", ROWS)
def test_act_shapes(n, K):
    """Part 1: n_rows x K, random weights (learner_ref._net), out_ld = 8 and out_col 0 / 4 into NaN: the written
    rows meet the bound, every other float is still NaN."""
    nets = _nets(K)
    bank = _bank(nets)
    obs, pol = _obs(n), _assign(n, K)
    for out_col in (0, 4):
        _, err, bound = _act_checked(bank, nets, obs, pol, out_col)
        print(f"MEASURED shapes n={n} K={K} out_col={out_col} err={err:.3g} bound={bound:.3g} ratio={err / bound:.2f}")
        assert err <= bound, (n, K, out_col, err, bound)


# ---------------------------------------------------------------------------------------------------- 2. independence
def test_row_result_is_independent_of_grouping():
    """Part 2 (1000 rows, K = 3): a row's four floats are the same bits under a row permutation, when the other
    rows' policies change, when the row is computed alone, and from the policy = NULL single-slot call on a bank
    that holds its slot's weights at slot 0."""
    n, K = 1000, 3
    nets = _nets(K)
    bank = _bank(nets)
    obs, pol = _obs(n), _assign(n, K)
    base, _, _ = _act_checked(bank, nets, obs, pol)
    base = _bits(base).cpu()
    acting = pol >= 0
    g = torch.Generator().manual_seed(3)
    # a row permutation
    perm = torch.randperm(n, generator=g)
    got, _, _ = _act_checked(bank, nets, obs[perm.to(DEV)], pol[perm])
    assert torch.equal(_bits(got).cpu()[acting[perm]], base[perm][acting[perm]])
    # every fifth row keeps its policy, the others draw a new one (or stop acting)
    keep = torch.zeros(n, dtype=torch.bool)
    keep[::5] = True
    pol2 = torch.where(keep, pol, torch.randint(-1, K, (n,), generator=g, dtype=torch.int32))
    got, _, _ = _act_checked(bank, nets, obs, pol2)
    assert (keep & acting).sum() > 100 and torch.equal(_bits(got).cpu()[keep & acting], base[keep & acting])
    # alone
    for i in torch.nonzero(acting).squeeze(1)[::97].tolist():
        got, _, _ = _act_checked(bank, nets, obs[i:i + 1], pol[i:i + 1])
        assert torch.equal(_bits(got).cpu()[0], base[i]), i
    # the single-slot call
    for k in (0, 2):
        single = _bank(nets[k:k + 1])
        got, _, _ = _act_checked(single, nets[k:k + 1], obs, None)
        assert torch.equal(_bits(got).cpu()[pol == k], base[pol == k]), k
        fn = _bits(bank.policy_fn(k, backend="hip")(obs)).cpu()
        assert torch.equal(fn[pol == k], base[pol == k]), k


# ---------------------------------------------------------------------------------------------------- 3. real weights
@functools.lru_cache(maxsize=None)
def _played_obs():
    """Observations of 64 arenas x 50 strong-vs-strong steps, then 16 rows of zeros and the first 64 rows x 50."""
    from hockey_amd.vec_env import VecHockeyEnv

    env = VecHockeyEnv(64, device=DEV, policies=("strong", "strong"), seed=11)
    params, _, _ = reset_params(64, 11)
    env.reset_params(params)
    rows = []
    for _ in range(50):
        rows.append(env.step(None).obs.clone())
    env.close()
    rows = torch.cat(rows)
    return torch.cat([rows, torch.zeros((16, 18), device=DEV), rows[:64] * 50.0])


def test_checkpoint_actors_on_played_observations():
    """Part 3: the 12 shipped actors on observations of real play, on zeros and on rows scaled x50 (tanh saturates):
    the bound holds, every output is finite and in [-1, 1]."""
    nets = _checkpoint_nets()
    bank = _bank(nets)
    obs = _played_obs()
    n = obs.shape[0]
    pol = torch.randint(0, 12, (n,), generator=torch.Generator().manual_seed(4), dtype=torch.int32)
    got, err, bound = _act_checked(bank, nets, obs, pol, out_col=4)
    print(f"MEASURED checkpoints n={n} K=12 err={err:.3g} bound={bound:.3g} ratio={err / bound:.2f}")
    assert err <= bound, (err, bound)
    assert torch.isfinite(got).all() and float(got.abs().max()) <= 1.0
    sat = got[-64:].abs().max(1).values
    assert float((sat > 0.999).float().mean()) > 0.5  # the x50 rows do saturate


# ---------------------------------------------------------------------------------------------------- 4. replacement
def test_replace_refreshes_the_slot_and_leaves_the_others():
    """Part 4: after replace(slot, other) the slot's rows follow the new weights (the pack was refreshed), the other
    slots' rows are the bits they were."""
    n, K = 200, 3
    nets = list(_nets(40)[:3])
    bank = _bank(nets)
    obs = _obs(n)
    pol = torch.arange(n, dtype=torch.int32) % K
    before, _, _ = _act_checked(bank, nets, obs, pol)
    before = _bits(before).cpu()
    nets[1] = _nets(40)[7]
    bank.replace(1, nets[1])
    after, err, bound = _act_checked(bank, nets, obs, pol)
    print(f"MEASURED replace n={n} K={K} err={err:.3g} bound={bound:.3g} ratio={err / bound:.2f}")
    assert err <= bound, (err, bound)
    after = _bits(after).cpu()
    assert torch.equal(after[pol != 1], before[pol != 1])
    assert not torch.equal(after[pol == 1], before[pol == 1])


# ---------------------------------------------------------------------------------------------------- 5. graph
def test_act_replays_from_a_graph():
    """Part 5: one act call captured with torch.cuda.graph and replayed after obs and policy changed in place equals
    the eager call on the same contents, bit for bit."""
    n, K = 1000, 3
    nets = _nets(K)
    bank = _bank(nets)
    obs, pol = _obs(n).clone(), _assign(n, K).to(DEV)
    out = torch.full((n, 8), float("nan"), device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        bank.act(obs, pol, out=out, out_col=4, backend="hip")  # warm-up: the scratch buffers exist before the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bank.act(obs, pol, out=out, out_col=4, backend="hip")
    for seed in (1, 2):
        obs.copy_(_obs(n, seed))
        pol.copy_(_assign(n, K, seed))
        out.fill_(float("nan"))
        graph.replay()
        eager = torch.full((n, 8), float("nan"), device=DEV)
        bank.act(obs, pol, out=eager, out_col=4, backend="hip")
        assert torch.equal(_bits(out), _bits(eager))
        assert int((_bits(out)[:, 4] != NAN_BITS).sum()) == int((pol >= 0).sum())


# ---------------------------------------------------------------------------------------------------- 6. select
def test_select_per_arena_on_the_gpu():
    """Part 6: OpponentMix(sampling="arena").select at 4096 arenas with 3 snapshots: the self-play arenas' player-2
    actions meet the bound against each arena's own snapshot, every other float of the action buffer is untouched."""
    from hockey_amd import _native as N
    from hockey_amd.opponents import OpponentMix

    n = 4096
    nets = _nets(3)
    mix = OpponentMix(n, [(1.0, 0.3, 0.2, 0.5)], pool_size=4, device=DEV, seed=6, sampling="arena")
    for sd in nets:
        a = Actor()
        a.load_state_dict(sd)
        mix.pool.add_snapshot(a.to(DEV))
    mix.pool.scores[:] = [1.0, 2.0, 5.0]
    obs2 = _obs(n)
    act8 = torch.full((n, 8), float("nan"), device=DEV)
    p2, out, policy = mix.select(obs2, out=act8)
    assert out is act8
    sp = (p2 == N.POLICY_EXTERNAL).cpu()
    policy = policy.cpu()
    assert torch.equal(policy >= 0, sp) and 0.4 < float(sp.float().mean()) < 0.6
    slot_to_snap = {s: i for i, s in enumerate(mix.pool.slots)}
    snap = torch.tensor([slot_to_snap.get(int(s), -1) for s in policy.tolist()], dtype=torch.int32)
    assert all(int((snap == i).sum()) > 100 for i in range(3))
    bits = _bits(act8).cpu()
    assert torch.all(bits[:, :4] == NAN_BITS) and torch.all(bits[~sp, 4:] == NAN_BITS)
    assert torch.isfinite(act8[:, 4:].cpu()[sp]).all()
    err, bound = _errors(act8[:, 4:], nets, obs2, snap)
    print(f"MEASURED select n={n} K=3 err={err:.3g} bound={bound:.3g} ratio={err / bound:.2f}")
    assert err <= bound, (err, bound)


# ---------------------------------------------------------------------------------------------------- 7. tournament
T_GAMES, T_SEED = 4, 21


def _fixture_actors():
    out = []
    for sd in _checkpoint_nets()[:3]:
        a = Actor()
        a.load_state_dict(sd)
        out.append(a.to(DEV).eval())
    return out


@torch.no_grad()
def _reference_winners(actors, games, seed, at_tournament_rows=True):
    """Each pair on its own, in a fresh VecHockeyEnv of ``games`` arenas that carries the pair's global arena ids
    (the bots' phase walks are keyed by them), with torch Actor forwards.

    torch's float32 GEMM picks its kernel, and with it the summation order, by the number of rows, so a row's
    forward in a batch of ``games`` rows need not be the bits of the same row in the tournament's batch, and one
    last-bit action difference may change a game.  The loop therefore evaluates its forwards at the tournament's
    row count, the pair's observations in the rows they have there and zeros elsewhere (at_tournament_rows; False
    evaluates the ``games`` rows alone)."""
    from hockey_amd.vec_env import VecHockeyEnv, _POLICIES

    k = len(actors)
    p1, p2, g = tournament_pairs(k, games, True)
    params, max_t, _ = reset_params(games, seed)
    phases = np.random.default_rng(seed).uniform(0, 2 * np.pi, (len(p1), 3))
    winners = np.zeros(len(p1), np.int8)
    for a0 in range(0, len(p1), games):
        i, j = int(p1[a0]), int(p2[a0])
        env = VecHockeyEnv(games, device=DEV, policies=("external", "external"), seed=seed, arena_offset=a0)
        env.reset_params(params)
        env.opponent_phase(phases[a0:a0 + games], rows=3)
        pid = _POLICIES["external"] if j >= 0 else _POLICIES["weak"] if j == -1 else _POLICIES["strong"]
        policy2 = torch.full((games,), pid, dtype=torch.uint8, device=DEV)
        obs, obs2 = (t.clone() for t in env.observe())
        act = torch.zeros((games, 8), device=DEV)
        live = torch.ones(games, dtype=torch.bool, device=DEV)
        winner = torch.zeros(games, device=DEV)
        pad = torch.zeros((len(p1), 18), device=DEV)

        def forward(actor, x):
            if not at_tournament_rows:
                return actor(x)
            pad[a0:a0 + games] = x
            return actor(pad)[a0:a0 + games]

        for _ in range(max_t + 1):
            act[:, :4] = forward(actors[i], obs)
            if j >= 0:
                act[:, 4:] = forward(actors[j], obs2)
            res = env.step(act, with_agent_two=True, policy2=policy2)
            d = res.done.bool()
            winner = torch.where(live & d, res.info[:, 0], winner)
            live &= ~d
            obs, obs2 = res.obs, res.obs2
            if not bool(live.any()):
                break
        env.close()
        winners[a0:a0 + games] = winner.cpu().numpy().astype(np.int8)
    return winners


def test_tournament_torch_backend_equals_pairwise_reference_loop():
    """Part 7a: 3 fixture actors, 4 games, both bot columns (60 arenas): with backend="torch" the winners equal,
    exactly, those of a plain loop that plays each pair on its own with the same placements and phases."""
    actors = _fixture_actors()
    out = tournament(actors, games=T_GAMES, seed=T_SEED, include_bots=True, backend="torch", per_game=True, device=DEV)
    want = _reference_winners(actors, T_GAMES, T_SEED).reshape(3, 5, T_GAMES)
    assert out["winner"].shape == (3, 5, T_GAMES)
    diff = np.argwhere((out["winner"] != want).any(2)).tolist()
    assert not diff, f"pairs (row, column) whose winners differ: {diff}"
    assert len({int(v) for v in want.reshape(-1)}) > 1  # not one outcome everywhere
    np.testing.assert_array_equal(out["win"], (want == 1).mean(2))


def test_tournament_hip_backend_teacher_forced_and_row_sums():
    """Part 7b: along the torch run, at every step the hip actions on that step's obs / obs2 meet the bound; the
    matrices of a backend="hip" tournament have rows win + draw + loss = 1."""
    actors = _fixture_actors()
    nets = _checkpoint_nets()[:3]
    bank = _bank(nets)
    p1, p2, _ = tournament_pairs(3, T_GAMES, True)
    pol1, pol2 = torch.as_tensor(p1), torch.as_tensor(np.maximum(p2, -1))
    worst = []

    def on_step(obs, obs2, act):
        hip = torch.full((len(p1), 8), float("nan"), device=DEV)
        bank.act(obs, pol1.to(DEV), out=hip, out_col=0, backend="hip")
        bank.act(obs2, pol2.to(DEV), out=hip, out_col=4, backend="hip")
        for x, pol, c in ((obs, pol1, 0), (obs2, pol2, 4)):
            rows = pol >= 0
            ref64 = _forward(nets, x, pol, torch.float64, "cpu")[rows]
            err = R.rel_err(hip[:, c:c + 4].cpu()[rows], ref64)
            bound = R.bound(R.rel_err(act[:, c:c + 4].cpu()[rows], ref64))  # act: torch's float32 of the same
            worst.append((err / bound, err, bound))
            assert err <= bound, (len(worst), c, err, bound)
        assert torch.all(_bits(hip[:, 4:]).cpu()[pol2 < 0] == NAN_BITS)

    tournament(actors, games=T_GAMES, seed=T_SEED, backend="torch", device=DEV, on_step=on_step)
    w = max(worst)
    print(f"MEASURED tournament steps={len(worst) // 2} worst err={w[1]:.3g} bound={w[2]:.3g} ratio={w[0]:.2f}")
    out = tournament(actors, games=T_GAMES, seed=T_SEED, backend="hip", device=DEV)
    for key in ("win", "draw", "loss", "score", "mean_length"):
        assert out[key].shape == (3, 5)
    np.testing.assert_allclose(out["win"] + out["draw"] + out["loss"], np.ones((3, 5)), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(out["score"], out["win"] + 0.5 * out["draw"])
