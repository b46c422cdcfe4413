"""Seeded resets drawn on the GPU: hk_seeded_params / hk_reset_seeded (csrc/hk_seeded_reset.hip, one lane per arena
over csrc/hk_seed.h) through VecHockeyEnv, evaluate and train, against the host path -- numpy's SeedSequence / PCG64
/ Generator.uniform in hockey_amd.placement, uploaded through hk_reset.  Every comparison is byte for byte.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import seed_cases as SC  # noqa: E402
from hockey_amd import _native as N  # noqa: E402
from hockey_amd.constants import Mode  # noqa: E402
from hockey_amd.placement import np_random, placement  # noqa: E402
from scene_lockstep import require_gfx950  # noqa: E402

DEV = "cuda:0"
MODES = (Mode.NORMAL, Mode.TRAIN_SHOOTING, Mode.TRAIN_DEFENSE)
N_TWIN = 200  # three full waves and a partial one


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gfx950()


def _vec(n, mode=Mode.NORMAL, **kw):
    from hockey_amd.vec_env import VecHockeyEnv

    kw.setdefault("policies", ("external", "external"))
    return VecHockeyEnv(n, mode=mode, device=DEV, **kw)


def _blob(env, indices=None):
    return env.snapshot(indices).blob.cpu().numpy()


def _one_flags(env):
    """The arenas' stored one_starts flags: bit 31 of the first packed int row of a whole-env snapshot (the rows
    follow the NFF float rows, 16-byte aligned)."""
    from hockey_amd import snapshot as S

    nff = S.library_layout()[0]
    off = (nff * 4 * env.n + 15) // 16 * 16
    return (_blob(env)[off:off + 4 * env.n].view(np.uint32) >> 31).astype(bool)


def _host_params(mode, seeds, one):
    p = np.zeros((len(seeds), 6), np.float32)
    for i, s in enumerate(seeds):
        p[i], _ = placement(mode, bool(one[i]), np_random(int(s))[0])
    return p


def _twin_seeds():
    # the edge seeds (both entropy lengths, the top bit) and the head of the random ones
    return np.ascontiguousarray(SC.SEEDS[:N_TWIN])


@pytest.mark.parametrize("mode", MODES)
def test_seeded_params_equal_the_host_placement_over_the_case_list(mode):
    seeds, one, want_p, want_t = SC.mode_rows(mode.value)
    assert len(seeds) % 64 != 0  # the last wave is partial
    env = _vec(len(seeds), mode)
    before = _blob(env)
    params, max_t = env.seeded_params(seeds, one_starting=one)
    got_p, got_t = params.cpu().numpy(), max_t.cpu().numpy()
    bad = np.nonzero((got_p.view(np.uint32) != want_p.view(np.uint32)).any(1) | (got_t != want_t))[0]
    assert bad.size == 0, (len(bad), int(seeds[bad[0]]), int(one[bad[0]]), got_p[bad[0]], want_p[bad[0]])
    # one_starting=None draws for the stored flag (True after the constructor's reset), and nothing touched an arena
    params1, _ = env.seeded_params(seeds)
    sel = one == 1
    assert np.array_equal(params1.cpu().numpy()[sel].view(np.uint32), want_p[sel].view(np.uint32))
    assert np.array_equal(_blob(env), before)
    env.close()


@pytest.mark.parametrize("mode", MODES)
def test_reset_seeded_leaves_the_host_paths_arena_bit_for_bit(mode):
    seeds = _twin_seeds()
    rng = np.random.default_rng(7)
    acts = rng.uniform(-1, 1, (N_TWIN, 8)).astype(np.float32)

    def run(dev_reset, host_reset):
        a, b = _vec(N_TWIN, mode), _vec(N_TWIN, mode)
        dev_reset(a)
        host_reset(b)
        assert np.array_equal(_blob(a), _blob(b))
        for _ in range(3):
            ra, rb = a.step(torch.as_tensor(acts, device=DEV)), b.step(torch.as_tensor(acts, device=DEV))
            for f in ("obs", "reward", "done"):
                ga, gb = getattr(ra, f).cpu().numpy(), getattr(rb, f).cpu().numpy()
                assert np.array_equal(ga.view(np.uint8), gb.view(np.uint8)), f
        assert np.array_equal(_blob(a), _blob(b))
        a.close()
        b.close()

    # one_starting=None toggles the constructor's True to False; reset_params toggles the same flag
    run(lambda e: e.reset_seeded(seeds),
        lambda e: e.reset_params(_host_params(mode, seeds, np.zeros(N_TWIN, bool))))
    # explicit puck sides against the host path of reset(seeds=...)
    side = rng.integers(0, 2, N_TWIN).astype(bool)
    run(lambda e: e.reset_seeded(seeds, one_starting=side),
        lambda e: e.reset(seeds=[int(s) for s in seeds], one_starting=side))


def test_mask_keeps_other_arenas_and_the_puck_side_alternates():
    seeds = _twin_seeds()
    rng = np.random.default_rng(11)
    a, b = _vec(N_TWIN), _vec(N_TWIN)
    for k in range(2):  # two successive calls: NORMAL mode alternates the side of the arenas each call selects
        mask = rng.integers(0, 2, N_TWIN).astype(bool)
        out = np.nonzero(~mask)[0]
        kept = _blob(a, out)
        was = a.one_starts.copy()
        s = seeds[rng.permutation(N_TWIN)]
        a.reset_seeded(s, mask=mask)
        b.reset(seeds=[int(x) for x in s], mask=mask)
        assert np.array_equal(_blob(a, out), kept)  # every word, the episode word and the flag included
        assert np.array_equal(_blob(a), _blob(b))
        assert np.array_equal(a.one_starts, np.where(mask, ~was, was))
        assert np.array_equal(a.one_starts, _one_flags(a)) and np.array_equal(b.one_starts, _one_flags(b))
        st, _ = a.get_state()
        left = st[:, 12].cpu().numpy() < 5.0  # the puck starts on player 1's side
        assert np.array_equal(left[mask], a.one_starts[mask])
    # reset(seeds=..., placement="device") is the same call
    s = seeds[::-1].copy()
    a.reset(seeds=s, placement="device")
    b.reset(seeds=[int(x) for x in s])
    assert np.array_equal(_blob(a), _blob(b)) and np.array_equal(a.one_starts, b.one_starts)
    for bad in ([None] * N_TWIN, [2**64] * N_TWIN, [-1] * N_TWIN, np.full(N_TWIN, -3, np.int64),
                torch.full((N_TWIN,), -1, dtype=torch.int64, device=DEV)):
        kept = _blob(a)
        with pytest.raises(ValueError):
            a.reset(seeds=bad, placement="device")
        assert np.array_equal(_blob(a), kept)
    a.close()
    b.close()


def test_max_t_passes_through_and_is_range_checked():
    seeds = _twin_seeds()
    mt = (np.arange(N_TWIN) % 300 + 1).astype(np.int32)
    a, b = _vec(N_TWIN), _vec(N_TWIN)
    a.reset_seeded(seeds, max_t=mt)
    b.reset_params(_host_params(Mode.NORMAL, seeds, np.zeros(N_TWIN, bool)), max_t=mt)
    assert np.array_equal(_blob(a), _blob(b))
    kept, mirror = _blob(a), a.one_starts.copy()
    bad = mt.copy()
    bad[137] = 65536
    st = torch.as_tensor(seeds.copy()).to(DEV)
    rc = a.L.hk_reset_seeded(a._ctx, None, N.ptr(st), N.ptr(torch.as_tensor(bad, device=DEV)), None, a._stream())
    assert rc == -1 and b"hk_reset_seeded: max_t out of range" in a.L.hk_last_error()  # HK_E_INVALID
    torch.cuda.synchronize()
    assert np.array_equal(_blob(a), kept) and np.array_equal(a.one_starts, mirror)
    bad[137] = 5  # ... and an out-of-range value of an arena the mask leaves out is not looked at
    bad[3] = -1
    mask = np.ones(N_TWIN, bool)
    mask[3] = False
    a.reset_seeded(seeds, mask=mask, max_t=bad)
    a.close()
    b.close()


def test_reset_seeded_replays_from_a_captured_graph():
    seeds = torch.as_tensor(_twin_seeds().copy()).to(DEV)  # uint64: the list has seeds above 2^63
    assert seeds.dtype == torch.uint64
    a, b = _vec(N_TWIN), _vec(N_TWIN)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a.reset_seeded(seeds)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    a.step(torch.zeros((N_TWIN, 8), device=DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.reset_seeded(seeds)
    g.replay()
    torch.cuda.synchronize()
    b.reset_seeded(seeds)
    b.step(torch.zeros((N_TWIN, 8), device=DEV))
    b.reset_seeded(seeds)
    assert np.array_equal(_blob(a), _blob(b))
    assert np.array_equal(a.one_starts, _one_flags(a))
    a.close()
    b.close()


def test_evaluate_plays_the_same_episodes_from_device_placement(golden):
    from hockey_amd.evaluate import Actor, evaluate

    z = golden("stage3_actor.npz")
    actor = Actor().to(DEV)
    with torch.no_grad():
        for name, p in actor.named_parameters():
            p.copy_(torch.from_numpy(z[name.replace(".", "_")]))
    actor.eval()
    dev = evaluate(actor, episodes=20, placement="device", per_episode=True)
    host = evaluate(actor, episodes=20, placement="host", per_episode=True)
    assert np.array_equal(dev["winner"], host["winner"])
    assert dev["mean_return"] == host["mean_return"] and dev["mean_length"] == host["mean_length"]


def test_train_rounds_start_from_the_same_observations():
    from hockey_amd.td3 import TD3Config, train

    cfg = TD3Config(max_steps=4, start_steps=0, batch_size=64)
    first = {}
    for how in ("seeded", "seeded_host"):
        seen = []

        def on_step(obs, a, r, o2, d, res, seen=seen):
            seen.append(obs.clone())

        train(n_arenas=64, rounds=2, reset=how, cfg=cfg, device=DEV, seed=3, updates_per_round=0, graphs=False,
              fused=False, on_step=on_step)
        assert len(seen) == 2 * cfg.max_steps
        first[how] = [seen[k * cfg.max_steps].cpu().numpy() for k in range(2)]
    for k in range(2):
        assert np.array_equal(first["seeded"][k].view(np.uint32), first["seeded_host"][k].view(np.uint32))
    assert not np.array_equal(first["seeded"][0], first["seeded"][1])
