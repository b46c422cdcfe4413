"""GPU tests of the renderer (include/hockey_render.h, hockey_amd.render): the gfx950 kernel writes the bytes of
the host build of the same per-pixel source (tests/render_host.py), which tests/test_render_law.py holds to the
float64 law; rendering reads the live state and leaves it alone; the facade returns the reference's frame shape."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import render_host as RH  # noqa: E402
import render_ref as R  # noqa: E402

SIZES = [(480, 600), (120, 152), (84, 84)]
DEV = "cuda:0"


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def states():
    """130 raw state rows: the law test's cases, then seeded random rows over the rink (row 129 among them)."""
    from hockey_amd.constants import H, W

    rows = list(R.case_states().values())
    rng = np.random.default_rng(77)
    while len(rows) < 130:
        xs, ys, an = rng.uniform(0.0, W, 3), rng.uniform(0.0, H, 3), rng.uniform(-7.0, 7.0, 2)
        rows.append(R.raw_state((xs[0], ys[0], an[0]), (xs[1], ys[1], an[1]), (xs[2], ys[2])))
    S = np.stack(rows).astype(np.float32)
    S.setflags(write=False)
    return S


@pytest.mark.parametrize("height,width", SIZES)
@pytest.mark.parametrize("fmt", ["rgb", "index"])
def test_kernel_bytes_equal_the_host_build(states, height, width, fmt):
    """Part 1: 5 frames through idx (out of order, one duplicate, row 129), twice: the second call reuses the cached
    background."""
    from hockey_amd.render import render_states

    idx = [129, 7, 40, 7, 0]
    want, bad = RH.render(states, idx=idx, height=height, width=width, format=fmt)
    assert bad == 0
    st = torch.tensor(states, device=DEV)
    it = torch.as_tensor(idx, dtype=torch.int32, device=DEV)
    first = _np(render_states(st, it, height, width, fmt))
    second = _np(render_states(st, it, height, width, fmt))
    assert first.shape == want.shape and first.dtype == np.uint8
    assert np.array_equal(first, want)
    assert np.array_equal(second, want)
    got_static = _np(render_states(st, it[:1], height, width, fmt, static_only=True))
    want_static, _ = RH.render(states, idx=idx[:1], height=height, width=width, format=fmt, static_only=True)
    assert np.array_equal(got_static, want_static)


@pytest.mark.parametrize("height,width", [(24, 32), (36, 52), (84, 100)])
def test_kernel_all_rows_partial_workgroups(states, height, width):
    """Part 1: idx = NULL over all 130 rows, both formats, at 24 x 32 (192 quads: less than one round of a
    workgroup's 256 lanes), 36 x 52 (468 quads: a full round and a partial one) and 84 x 100 (2100 quads: a full
    workgroup of 8 rounds plus a partial one)."""
    from hockey_amd.render import PALETTE, render_states

    st = torch.tensor(states, device=DEV)
    for fmt in ("rgb", "index"):
        want, _ = RH.render(states, height=height, width=width, format=fmt)
        got = _np(render_states(st, None, height, width, fmt))
        assert np.array_equal(got, want), fmt
    assert np.array_equal(np.array(PALETTE, np.uint8)[got], _np(render_states(st, None, height, width, "rgb")))


def test_render_reads_the_live_state_and_leaves_it_alone():
    """Part 2: after 40 strong-vs-strong steps (rackets rotate: an origin / centre-of-mass mix-up would show),
    env.render equals the host render of env.get_state(); and the next 10 steps are bit-identical with and without
    render calls in between."""
    from hockey_amd.vec_env import VecHockeyEnv

    n = 130
    env, twin = (VecHockeyEnv(n, device=DEV, policies=("strong", "strong"), seed=21) for _ in range(2))
    for e in (env, twin):
        e.reset(seeds=list(range(n)))
        for _ in range(40):
            e.step()
    st = _np(env.get_state()[0])
    assert np.abs(st[:, [2, 8]]).max() > 0.05  # the rackets did turn
    indices = [129, 3, 64, 3]
    got = _np(env.render(indices))
    want, _ = RH.render(st, idx=indices)
    assert got.shape == (4, 480, 600, 3) and np.array_equal(got, want)
    got = _np(env.render(height=84, width=84, format="index"))
    want, _ = RH.render(st, height=84, width=84, format="index")
    assert np.array_equal(got, want)
    for k in range(10):
        a, b = env.step(), twin.step()
        assert np.array_equal(_np(a.obs).view(np.uint32), _np(b.obs).view(np.uint32)), k
        assert np.array_equal(_np(a.reward).view(np.uint32), _np(b.reward).view(np.uint32)), k
        env.render([k], height=84, width=84)
    for x, y in zip(env.get_state(), twin.get_state()):
        assert np.array_equal(_np(x).view(np.uint32), _np(y).view(np.uint32))
    env.close()
    twin.close()


def test_facade_rgb_array():
    """Part 3: HockeyEnv.render("rgb_array") is the reference's (480, 600, 3) uint8 frame, equal to the batched render
    of the same state after reset(seed=3) and after 5 steps (through the step server); "human" and None warn and
    return None."""
    from hockey_amd.hockey_env import HockeyEnv
    from hockey_amd.render import render_states

    env = HockeyEnv()
    env.reset(seed=3)
    for steps in (0, 5):
        for k in range(steps):
            env.step(np.array([0.5, -0.3, 0.8, 0.0, -0.6, 0.2, -0.9, 0.0]))
        frame = env.render("rgb_array")
        assert isinstance(frame, np.ndarray) and frame.shape == (480, 600, 3) and frame.dtype == np.uint8
        st = env._vec.get_state()[0]
        assert np.array_equal(frame, _np(render_states(st))[0])
        want, _ = RH.render(_np(st))
        assert np.array_equal(frame, want[0])
        assert (frame == R.PALETTE[R.P1]).all(-1).sum() > 1000 and (frame == R.PALETTE[R.P2]).all(-1).sum() > 1000
    with pytest.warns(UserWarning, match="nothing is drawn"):
        assert env.render("human") is None
    with pytest.warns(UserWarning, match="rendering mode"):
        assert env.render(None) is None
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        env.render("rgb_array")  # draws without a warning
    env.close()


def test_bad_index_leaves_its_frame_and_counts_once(states):
    """Part 4."""
    from hockey_amd.render import render_states

    st = torch.tensor(states, device=DEV)
    idx = torch.as_tensor([5, 130, -1, 129], dtype=torch.int32, device=DEV)
    out = torch.full((4, 36, 52, 3), 0xA5, dtype=torch.uint8, device=DEV)
    bad = torch.zeros(1, dtype=torch.int64, device=DEV)
    render_states(st, idx, 36, 52, out=out, bad_index_count=bad)
    got = _np(out)
    assert int(bad.item()) == 2
    assert (got[1] == 0xA5).all() and (got[2] == 0xA5).all()
    want, _ = RH.render(states, idx=[5, 129], height=36, width=52)
    assert np.array_equal(got[[0, 3]], want)


def test_render_replays_from_a_graph(states):
    """Part 5: one hkr_render captured in a torch.cuda.graph (a single branch) and replayed equals the eager output,
    also after the state buffer's contents changed."""
    from hockey_amd.render import render_states

    st = torch.as_tensor(states[:64].copy(), device=DEV)
    out = torch.zeros((64, 84, 84, 3), dtype=torch.uint8, device=DEV)
    eager = _np(render_states(st, None, 84, 84))  # also builds the size's background, outside the capture
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        render_states(st, None, 84, 84, out=out)
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        render_states(st, None, 84, 84, out=out)
    out.zero_()
    graph.replay()
    assert np.array_equal(_np(out), eager)
    st.copy_(torch.as_tensor(states[64:128].copy(), device=DEV))
    graph.replay()
    want, _ = RH.render(states[64:128], height=84, width=84)
    assert np.array_equal(_np(out), want)
