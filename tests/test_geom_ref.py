"""hk_geom.h's four primitives on their own, on the CPU: the oracle's functions and the host build of the header
run through the geometry probe (tests/native/geom_probe.h) must agree on every output word, and each must obey the
float64 laws of tests/geom_cases.py (model: tests/geom_ref.py).  A few cases with closed-form answers pin the probe
and the model themselves."""
import numpy as np
import pytest

import geom_cases as C
import geom_ref as G


@pytest.fixture(scope="module")
def batch():
    c, mods = C.committed()
    return c, mods, C.run_all(C.oracle_probe(), c), C.run_all(C.host_probe(), c)


def test_three_builds_export_the_same_scene():
    fo, bo = C.scene_table(C.oracle_probe())
    fh, bh = C.scene_table(C.host_probe())
    assert np.array_equal(C.words(fo), C.words(fh)) and np.array_equal(bo.view(np.uint32), bh.view(np.uint32))
    assert [int(f["count"]) for f in fo] == [4] * 10 + [7, 7, 1] and int(fo[C.F_PK]["circle"]) == 1


def test_oracle_and_host_build_agree_on_every_word(batch):
    c, _, o, h = batch
    for k in "DMT":
        wo, wh = C.words(o[k]), C.words(h[k])
        assert not (wo == C.SENTINEL).any() and not (wh == C.SENTINEL).any(), k  # every word was written
        diff = np.nonzero((wo != wh).any(1))[0]
        assert diff.size == 0, (k, diff[:10], o[k][diff[:3]], h[k][diff[:3]])


@pytest.mark.parametrize("build", ["oracle", "host"])
def test_laws(batch, build):
    c, mods, o, h = batch
    dev = C.check(c, o if build == "oracle" else h, mods)
    print({k: v for k, v in sorted(dev.items()) if k != "violations"})
    print("rotating sweeps (recorded, not asserted):", C.rotating_record(dev))


def test_rotating_sweep_record_agrees(batch):
    c, mods, o, h = batch
    assert np.array_equal(o["T"]["state"], h["T"]["state"])


def test_generator_is_seeded():
    c, _ = C.committed()
    c2 = C.Cases(0)
    for a, b in ((c.table, c2.table), (c.D, c2.D), (c.M, c2.M), (c.T, c2.T)):
        assert np.array_equal(C.words(a), C.words(b))
    waves = [set(c.Mgroup[i:i + 64]) for i in range(0, len(c.M), 64)]
    assert min(len(w) for w in waves[:-1]) >= 4  # every full wave mixes groups


# ------------------------------------------------------------------------------------------------ closed forms
def _table():
    sq = np.zeros((), C.FIX)
    v = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]], np.float32)
    sq["count"], sq["radius"] = 4, np.float32(G.POLY_RADIUS)
    sq["vx"][:4], sq["vy"][:4] = v[:, 0], v[:, 1]
    sq["nx"][:4], sq["ny"][:4] = (0, 1, 0, -1), (-1, 0, 1, 0)
    ci = np.zeros((), C.FIX)
    ci["circle"], ci["count"], ci["radius"] = 1, 1, 0.6
    small = ci.copy()
    small["radius"] = 0.25
    return np.array([sq, ci, small], C.FIX)


def _pose(fA, fB, xb, th=0.0):
    r = np.zeros(1, C.POSE)
    r["fA"], r["fB"] = fA, fB
    r["xa"] = (0, 0, 0, 1)
    r["xb"] = (xb[0], xb[1], np.sin(th), np.cos(th))
    return r


@pytest.mark.parametrize("probe", [C.oracle_probe, C.host_probe], ids=["oracle", "host"])
def test_closed_forms(probe):
    L, tab = probe(), _table()
    # a unit square beside a unit square, 0.5 apart: parallel edges
    d = C.run(L, tab, _pose(0, 0, (1.5, 0.25)), "D")[0]
    assert d["dist"] == np.float32(0.5) and d["dist_radii"] == np.float32(0.5) - np.float32(0.02)
    assert d["count"] == 2
    # ... 0.015 apart (inside the two skins): a two-point face-A manifold on A's +x face
    m = C.run(L, tab, _pose(0, 0, (1.015, 0.25)), "M")[0]
    assert (m["type"], m["count"]) == (1, 2) and tuple(m["ln"]) == (1.0, 0.0) and tuple(m["lp"]) == (0.5, 0.0)
    # B's -x face, clipped at A's upper end pushed out by the total radius (y = 0.52), in B's frame
    assert np.allclose(sorted([m["p0"][1], m["p1"][1]]), [-0.5, 0.52 - 0.25], atol=1e-6, rtol=0)
    assert np.allclose([m["p0"][0], m["p1"][0]], -0.5, atol=1e-6, rtol=0) and m["id0"] != m["id1"]
    assert C.run(L, tab, _pose(0, 0, (1.03, 0.25)), "M")[0]["count"] == 0
    # a circle at the corner (0.5, 0.5), its centre 0.5 away along (0.6, 0.8)
    m = C.run(L, tab, _pose(0, 1, (0.8, 0.9)), "M")[0]  # radius 0.6: touches
    assert (m["type"], m["count"], m["id0"]) == (1, 1, 0) and tuple(m["lp"]) == (0.5, 0.5)
    assert np.allclose(m["ln"], (0.6, 0.8), atol=2e-7, rtol=0)
    assert C.run(L, tab, _pose(0, 2, (0.8, 0.9)), "M")[0]["count"] == 0  # radius 0.25: 0.5 > 0.26
    d = C.run(L, tab, _pose(0, 1, (0.8, 0.9)), "D")[0]
    assert abs(float(d["dist"]) - 0.5) < 1e-7 and d["count"] == 1 and d["iA"][0] == 2
    # a square translating at `speed` towards a square `gap` away: t = (gap - target) / speed
    gap, speed = 1.0, 2.0
    target = G.toi_target(2 * G.POLY_RADIUS)
    assert abs(target - G.LINEAR_SLOP) < 1e-15  # max(linearSlop, 0.02 - 3 linearSlop)
    r = np.zeros(1, C.TOI)
    r["fA"], r["fB"], r["tMax"] = 0, 0, 1.0
    r["sB"] = (0, 0, 1.0 + gap, 0.25, 1.0 + gap - speed, 0.25, 0, 0)
    o = C.run(L, tab, r, "T")[0]
    assert o["state"] == C.TOUCHING and abs(float(o["t"]) - (gap - target) / speed) <= G.TOI_TOL / speed + 1e-6
    r["sB"] = (0, 0, 1.0 + gap, 0.25, 1.0 + gap - 0.5, 0.25, 0, 0)  # stops short
    o = C.run(L, tab, r, "T")[0]
    assert (o["state"], o["t"]) == (C.SEPARATED, 1.0)


def test_model_closed_forms():
    sq = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]], np.float32)
    P = G.world(sq, (0, 0, 0, 1))
    d, s = G.distance(P, G.world(sq, (1.5, 0.25, 0, 1)))
    assert d[0] == 0.5 and s[0] == 0.5 and G.closest_class(P, G.world(sq, (1.5, 0.25, 0, 1))) == "par"
    th = np.pi / 4  # a diamond: its left vertex at (1.5 - sqrt(0.5), 0) against the +x face
    Q = G.world(sq, (1.5, 0.0, np.sin(th), np.cos(th)))
    d, s = G.distance(P, Q)
    assert abs(d[0] - (1.0 - np.sqrt(0.5))) < 1e-7 and G.closest_class(P, Q) == "b_on_a"
    d, s = G.distance(P, G.world(sq, (0.75, 0.0, 0, 1)))
    assert d[0] == 0.0 and s[0] == -0.25  # overlap depth
    d, s = G.distance(P, np.array([[[0.8, 0.9]]]))
    assert abs(d[0] - 0.5) < 1e-15
    m = G.SweepModel(sq, (0, 0, 0, 0, 0, 0, 0, 0), sq, (0, 0, 2.0, 0.25, 0.0, 0.25, 0, 0))
    assert abs(m.first_below(0.5) - 0.25) < 1e-3 and m.min_upto(1.0) == 0.0 and abs(m.S([0.1])[0] - 0.8) < 1e-12
