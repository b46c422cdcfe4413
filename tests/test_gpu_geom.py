"""hk_geom.h's four primitives on gfx950, on their own: the geometry probe (tests/native/geom_probe.hip, one lane per
case, built with the step library's flags) against the host build of the same header and the CPU oracle's functions,
word for word at tolerance zero; then the float64 laws of tests/geom_cases.py on the GPU's own outputs.  Every wave
mixes the groups of its family and the last wave is partial."""
import numpy as np
import pytest

import geom_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    c, mods = C.committed()
    L = C.gpu_probe()  # built once for the module
    return c, mods, L, C.run_all(L, c)  # one launch per primitive, into sentinel-prefilled outputs


def test_scene_table(gpu):
    c, _, L, _ = gpu
    fx, body = C.scene_table(L)
    assert np.array_equal(C.words(fx), C.words(c.table[: C.NSCENE])) and np.array_equal(body, c.body)


@pytest.mark.parametrize("family", ["D", "M", "T"])
def test_every_word_equals_host_build_and_oracle(gpu, family):
    c, _, _, g = gpu
    wg = C.words(g[family])
    assert not (wg == C.SENTINEL).any(), "a word the kernel did not write"
    cases = getattr(c, family)
    for name, probe in (("host", C.host_probe), ("oracle", C.oracle_probe)):
        ref = C.run(probe(), c.table, cases, family)
        diff = np.nonzero((wg != C.words(ref)).any(1))[0]
        assert diff.size == 0, (name, family, diff[:10], g[family][diff[:3]], ref[diff[:3]])


def test_laws_on_the_gpu_outputs(gpu):
    c, mods, _, g = gpu
    dev = C.check(c, g, mods)  # the laws and the same coverage counts
    print({k: v for k, v in sorted(dev.items()) if k != "violations"})
    # the rotating sweeps' record (SEPARATED although the model crossed, FAILED) is a function of the states and the
    # model alone: all builds agree on it when they agree on every state
    for probe in (C.host_probe, C.oracle_probe):
        assert np.array_equal(C.run(probe(), c.table, c.T, "T")["state"], g["T"]["state"])
    print("rotating sweeps (recorded, not asserted):", C.rotating_record(dev))


@pytest.mark.parametrize("family", ["D", "M", "T"])
def test_lane_order_does_not_matter(gpu, family):
    c, _, L, g = gpu
    cases = getattr(c, family)
    perm = np.random.default_rng(7).permutation(len(cases))
    again = C.run(L, c.table, cases[perm], family)
    assert np.array_equal(C.words(again), C.words(g[family])[perm])
