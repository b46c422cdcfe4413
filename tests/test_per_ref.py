"""tests/per_ref.py (the numpy float64 reference of prioritized replay sampling) pinned on the CPU, and the host side
of the hkl_per_* ABI (include/hockey_learner.h): struct layouts and argument checks.  No GPU needed.

* per_ref.sample gives PrioritizedRing.sample_indices' slots for the exact-sum inputs of tests/test_gpu_per.py (fed the
  same uniforms), per_ref.importance its importance weights, and per_ref.RefRing / write_back its weights over a push /
  sample / update sequence that wraps;
* the exact-sum construction is what it claims: sequential and reversed-block float64 totals are identical and
  u T == cdf[j] bitwise for u = cdf[j] / T;
* per_ref.check_general accepts the sequential float64 cumsum with no draw in its excluded band.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import per_ref as P  # noqa: E402
from hockey_amd import learner_hip as LH  # noqa: E402
from hockey_amd.td3 import PrioritizedRing  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _blk():
    return LH.lib().hkl_per_block()


def capacities():
    return P.capacities(_blk())


def fills(cap):
    return P.fills(cap, _blk())


def _cpu_ring(w, size):
    ring = PrioritizedRing(len(w), device="cpu")
    ring.w.copy_(torch.from_numpy(w))
    ring.size = size
    ring.size_t.fill_(size)
    return ring


def test_fill_levels_cover_full_mid_block_and_block_edge():
    b = _blk()
    for cap in capacities():
        f = fills(cap)
        assert cap in f
        if cap > b:
            assert any(s % b == 0 and s < cap for s in f) and any(s % b for s in f), (cap, f)


@pytest.mark.parametrize("ci", range(5))
def test_per_ref_indices_equal_prioritized_ring_on_exact_sums(ci, monkeypatch):
    cap = capacities()[ci]
    for size in fills(cap):
        w = P.dyadic_weights(size, 100 + ci, cap)
        u = P.exact_draws(w, size, 7)
        ring = _cpu_ring(w, size)
        monkeypatch.setattr(torch, "rand", lambda *a, **k: torch.from_numpy(u))
        got = ring.sample_indices(len(u)).numpy()
        monkeypatch.undo()
        assert np.array_equal(got, P.sample(w, size, u)), (cap, size)


@pytest.mark.parametrize("ci", range(5))
def test_exact_sum_inputs_are_exact_in_any_order(ci):
    cap, b = capacities()[ci], _blk()
    p = P.sanitised(P.dyadic_weights(cap, 100 + ci), cap)
    seq = np.cumsum(p)
    rev = 0.0
    for lo in reversed(range(0, cap, b)):
        rev += float(np.sum(p[lo:lo + b][::-1]))
    T = seq[-1]
    assert rev == T and np.log2(T) == int(np.log2(T))
    u = seq / T
    assert np.array_equal((u * T).view(np.uint64), seq.view(np.uint64))


def test_importance_weights_match_prioritized_ring(monkeypatch):
    size = 3000
    w = P.general_weights(size, "a", 3)
    w[:7] = 1.0
    ring = _cpu_ring(w, size)
    u = np.random.default_rng(0).random(257)
    monkeypatch.setattr(torch, "rand", lambda *a, **k: torch.from_numpy(u))
    *_, iw = ring.sample(257)
    monkeypatch.undo()
    ref = P.importance(w, ring.last.numpy(), size, ring.beta)
    assert np.abs(iw.numpy() - ref).max() <= 8 * 2.0 ** -24  # the float32 evaluation of the same expressions


def test_ref_ring_weights_equal_prioritized_ring_over_a_wrapping_sequence():
    cap = 3 * _blk() + 17
    ring, ref = PrioritizedRing(cap, device="cpu"), P.RefRing(cap)
    rng = np.random.default_rng(5)
    z = lambda n, *s: torch.zeros((n,) + s)  # noqa: E731
    for step, n in enumerate([700, 1500, 900, 400, 1300, 64]):  # wraps at the third push; full from then on
        ring.push(z(n, 18), z(n, 4), z(n), z(n, 18), z(n))
        ref.push(n)
        assert np.array_equal(ring.w.numpy(), ref.w) and (ring.size, ring.pos) == (ref.size, ref.pos), step
        torch.manual_seed(step)
        i = ring.sample_indices(256).numpy().copy()
        assert i.max() < ref.size
        i[:40] = i[40]  # a slot drawn many times: the last occurrence wins
        ring.last = torch.from_numpy(i)
        td = np.exp(rng.normal(0, 6, 256)).astype(np.float32)
        ring.update_priorities(torch.from_numpy(td))
        ref.update(i, td)
        assert np.array_equal(ring.w.numpy(), ref.w), step
    assert ref.size == cap and ref.w.min() >= 1e-6 and (ref.w == 1e6).any()


@pytest.mark.parametrize("regime", ["a", "b"])
def test_check_general_accepts_the_sequential_cumsum(regime):
    size = 3 * _blk() + 17
    w = P.general_weights(size, regime, 11)
    u = np.random.default_rng(12).random(4096)
    assert P.check_general(w, size, u, P.sample(w, size, u)) <= 1
    wrong = P.sample(w, size, u)
    wrong[5] = (wrong[5] + 1) % size
    with pytest.raises(AssertionError):
        P.check_general(w, size, u, wrong)


# ------------------------------------------------------------------------------------------------------ ABI
def test_per_ctypes_struct_layout_matches_header(tmp_path):
    """Sizes and field offsets of the hkl_per_* structs as the C compiler lays them out from the header."""
    probes = {"Per": "hkl_per", "PerSampleIO": "hkl_per_sample_io", "PerUpdateIO": "hkl_per_update_io"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hockey_learner.h"', "int main(void) {",
             '  printf("block %d\\n", HKL_PER_BLOCK);']
    for py, cname in probes.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in getattr(LH, py)._fields_:
            lines.append(f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    want = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert _blk() == int(want["block"])
    for py, cname in probes.items():
        S = getattr(LH, py)
        assert ctypes.sizeof(S) == int(want[cname]), cname
        for f, _ in S._fields_:
            assert getattr(S, f).offset == int(want[f"{cname}.{f}"]), (cname, f)


def test_per_entry_points_reject_bad_arguments_before_any_launch():
    """Null pointers, cap <= 0, batch <= 0 and ranges outside the ring return HKL_E_INVALID on the host: nothing here
    reaches a HIP call."""
    L = LH.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fields = [f for f, _ in LH.Per._fields_]

    def per(**kw):
        s = LH.Per(2048, p, p, p, p, p, p, p)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    bad_pers = [per(cap=0), per(cap=-3)] + [per(**{f: None}) for f in fields[1:]]
    for bp in bad_pers:
        assert L.hkl_per_refresh(bp, 0, 1, None) == 1
        assert L.hkl_per_push(bp, 0, 1, 1, None) == 1
        assert L.hkl_per_sample(LH.PerSampleIO(bp, 4, 0, p, p, p, p, 0.2, 0.3, p, 0.15), None) == 1
        assert L.hkl_per_weights(LH.PerSampleIO(bp, 4, 0, p, p, p, p, 0.2, 0.3, p, 0.15), None) == 1
        assert L.hkl_per_update(LH.PerUpdateIO(bp, 4, p, p), None) == 1
    ok = per()
    assert L.hkl_per_refresh(None, 0, 1, None) == 1
    for lo, n in ((-1, 1), (0, 0), (0, 2049), (2048, 1), (2000, 49)):
        assert L.hkl_per_refresh(ok, lo, n, None) == 1, (lo, n)
    for pos, n, after in ((-1, 1, 1), (2048, 1, 1), (0, 0, 1), (0, 2049, 2048), (0, 8, 7), (0, 8, 2049)):
        assert L.hkl_per_push(ok, pos, n, after, None) == 1, (pos, n, after)
    assert L.hkl_per_sample(None, None) == 1 and L.hkl_per_weights(None, None) == 1 and L.hkl_per_update(None, None) == 1
    for batch in (0, -256, 1 << 31):
        assert L.hkl_per_sample(LH.PerSampleIO(ok, batch, 0, p, p, p, p, 0.2, 0.3, p, 0.15), None) == 1
        assert L.hkl_per_weights(LH.PerSampleIO(ok, batch, 0, p, p, p, p, 0.2, 0.3, p, 0.15), None) == 1
        assert L.hkl_per_update(LH.PerUpdateIO(ok, batch, p, p), None) == 1
    assert L.hkl_per_sample(LH.PerSampleIO(ok, 4, 0, None, None, p, p, 0.2, 0.3, p, 0.15), None) == 1  # no u, no counter
    assert L.hkl_per_sample(LH.PerSampleIO(ok, 4, 0, p, p, None, p, 0.2, 0.3, p, 0.15), None) == 1  # no idx
    assert L.hkl_per_weights(LH.PerSampleIO(ok, 4, 0, p, p, p, p, 0.2, 0.3, None, 0.15), None) == 1  # no iw
    assert L.hkl_per_update(LH.PerUpdateIO(ok, 4, None, p), None) == 1
    assert L.hkl_per_update(LH.PerUpdateIO(ok, 4, p, None), None) == 1


def test_device_ring_is_gpu_only_and_train_validates_per_sampler():
    from hockey_amd import _native
    from hockey_amd.td3 import DevicePrioritizedRing, TD3Config, train

    with pytest.raises(_native.HockeyNativeError):
        DevicePrioritizedRing(64, device="cpu")
    with pytest.raises(ValueError):
        train(n_arenas=1, rounds=0, device="cpu", cfg=TD3Config(prioritized_replay=True), per_sampler="numpy",
              env=object())
