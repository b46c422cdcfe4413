"""csrc/hk_seed.h against numpy, layer by layer, on the host build (no GPU): the SeedSequence state, PCG64's raw
words and doubles, and the seeded reset placement -- every word equal over tests/seed_cases.py's list.  A wrong
hash constant shows at the first test, not three layers up.  The last test runs the list through the header under
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program."""
import os
import subprocess

import numpy as np

import seed_cases as SC


def _seeds_arg():
    return np.ascontiguousarray(SC.SEEDS)


def test_seed_sequence_state_is_numpys():
    L = SC.host_probe()
    seeds = _seeds_arg()
    got = np.zeros((len(seeds), 4), np.uint64)
    L.sp_state(seeds.ctypes.data, len(seeds), got.ctypes.data)
    want = np.stack([np.random.SeedSequence(int(s)).generate_state(4, np.uint64) for s in seeds])
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, (len(bad), int(seeds[bad[0]]), got[bad[0]], want[bad[0]])


def test_pcg64_words_and_doubles_are_numpys():
    L = SC.host_probe()
    seeds = _seeds_arg()
    raw = np.zeros((len(seeds), SC.N_RAW), np.uint64)
    dbl = np.zeros((len(seeds), SC.N_DOUBLES), np.float64)
    L.sp_raw(seeds.ctypes.data, len(seeds), raw.ctypes.data)
    L.sp_double(seeds.ctypes.data, len(seeds), dbl.ctypes.data)
    want_raw = np.stack([np.random.PCG64(np.random.SeedSequence(int(s))).random_raw(SC.N_RAW) for s in seeds])
    bad = np.nonzero((raw != want_raw).any(1))[0]
    assert bad.size == 0, (len(bad), int(seeds[bad[0]]), raw[bad[0]], want_raw[bad[0]])
    want_dbl = np.zeros_like(dbl)
    for i, s in enumerate(seeds):
        g = np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(s))))
        want_dbl[i] = [g.random() for _ in range(SC.N_DOUBLES)]  # one at a time, as reset draws them
    assert np.array_equal(dbl.view(np.uint64), want_dbl.view(np.uint64))
    # the words above cover every rotation count state >> 122, the shift-by-zero case included: read numpy's state
    rots = set()
    for s in seeds[:400]:
        bg = np.random.PCG64(np.random.SeedSequence(int(s)))
        for _ in range(SC.N_RAW):
            bg.random_raw(1)
            rots.add(bg.state["state"]["state"] >> 122)
    assert rots == set(range(64))


def test_seeded_placement_is_the_host_placement():
    L = SC.host_probe()
    rows, want = SC.cases(), SC.reference()
    got = np.zeros(len(rows), SC.PLACEMENT)
    assert L.sp_placement(rows.ctypes.data, len(rows), got.ctypes.data) == 0
    same = (got["p6"].view(np.uint32) == want["p6"].view(np.uint32)).all(1) & (got["max_t"] == want["max_t"])
    bad = np.nonzero(~same)[0]
    assert bad.size == 0, (len(bad), rows[bad[0]], got[bad[0]], want[bad[0]])
    # the list exercises what it claims: both puck sides in NORMAL, a non-zero shot only in TRAIN_DEFENSE
    nrm = rows["mode"] == 0
    assert (want["p6"][nrm & (rows["one_starts"] == 1), 2] < 5.0).all()
    assert (want["p6"][nrm & (rows["one_starts"] == 0), 2] > 5.0).all()
    assert (want["p6"][rows["mode"] == 2, 4] != 0).all() and (want["p6"][rows["mode"] != 2, 4:] == 0).all()
    assert set(want["max_t"][nrm]) == {250} and set(want["max_t"][~nrm]) == {80}


def test_header_under_asan_ubsan(tmp_path):
    """tests/native/seed_sanity.cpp: the case list through all three layers of the header, compiled with
    -fsanitize=address,undefined as a stand-alone program and run as a subprocess (never loaded into python)."""
    rows, want = SC.cases(), SC.reference()
    cases_bin, want_bin = tmp_path / "cases.bin", tmp_path / "want.bin"
    rows.tofile(cases_bin)
    want.tofile(want_bin)
    exe = str(tmp_path / "seed_sanity")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", *SC.host_flags(),
                           "-Wno-unknown-pragmas", "-I", SC.CSRC, "-I", SC.NATIVE, "-o", exe,
                           os.path.join(SC.NATIVE, "seed_sanity.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(cases_bin), str(want_bin)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"seed sanity: ok ({len(rows)} cases" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
