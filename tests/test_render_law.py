"""The renderer's coverage law on the CPU (no GPU): (A) the law reproduces the static scene of the one real pygame
frame the reference ships, (B) the host build of csrc/hk_render.h follows the law at every pixel that is not a
float32 knife edge, (C) that host source is clean under AddressSanitizer + UndefinedBehaviorSanitizer.

tests/render_ref.py is the float64 statement of the law; tests/test_gpu_render.py holds the gfx950 kernel to the host
build byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import render_host as RH
import render_ref as R
from conftest import ROOT

SIZES = [(480, 600), (120, 152), (84, 84)]
KNIFE_SHARE_CAP = 1e-3  # of a frame


def _dilate(mask, r):
    out = mask.copy()
    h, w = mask.shape
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            out[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)] |= \
                mask[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)]
    return out


def test_law_reproduces_the_reference_frame_static_scene():
    """Part A.  tests/golden/render_reference_frame.png is the reference's assets/hockeyenv1.png, a pygame frame of
    render().  With the dynamic bodies masked (its red and blue pixels and the puck's rows 140..180 x cols 355..400,
    dilated by 3 px), every pixel whose sample point is more than 1 px from every static shape boundary equals the
    law's static_only picture exactly.  Measured: 248 pixels of 288 000 differ outside the mask, all of them inside
    the 1-px band (4.04 % of the frame; the mask is 2.2 %)."""
    frame = R.reference_frame()
    index, _ = R.render(None, 480, 600, static_only=True)
    law = R.PALETTE[index]
    mask = (frame == R.PALETTE[R.P1]).all(-1) | (frame == R.PALETTE[R.P2]).all(-1)
    mask[140:181, 355:401] = True
    mask = _dilate(mask, 3)
    band = R.static_boundary_distance(480, 600) <= 1.0
    differ = (law != frame).any(-1) & ~mask
    print(f"reference frame: {int(differ.sum())} of {differ.size} pixels differ outside the mask, "
          f"{int((differ & ~band).sum())} of them outside the band; band {band.mean():.4%}, mask {mask.mean():.4%}")
    assert band.mean() <= 0.05
    assert mask.mean() <= 0.03
    assert not (differ & ~band).any()


@pytest.fixture(scope="module")
def cases():
    states = R.case_states()
    return list(states), np.stack(list(states.values()))


def test_case_states_cover_what_they_claim(cases):
    """The chosen states do put the puck on a racket, a racket on a wall and on the centre circle, and two rackets
    on each other, so draw order is exercised; and the NaN racket is absent."""
    names, S = cases
    k = names.index("puck_over_racket")
    before, _ = R.rasterise(R.dynamic_shapes(S[k])[:2], 480, 600)
    after, _ = R.render(S[k])
    assert ((before == R.P1) & (after == R.BLACK)).sum() > 100
    static, _ = R.render(None, static_only=True)
    after, _ = R.render(S[names.index("racket_over_wall_and_centre")])
    assert ((static == R.BLACK) & (after == R.P1)).sum() > 100 and ((static == R.GREY) & (after == R.P2)).sum() > 100
    k = names.index("rackets_overlap")
    only1, _ = R.rasterise(R.dynamic_shapes(S[k])[:1], 480, 600)
    after, _ = R.render(S[k])
    assert ((only1 == R.P1) & (after == R.P2)).sum() > 100
    nan, _ = R.render(S[names.index("nan_pose")])
    assert not (nan == R.P1).any() and (nan == R.P2).any()
    assert max(np.abs(S[names.index(f"random{j}")][[2, 8]]).max() for j in range(32)) > 2 * np.pi


@pytest.mark.parametrize("height,width", SIZES)
def test_host_build_follows_the_law(cases, height, width):
    """Part B.  INDEX, RGB and static_only of the host build against the float64 law: equal at every pixel that is
    not within 1e-3 px of some shape's threshold, and such knife-edge pixels are at most 0.1 % of each frame."""
    names, S = cases
    index, bad = RH.render(S, height=height, width=width, format="index")
    rgb, bad2 = RH.render(S, height=height, width=width, format="rgb")
    assert bad == 0 and bad2 == 0
    palette = RH.palette()
    assert np.array_equal(palette, R.PALETTE)
    assert np.array_equal(palette[index], rgb)
    worst = 0.0
    for k, name in enumerate(names):
        law, knife = R.render(S[k], height, width)
        worst = max(worst, knife.mean())
        assert knife.mean() <= KNIFE_SHARE_CAP, (name, knife.mean())
        wrong = (law != index[k]) & ~knife
        assert not wrong.any(), (name, int(wrong.sum()), np.argwhere(wrong)[:5].tolist())
    law, knife = R.render(None, height, width, static_only=True)
    assert knife.mean() <= KNIFE_SHARE_CAP
    for fmt in ("index", "rgb"):
        got, _ = RH.render(S[:2], height=height, width=width, format=fmt, static_only=True)
        want = law if fmt == "index" else R.PALETTE[law]
        for k in range(2):
            assert not ((want != got[k]).reshape(height, width, -1).any(-1) & ~knife).any(), fmt
    print(f"{height} x {width}: worst knife-edge share {worst:.5%}")


def test_host_build_bad_index_and_rejections(cases):
    _, S = cases
    out = np.full((4, 84, 84, 3), 0xA5, np.uint8)
    got, bad = RH.render(S, idx=[3, len(S), -7, 0], height=84, width=84, out=out)
    assert bad == 2
    assert (got[1] == 0xA5).all() and (got[2] == 0xA5).all()
    want, _ = RH.render(S[[3, 0]], height=84, width=84)
    assert np.array_equal(got[[0, 3]], want)
    for h, w in ((84, 86), (2, 84), (84, 4100)):
        with pytest.raises(ValueError):
            RH.render(S[:1], height=h, width=w, out=np.zeros((1, h, w, 3), np.uint8))


def test_host_source_under_asan_ubsan(cases, tmp_path):
    """Part C.  tests/native/render_sanity.cpp: a stand-alone program over the same states, every format, flag and
    size and the bad-index case, compiled with -fsanitize=address,undefined against the host source and run as a
    subprocess."""
    _, S = cases
    states = tmp_path / "states.bin"
    S.astype(np.float32).tofile(states)
    exe = str(tmp_path / "render_sanity")
    csrc = os.path.join(ROOT, "hockey-env_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-ffp-contract=off",
                           "-fno-fast-math", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I", os.path.join(ROOT, "include"), "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "render_sanity.cpp"),
                           os.path.join(csrc, "hostcheck", "hk_render_host.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(states)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "render sanity: ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
