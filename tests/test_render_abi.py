"""libhockey_render.so loads without a GPU, exports what include/hockey_render.h declares, and rejects bad
arguments on the host before any HIP call; the binding has no CPU path."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _declared():
    src = open(os.path.join(ROOT, "include", "hockey_render.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(hkr_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def L():
    from hockey_amd import render as HR

    if not os.path.exists(HR.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "hockey-env_amd", "csrc"), "render"])
    return HR.lib()


def test_render_library_exports_every_declared_symbol(L):
    from hockey_amd import render as HR

    assert not [n for n in _declared() if not hasattr(L, n)]
    assert set(_declared()) == set(HR.EXPORTS)
    pal = np.zeros((6, 3), np.uint8)
    L.hkr_palette(pal.ctypes.data)
    assert pal.tolist() == [list(c) for c in HR.PALETTE]


def test_render_rejects_invalid_arguments_before_any_launch(L):
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(state=p, n=1, idx=None, m=1, h=8, w=8, fmt=0, flags=0, out=p):
        rc = L.hkr_render(state, n, idx, m, h, w, fmt, flags, out, None, None)
        return rc, L.hkr_last_error().decode()

    for kw, msg in ((dict(state=None), "state is NULL"), (dict(out=None), "out is NULL"),
                    (dict(w=10), "multiple of 4"), (dict(h=3), "[4, 4096]"), (dict(w=4100), "[4, 4096]"),
                    (dict(h=4097), "[4, 4096]"), (dict(fmt=2), "format"), (dict(flags=2), "flags"),
                    (dict(m=-1), "negative"), (dict(m=2), "exceeds n_states"),
                    (dict(out=ctypes.c_void_p(p.value + 1)), "aligned")):
        rc, err = call(**kw)
        assert rc == 1 and err.startswith("hkr_render:") and msg in err, (kw, rc, err)
    assert call(m=0)[0] == 0  # nothing to draw: no device is touched


def test_render_binding_has_no_cpu_path(monkeypatch, tmp_path):
    import torch

    from hockey_amd import _native as N
    from hockey_amd import render as HR

    with pytest.raises(N.HockeyNativeError):
        HR.render_states(torch.zeros((1, 18)))
    monkeypatch.setattr(HR, "LIB_PATH", str(tmp_path / "missing.so"))
    monkeypatch.setattr(HR, "_lib", None)
    with pytest.raises(N.HockeyNativeError):
        HR.lib()
