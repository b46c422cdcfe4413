"""Prioritized replay in a population, without a GPU: the grouped hkl_per_* calls' host-side argument checks (they
return before any launch) and what still refuses a CPU device."""
import ctypes

import pytest
import torch

from hockey_amd import _native, learner_hip as LH
from hockey_amd.population import PopulationLearner, PopulationPrioritizedRing
from hockey_amd.td3 import TD3, PrioritizedRing, TD3Config

FAKE = 4096  # a non-null, 16-byte aligned "device" address: never dereferenced, the checks fail first


def _per(cap):
    return LH.Per(cap, *([FAKE] * 7))


def _sample_io(cap=2048, batch=256):
    return LH.PerSampleIO(_per(cap), batch, 1, FAKE, None, FAKE, FAKE, 0.2, 0.5, FAKE, 0.15)


def _update_io(cap=2048, batch=256):
    return LH.PerUpdateIO(_per(cap), batch, FAKE, FAKE)


def _calls(L):
    """name -> (a valid member's struct maker, call(host array, dev, n_members, **push arguments))."""
    push = lambda h, dev, n, max_n=8, pos=FAKE: L.hkl_per_push_group(h, dev, pos, FAKE, FAKE, max_n, n, None)  # noqa: E731
    return {
        "hkl_per_sample_group": (LH.PerSampleIO, _sample_io, lambda h, dev, n: L.hkl_per_sample_group(h, dev, n, None)),
        "hkl_per_weights_group": (LH.PerSampleIO, _sample_io,
                                  lambda h, dev, n: L.hkl_per_weights_group(h, dev, n, None)),
        "hkl_per_update_group": (LH.PerUpdateIO, _update_io, lambda h, dev, n: L.hkl_per_update_group(h, dev, n, None)),
        "hkl_per_refresh_group": (LH.Per, lambda cap=2048, batch=None: _per(cap),
                                  lambda h, dev, n: L.hkl_per_refresh_group(h, dev, n, None)),
        "hkl_per_push_group": (LH.Per, lambda cap=2048, batch=None: _per(cap), push),
    }


def test_grouped_per_calls_check_their_arguments_on_the_host():
    """Each of the five calls refuses n_members of 0 and 65, a null dev, a zeroed member, unequal cap and (where the
    struct has one) unequal batch, the push call also max_n of 0, max_n past cap and a null pos: return code 1 and a
    message that starts with the call's name and names the member at fault.  The checks fail before anything is
    launched, so no GPU is needed to see it (the pointers are fakes)."""
    L = LH.lib()
    dev = ctypes.c_void_p(FAKE)

    def refused(name, rc, member=None):
        msg = L.hkl_last_error().decode()
        assert rc == 1 and msg.startswith(name) and len(msg) > len(name) + 2, (name, rc, msg)
        if member is not None:
            assert f"member {member}" in msg, (name, msg)

    for name, (struct, make, call) in _calls(L).items():
        good = (struct * 65)(*[make() for _ in range(65)])
        for n in (0, 65):
            refused(name, call(good, dev, n))
        refused(name, call(good, None, 3))
        refused(name, call((struct * 3)(), dev, 3), member=0)  # zeroed members
        h = (struct * 3)(make(), make(), make())
        (h[1].per if hasattr(h[1], "per") else h[1]).w = None
        refused(name, call(h, dev, 3), member=1)
        h = (struct * 3)(make(), make(), make())
        (h[2].per if hasattr(h[2], "per") else h[2]).w = FAKE + 4  # a member's weights off the float4 alignment
        refused(name, call(h, dev, 3), member=2)
        refused(name, call((struct * 3)(make(), make(), make(cap=4096)), dev, 3), member=2)
        assert "cap" in L.hkl_last_error().decode()
        if hasattr(struct, "batch"):
            refused(name, call((struct * 3)(make(), make(batch=512), make()), dev, 3), member=1)
            assert "batch" in L.hkl_last_error().decode()
            refused(name, call((struct * 3)(make(batch=0), make(batch=0), make(batch=0)), dev, 3), member=0)
    # what only some calls have
    push = _calls(L)["hkl_per_push_group"][2]
    good = (LH.Per * 3)(_per(2048), _per(2048), _per(2048))
    for max_n in (0, 2049):
        refused("hkl_per_push_group", push(good, dev, 3, max_n=max_n))
        assert "max_n" in L.hkl_last_error().decode()
    refused("hkl_per_push_group", push(good, dev, 3, pos=None))
    h = (LH.PerSampleIO * 2)(_sample_io(), _sample_io())
    h[1].u = h[1].counter = None
    refused("hkl_per_sample_group", L.hkl_per_sample_group(h, dev, 2, None), member=1)
    h = (LH.PerSampleIO * 2)(_sample_io(), _sample_io())
    h[1].iw = None  # optional when sampling (checked no further on the host), required for the weights alone
    refused("hkl_per_weights_group", L.hkl_per_weights_group(h, dev, 2, None), member=1)
    h = (LH.PerUpdateIO * 2)(_update_io(), _update_io())
    h[0].td = None
    refused("hkl_per_update_group", L.hkl_per_update_group(h, dev, 2, None), member=0)


def test_population_prioritized_ring_is_gpu_only():
    with pytest.raises(_native.HockeyNativeError):
        PopulationPrioritizedRing(2, 64, device="cpu")
    with pytest.raises(_native.HockeyNativeError):
        PopulationPrioritizedRing(2, 64, prioritized=[True, False], beta=[0.15, 0.6], device="cpu")


def test_population_learner_still_refuses_a_whole_ring_prioritized_ring():
    agents = [TD3(TD3Config(batch_size=32), device="cpu", seed=j) for j in range(2)]
    rings = [PrioritizedRing(64, device="cpu") for _ in range(2)]
    with pytest.raises(ValueError, match="prioritized"):
        PopulationLearner(agents, rings, 32)
