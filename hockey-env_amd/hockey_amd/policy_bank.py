"""A bank of actors (18 -> 256 -> 256 -> 4, tanh; rl/td3/networks.py ActorNetwork) that act side by side.

``PolicyBank(capacity, device)`` keeps up to ``capacity`` (at most 64; with ``wide=True`` at most 4 096) actors' weights in one strided device buffer
and runs, in ONE call, a different actor on every row of a batch: ``act(obs, policy)`` gives row i the actions of
slot ``policy[i]`` and leaves rows with ``policy[i] = -1`` alone.  This is what per-arena self-play
(``hockey_amd.opponents.OpponentMix(sampling="arena")``: every arena draws its own pool snapshot at every step, as
the reference's single env does) and cross-play (``hockey_amd.evaluate.tournament``) need; with one masked PyTorch
forward per slot either costs K forwards over the whole batch per step.

backend="hip" is ``hkl_act`` for capacities up to 64 and ``hkl_act_wide`` above (include/hockey_learner.h,
csrc/hkl_act.h; the two run one acting body, so a row's actions are the same bits): the rows are grouped by policy on the
device and every workgroup runs 64 rows of one policy through the learner's fp32 MFMA layer routines; asynchronous
on torch's current stream, graph-capturable, no host synchronisation.  A row's result does not depend on the other
rows (bit for bit).  backend="torch" is the reference path: one masked eager forward per occupied slot, writing the
same rows and columns; it works on any device.  backend="auto" takes "hip" on a GPU when the learner library is
built and "torch" otherwise.  The two differ by fp32 summation order and the kernels' tanh
(tests/test_gpu_policy_bank.py holds the kernel to a float64 forward).
"""
import ctypes

import torch

from . import _native
from .learner_hip import (ACT_MAX_POLICIES, ACT_PARAM_FLOATS, ACT_WIDE_MAX_POLICIES, GROUP_MAX, PACK_FLOATS, ActIO,
                          ActWideIO, Net, PackIO, act_wide_max_tiles, check, lib, stream_ptr, upload)

# floats of fc1.weight, fc1.bias, fc2.weight, fc2.bias, fc3.weight, fc3.bias inside a slot (torch layout, this order)
_SHAPES = (("fc1.weight", (256, 18)), ("fc1.bias", (256,)), ("fc2.weight", (256, 256)), ("fc2.bias", (256,)),
           ("fc3.weight", (4, 256)), ("fc3.bias", (4,)))


def _offsets():
    out, o = {}, 0
    for name, shape in _SHAPES:
        n = 1
        for d in shape:
            n *= d
        out[name] = (o, n, shape)
        o += n
    assert o == ACT_PARAM_FLOATS
    return out


_OFF = _offsets()


def _hip_ready(device):
    from .td3 import fused_available

    return device.type == "cuda" and fused_available()


def resolve_backend(backend, device):
    """``backend`` checked, with "auto" turned into "hip" on a GPU when the learner library is built, else "torch"."""
    if backend not in ("auto", "hip", "torch"):
        raise ValueError("backend must be 'auto', 'hip' or 'torch'")
    if backend == "auto":
        backend = "hip" if _hip_ready(device) else "torch"
    return backend


class PolicyBank:
    """Up to ``capacity`` actors acting side by side (module docstring)."""

    def __init__(self, capacity, device="cuda:0", wide=False):
        """wide: allow more than ``hkl_act``'s 64 slots, up to 4 096 (``hkl_act_wide`` under backend="hip").  Without it
        the limit stays 64, as callers written against ``hkl_act`` expect."""
        self.capacity = int(capacity)
        limit = ACT_WIDE_MAX_POLICIES if wide else ACT_MAX_POLICIES
        if not 1 <= self.capacity <= limit:
            raise ValueError(f"PolicyBank capacity must be in [1, {limit}], got {capacity}"
                             + ("" if wide else f" (wide=True allows up to {ACT_WIDE_MAX_POLICIES})"))
        self.device = torch.device(device)
        self.params = torch.zeros((self.capacity, ACT_PARAM_FLOATS), dtype=torch.float32, device=self.device)
        self.occupied = [False] * self.capacity
        self._packs = None  # [capacity][PACK_FLOATS], allocated with the first slot packed for the hip backend
        self._scratch = {}  # n_rows -> (order, counts, offsets), and tiles for a wide bank

    # ------------------------------------------------------------------ slots
    def __len__(self):
        return sum(self.occupied)

    def slots(self):
        return [k for k, o in enumerate(self.occupied) if o]

    def add(self, actor):
        """Copy ``actor`` into the first free slot; returns the slot."""
        for k, o in enumerate(self.occupied):
            if not o:
                return self.replace(k, actor)
        raise RuntimeError(f"PolicyBank is full ({self.capacity} slots)")

    def replace(self, slot, actor):
        """Copy ``actor`` (a module with fc1 / fc2 / fc3, or its state dict) into ``slot`` and refresh the slot's
        MFMA operand pack; returns the slot."""
        return self.replace_many([slot], [actor])[0]

    def replace_many(self, slots, actors):
        """``replace`` for several slots at once: actor i goes to ``slots[i]`` and their operand packs are refreshed
        together -- one ``hkl_pack`` call for up to the 4 networks it takes, one ``hkl_pack_group`` launch per 64
        slots above that -- so a population-wide snapshot (at most 64 members) is one launch, not one per slot.
        Returns the slots."""
        slots = [self._slot(k) for k in slots]
        actors = list(actors)
        if len(slots) != len(actors):
            raise ValueError("replace_many takes one actor per slot")
        if len(set(slots)) != len(slots):
            raise ValueError("replace_many: a slot is named twice")
        sds = []
        for actor in actors:
            sd = actor.state_dict() if hasattr(actor, "state_dict") else dict(actor)
            for name, (_, _, shape) in _OFF.items():
                if name not in sd or tuple(sd[name].shape) != shape:
                    got = tuple(sd[name].shape) if name in sd else None
                    raise ValueError(f"PolicyBank holds actors 18 -> 256 -> 256 -> 4: {name} must be {shape}, "
                                     f"got {got}")
            sds.append(sd)
        with torch.no_grad():
            for slot, sd in zip(slots, sds):
                row = self.params[slot]
                for name, (o, n, _) in _OFF.items():
                    row[o:o + n].copy_(sd[name].detach().reshape(-1))
                self.occupied[slot] = True
        if slots and _hip_ready(self.device):
            self._pack(slots)
        return slots

    def free(self, slot):
        self.occupied[self._slot(slot)] = False

    def _slot(self, slot):
        slot = int(slot)
        if not 0 <= slot < self.capacity:
            raise IndexError(f"PolicyBank slot {slot} outside [0, {self.capacity})")
        return slot

    def state_dict(self, slot):
        """The slot's weights as an Actor state dict (views of the bank's buffer)."""
        row = self.params[self._slot(slot)]
        return {name: row[o:o + n].view(shape) for name, (o, n, shape) in _OFF.items()}

    # ------------------------------------------------------------------ hip
    def _pack(self, slots):
        """Refresh the operand packs of ``slots``: one ``hkl_pack`` for up to its 4 networks, else one
        ``hkl_pack_group`` launch per 64 slots (one network per member of the group, no step counter)."""
        if self._packs is None:
            self._packs = torch.zeros((self.capacity, PACK_FLOATS), dtype=torch.float32, device=self.device)
        base, pbase = self.params.data_ptr(), self._packs.data_ptr()
        nets = []
        for slot in slots:
            b = base + 4 * ACT_PARAM_FLOATS * slot
            p = [ctypes.c_void_p(b + 4 * _OFF[name][0]) for name, _ in _SHAPES]
            nets.append(Net(p[0], p[1], p[2], p[3], p[4], p[5], ctypes.c_void_p(pbase + 4 * PACK_FLOATS * slot), 18, 4))
        if len(nets) <= 4:
            check(lib().hkl_pack((Net * len(nets))(*nets), len(nets), None, stream_ptr(self.device)), "hkl_pack")
            return
        for lo in range(0, len(nets), GROUP_MAX):
            chunk = nets[lo:lo + GROUP_MAX]
            ios = (PackIO * len(chunk))()
            for io, net in zip(ios, chunk):
                io.net[0] = net
            dev = upload(ios, self.device)
            check(lib().hkl_pack_group(ios, ctypes.c_void_p(dev.data_ptr()), 1, len(chunk), stream_ptr(self.device)),
                  "hkl_pack_group")

    def _act_hip(self, obs, policy, out, out_col, base_slot=0):
        L = lib()
        if self.device.type != "cuda":
            raise _native.HockeyNativeError("PolicyBank backend='hip' runs on the GPU only")
        if self._packs is None:
            raise _native.HockeyNativeError("PolicyBank backend='hip': no slot has been packed")
        n = obs.shape[0]
        wide = policy is not None and self.capacity > ACT_MAX_POLICIES  # hkl_act's own range stays on hkl_act
        if wide and n == 0:  # an empty tensor has no address to hand to the call, and there is nothing to write
            return
        io = ActWideIO() if wide else ActIO()
        io.n_rows = n
        io.params = self.params[base_slot].data_ptr()
        io.packs = self._packs[base_slot].data_ptr()
        io.obs, io.obs_ld = obs.data_ptr(), obs.stride(0)
        io.out, io.out_ld, io.out_col = out.data_ptr(), out.stride(0), out_col
        if policy is None:
            io.n_policies = 1
        else:
            io.n_policies = self.capacity
            sc = self._scratch.get(n)
            if sc is None:
                z = lambda m: torch.zeros(m, dtype=torch.int32, device=self.device)  # noqa: E731
                if wide:
                    K = self.capacity
                    sc = (z(max(n, 1)), z(K + 1), z(K + 1), z(3 * max(act_wide_max_tiles(n, K), 1)))
                else:
                    sc = (z(max(n, 1)), z(ACT_MAX_POLICIES + 1), z(ACT_MAX_POLICIES + 1))
                self._scratch[n] = sc
            io.policy = policy.data_ptr()
            if wide:
                io.order, io.counts, io.offsets, io.tiles = (t.data_ptr() for t in sc)
            else:
                io.order, io.counts, io.offsets = (t.data_ptr() for t in sc)
        if wide:
            check(L.hkl_act_wide(ctypes.byref(io), stream_ptr(self.device)), "hkl_act_wide")
        else:
            check(L.hkl_act(ctypes.byref(io), stream_ptr(self.device)), "hkl_act")

    # ------------------------------------------------------------------ torch (the reference path)
    def _forward_torch(self, slot, x):
        p = self.state_dict(slot)
        lin = torch.nn.functional.linear
        h = torch.tanh(lin(x, p["fc1.weight"], p["fc1.bias"]))
        h = torch.tanh(lin(h, p["fc2.weight"], p["fc2.bias"]))
        return torch.tanh(lin(h, p["fc3.weight"], p["fc3.bias"]))

    def _act_torch(self, obs, policy, out, out_col, base_slot=0):
        x = obs[:, :18]
        dst = out[:, out_col:out_col + 4]
        if policy is None:
            dst.copy_(self._forward_torch(base_slot, x))
            return
        for k in self.slots():  # one masked forward over every row per occupied slot
            dst.copy_(torch.where((policy == k).unsqueeze(1), self._forward_torch(k, x), dst))

    # ------------------------------------------------------------------ acting
    @torch.no_grad()
    def act(self, obs, policy=None, out=None, out_col=0, backend="auto", _base_slot=0):
        """Actions of a batch: row i of ``obs`` ([n, >= 18] float32, the first 18 columns are the observation) runs
        slot ``policy[i]`` ([n] int32 in [-1, capacity); -1: the row does not act); its four actions go to
        ``out[i, out_col : out_col + 4]``.  Rows at -1 and every other column of ``out`` keep what they held.
        policy=None: every row runs slot 0 (the single-actor case, nothing is grouped).  out=None: a new zero
        [n, out_col + 4] tensor.  Rows whose policy names a free slot are undefined under "hip" (the slot's last
        weights) and untouched under "torch".  Returns ``out``."""
        backend = resolve_backend(backend, self.device)
        if obs.dim() != 2 or obs.shape[1] < 18 or obs.dtype != torch.float32:
            raise ValueError(f"obs must be float32 [n, >= 18], got {obs.dtype} {tuple(obs.shape)}")
        if obs.device != self.device:
            raise ValueError(f"obs is on {obs.device}, the bank on {self.device}")
        n, out_col = obs.shape[0], int(out_col)
        if obs.stride(1) != 1 or obs.stride(0) < 18:
            obs = obs.contiguous()
        if out is None:
            out = torch.zeros((n, out_col + 4), dtype=torch.float32, device=self.device)
        if (out.dim() != 2 or out.shape[0] != n or out.dtype != torch.float32 or out.device != self.device or
                out_col < 0 or out.shape[1] < out_col + 4 or (out.shape[1] > 1 and out.stride(1) != 1)
                or out.stride(0) < out.shape[1]):
            raise ValueError(f"out must be a float32 [n, >= out_col + 4] tensor with unit column stride on "
                             f"{self.device}, got {out.dtype} {tuple(out.shape)}")
        if policy is not None:
            if policy.shape != (n,) or policy.dtype != torch.int32 or policy.device != self.device:
                raise ValueError(f"policy must be int32 [n] on {self.device}, got {policy.dtype} {tuple(policy.shape)}")
            policy = policy.contiguous()
        elif not self.occupied[_base_slot]:
            raise ValueError(f"PolicyBank slot {_base_slot} is free")
        (self._act_hip if backend == "hip" else self._act_torch)(obs, policy, out, out_col, _base_slot)
        return out

    @torch.no_grad()
    def explore(self, explorer, obs, out=None, out_col=0, count=None, ext=None):
        """``act`` with exploration (hockey_amd.explore): row i runs slot ``explorer.policy[i]`` (slot 0 for a policy of
        None) and ``explorer``'s law turns its action into the one to play, written to ``out[i, out_col : out_col +
        4]``.  Under the explorer's backend "hip" this is ONE ``hkl_explore`` call (banks of up to 64 slots);
        under "torch" the bank's torch forward followed by the law in numpy.  Returns ``out``."""
        n, out_col, policy = explorer.N, int(out_col), explorer.policy
        if obs.dim() != 2 or obs.shape != (n, obs.shape[1]) or obs.shape[1] < 18 or obs.dtype != torch.float32:
            raise ValueError(f"obs must be float32 [{n}, >= 18], got {obs.dtype} {tuple(obs.shape)}")
        if obs.device != self.device:
            raise ValueError(f"obs is on {obs.device}, the bank on {self.device}")
        if obs.stride(1) != 1 or obs.stride(0) < 18:
            obs = obs.contiguous()
        if out is None:
            out = torch.zeros((n, out_col + 4), dtype=torch.float32, device=self.device)
        if (out.dim() != 2 or out.shape[0] != n or out.dtype != torch.float32 or out.device != self.device or
                out_col < 0 or out.shape[1] < out_col + 4 or (out.shape[1] > 1 and out.stride(1) != 1)
                or out.stride(0) < out.shape[1]):
            raise ValueError(f"out must be a float32 [n, >= out_col + 4] tensor with unit column stride on "
                             f"{self.device}, got {out.dtype} {tuple(out.shape)}")
        if policy is None and not self.occupied[0]:
            raise ValueError("PolicyBank slot 0 is free")
        if explorer.backend == "torch":
            a = torch.zeros((n, 4), dtype=torch.float32, device=self.device)
            self._act_torch(obs, policy, a, 0)
            acting = None
            if policy is not None:
                occ = torch.tensor(self.occupied, device=self.device)
                inside = (policy >= 0) & (policy < self.capacity)
                acting = inside & occ[policy.clamp(0, self.capacity - 1).long()]
            explorer._run_torch(a, acting, out, out_col, count, ext)
            return out
        if self.capacity > ACT_MAX_POLICIES:
            raise _native.HockeyNativeError(f"hkl_explore takes banks of up to {ACT_MAX_POLICIES} slots")
        if self.device.type != "cuda" or self._packs is None:
            raise _native.HockeyNativeError("PolicyBank.explore backend='hip' needs a GPU and a packed slot")
        io = ActIO()
        io.n_rows = n
        io.params, io.packs = self.params.data_ptr(), self._packs.data_ptr()
        io.obs, io.obs_ld = obs.data_ptr(), obs.stride(0)
        io.out, io.out_ld, io.out_col = out.data_ptr(), out.stride(0), out_col
        io.n_policies = 1
        if policy is not None:
            io.n_policies = self.capacity
            sc = self._scratch.get(n)
            if sc is None:
                sc = self._scratch[n] = tuple(torch.zeros(m, dtype=torch.int32, device=self.device)
                                              for m in (n, ACT_MAX_POLICIES + 1, ACT_MAX_POLICIES + 1))
            io.policy = policy.data_ptr()
            io.order, io.counts, io.offsets = (t.data_ptr() for t in sc)
        self._explore_obs = obs  # a contiguous copy stays alive until the next call
        explorer._run_hip(io, count, ext)
        return out

    def policy_fn(self, slot, backend="auto"):
        """``obs [n, 18] -> actions [n, 4]`` of one slot (``hockey_amd.evaluate.evaluate(policy=...)``)."""
        slot = self._slot(slot)
        return lambda obs: self.act(obs.float(), backend=backend, _base_slot=slot)
