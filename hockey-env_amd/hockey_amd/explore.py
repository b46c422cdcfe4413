"""Exploration acting on the device: ``TD3.act`` for S members side by side in ONE ``hkl_explore`` call per step.

``TD3.act`` (rl/td3/agent.py get_action) is an actor forward followed by a dozen small launches and host arithmetic:
the annealed noise scale of the agent's ``total_steps``, a noise draw, multiply / add / clamp, the random-phase mask
while ``total_steps < start_steps`` and its uniform actions.  All of it is a function of the observation row, two
counters per member and a counter-based random draw, so ``hkl_explore`` (include/hockey_explore.h,
csrc/hkl_explore.h) runs it as the epilogue of ``hkl_act``'s acting kernel and writes the step kernel's action
columns directly.  The counters live on the device and advance there; nothing is uploaded or read back per step.

The law, for member m owning rows [m n, (m + 1) n) and row i with local(i) = i - m n (every symbol as in the header)::

    T0 = total[m]; T1 = T0 + count[m]
    all_random = T1 < start_steps;  random(i) = all_random or T0 + 1 + local(i) < start_steps
    s_m = float32(TD3.noise_scale() at total_steps = T1)                 (float64 arithmetic, one rounding)
    out[i] = 2 u - 1 if random(i) else clamp(a + unit * s_m, -1, 1)      (float32, each operation rounded)

Draws are Philox4x32-10 blocks keyed by ``seed_m ^ purpose`` at counter (local(i), calls[m]): member j's draws are the
same bits in a population of 64 and in a run of its own, whatever its position -- the acting side of the learner's
composition independence (hockey_amd.population).  ``unit`` is N(0, 1) (gaussian), U(-sqrt 3, sqrt 3) (uniform), an
Ornstein-Uhlenbeck state of sigma 1 kept per row on the device, or the caller's / the Explorer's own pink blocks
("external": the kernel reads a strided view of ``noise.pink_block``'s [N, 4, seq_len] at the block index).

Batched differences from ``TD3.act`` / ``hockey_amd.noise``: the draws come from Philox, not
from torch's generator; the scale multiplies a unit-scale draw as one float32 product (the reference multiplies a
sigma-scaled draw by current / initial); the pink index advances on EVERY call, also while the member is wholly in the
random phase (``TD3.act`` does not call the generator then), and one fresh block per member is drawn from a generator
seeded by the member, not by the population.

backend="hip" is the kernel; backend="torch" evaluates the same law without the library, through numpy and the
bank's torch forward, on any device: slow, and the executable specification the GPU tests hold the kernel to.  The two
agree bit for bit in everything but the actor's output and the Box-Muller normals (libm against the device's).
"""
import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from .noise import pink_block
from .philox_ref import U64, draw_words, normals, philox4x32_10, uniform_pm1  # noqa: F401 (philox4x32_10: re-exported)
from .policy_bank import resolve_backend

KEY_NOISE = 0x6578706C6F7265  # HKL_EXPLORE_KEY_NOISE ("explore")
KEY_RANDOM = 0x72616E646F6D  # HKL_EXPLORE_KEY_RANDOM ("random")
ANNEAL = {"none": 0, "linear": 1, "exp": 2}
NOISE = {"none": 0, "gaussian": 1, "uniform": 2, "ornstein-uhlenbeck": 3, "external": 4, "pink": 4}
_NONE, _GAUSS, _UNIFORM, _OU, _EXT = range(5)
GROUP_MAX = 64  # HKL_GROUP_MAX
SQRT3 = np.float32(math.sqrt(3.0))


@dataclass
class Member:
    """One member's exploration parameters (hkl_explore_member).  noise: "none", "gaussian", "uniform",
    "ornstein-uhlenbeck", "pink" (blocks of ``seq_len`` steps drawn by the Explorer) or "external" (the caller passes
    ``ext`` to every ``explore``).  max_total_steps 0: no schedule, the scale stays ``init_scale``."""
    seed: int = 0
    start_steps: int = 0
    max_total_steps: int = 0
    init_scale: float = 0.2
    min_scale: float = 0.0
    anneal: str = "none"
    noise: str = "gaussian"
    theta: float = 0.15
    dt: float = 1.0
    seq_len: int = 500

    @classmethod
    def from_config(cls, cfg, seed, max_total_steps=None):
        """The member ``TD3(cfg, seed=seed, max_total_steps=...)`` explores as."""
        return cls(seed=int(seed), start_steps=int(cfg.start_steps), max_total_steps=int(max_total_steps or 0),
                   init_scale=float(cfg.action_noise_scale), min_scale=float(cfg.noise_min_scale),
                   anneal=cfg.noise_anneal_mode if cfg.use_noise_annealing else "none", noise=cfg.noise_mode,
                   seq_len=int(cfg.max_steps))

    @classmethod
    def from_agent(cls, agent):
        return cls.from_config(agent.cfg, agent.seed, agent.max_total_steps)

    def check(self):
        if self.anneal not in ANNEAL:
            raise ValueError(f"Unknown anneal mode: {self.anneal}")
        if self.noise not in NOISE:
            raise ValueError(f"Unknown noise mode: {self.noise}")
        if self.noise == "pink" and self.seq_len < 1:
            raise ValueError("a pink member needs seq_len >= 1")
        return self


# ---------------------------------------------------------------------------------------------------- the law in numpy
def noise_scale(mem, t1):
    """float32(TD3.noise_scale()) at total_steps = t1 for ``mem``."""
    s = float(mem.init_scale)
    if mem.anneal != "none" and mem.max_total_steps > 0:
        progress = min(int(t1) / int(mem.max_total_steps), 1.0)
        s = s * (1 - progress) if mem.anneal == "linear" else s * (0.1 ** progress)
        s = max(s, float(mem.min_scale))
    return np.float32(s)


def law(members, n, total, calls, count, a, x=None, ext=None, z=None):
    """One ``hkl_explore`` call in numpy.  members: S ``Member``s; total, calls [S] int64 and count [S] int32: the state
    before the call; a [S n, 4] float32: the actor's actions; x [S n, 4] float32: the OU state; ext [S n, 4] float32:
    the external members' unit noise; z (optional) [S n, 4] float32: normals to use in place of this module's float32
    Box-Muller (the kernel's ``z_out``).  Returns a dict: "out", "x", "z" (the raw draws, as ``z_out``), "scale" [S],
    "random" [S n] bool, "total", "calls" (the state after the call)."""
    S, n = len(members), int(n)
    a = np.asarray(a, np.float32)
    out = np.empty((S * n, 4), np.float32)
    x_new = np.zeros((S * n, 4), np.float32) if x is None else np.array(x, np.float32)
    raw = np.zeros((S * n, 4), np.float32)
    scale = np.zeros(S, np.float32)
    rnd = np.zeros(S * n, bool)
    total, calls = np.array(total, np.int64), np.array(calls, np.int64)
    f32 = np.float32
    for m, mem in enumerate(members):
        rows = slice(m * n, (m + 1) * n)
        t0 = max(int(total[m]), 0)
        t1 = t0 + min(max(int(count[m]), 0), n)
        all_random = t1 < mem.start_steps
        rnd[rows] = all_random | (t0 + 1 + np.arange(n, dtype=np.int64) < mem.start_steps)
        s = scale[m] = noise_scale(mem, t1)
        kind = NOISE[mem.noise]
        if not all_random:
            unit = np.zeros((n, 4), f32)
            if kind in (_GAUSS, _UNIFORM, _OU):
                w = draw_words(mem.seed, KEY_NOISE, n, calls[m])
                if kind == _UNIFORM:
                    raw[rows] = uniform_pm1(w)
                    unit = raw[rows] * SQRT3
                else:
                    raw[rows] = normals(w) if z is None else np.asarray(z, f32)[rows]
                    unit = raw[rows]
                    if kind == _OU:
                        xm = x_new[rows]
                        unit = (xm + (f32(mem.theta) * -xm) * f32(mem.dt)) + f32(math.sqrt(mem.dt)) * raw[rows]
                        x_new[rows] = unit
            elif kind == _EXT:
                unit = np.asarray(ext, f32)[rows]
            v = a[rows] + unit * s
            out[rows] = np.where(v < f32(-1), f32(-1), np.where(v > f32(1), f32(1), v))  # NaN stays NaN
        if rnd[rows].any():
            u = uniform_pm1(draw_words(mem.seed, KEY_RANDOM, n, calls[m]))
            out[rows] = np.where(rnd[rows, None], u, out[rows]) if not all_random else u
        total[m] = t1
        calls[m] += 1
    return {"out": out, "x": x_new, "z": raw, "scale": scale, "random": rnd, "total": total, "calls": calls}


# ---------------------------------------------------------------------------------------------------- Explorer
class Explorer:
    """The exploration state of S = len(members) members of ``rows_per_member`` rows each, acting through ``bank``.

    ``explore(obs, out, out_col, count)`` is one ``hkl_explore`` call (backend "hip") or the same law in numpy
    (backend "torch"); "auto" takes "hip" on a GPU when the learner library is built.  policy: "member" (default)
    runs row i on bank slot i // rows_per_member (slot 0 without grouping when S == 1), or an int32 [N] tensor.
    The state -- ``total`` / ``calls`` [S] int64, the OU state ``x`` [N, 4], the pink blocks -- lives on ``device``;
    ``scale`` [S] receives the float32 scale of the last call and, with keep_draws, ``z`` [N, 4] its raw draws."""

    count_on_device = True  # a collector hands ``explore`` the running arenas as int32 [S] on the device

    def __init__(self, bank, members, rows_per_member, device=None, backend="auto", policy="member",
                 keep_draws=False):
        self.bank = bank
        self.members = [m.check() for m in members]
        S, n = len(self.members), int(rows_per_member)
        if not 1 <= S <= GROUP_MAX:
            raise ValueError(f"an Explorer has 1 to {GROUP_MAX} members, got {S}")
        if n < 1:
            raise ValueError("rows_per_member must be positive")
        self.S, self.n, self.N = S, n, S * n
        dev = self.device = torch.device(bank.device if device is None else device)
        if dev != bank.device:
            raise ValueError(f"the Explorer is on {dev}, its bank on {bank.device}")
        self.backend = resolve_backend(backend, dev)
        if isinstance(policy, str):
            if policy != "member":
                raise ValueError("policy must be 'member' or an int32 tensor")
            policy = None if S == 1 else (torch.arange(self.N, device=dev) // n).to(torch.int32)
        elif policy.shape != (self.N,) or policy.dtype != torch.int32 or policy.device != dev:
            raise ValueError(f"policy must be int32 [{self.N}] on {dev}")
        self.policy = policy
        self.total = torch.zeros(S, dtype=torch.int64, device=dev)
        self.calls = torch.zeros(S, dtype=torch.int64, device=dev)
        self.full = torch.full((S,), n, dtype=torch.int32, device=dev)
        self.x = torch.zeros((self.N, 4), dtype=torch.float32, device=dev)
        self.scale = torch.zeros(S, dtype=torch.float32, device=dev)
        self.z = torch.zeros((self.N, 4), dtype=torch.float32, device=dev) if keep_draws else None
        self._pink = [j for j, m in enumerate(self.members) if m.noise == "pink"]
        self._needs_ext = any(m.noise == "external" for m in self.members)
        if self._pink and self._needs_ext:
            raise ValueError("pink and external members share the kernel's one ext view: not in one Explorer")
        self.seq_len = max((self.members[j].seq_len for j in self._pink), default=0)
        if any(self.members[j].seq_len != self.seq_len for j in self._pink):
            raise ValueError("the pink members of an Explorer share seq_len")
        self.block, self.t = None, 0
        self._gens = {j: torch.Generator(device=dev) for j in self._pink}
        for j, g in self._gens.items():
            g.manual_seed((self.members[j].seed + 0xA0) & (2 ** 63 - 1))
        self._host = self._dev = self._io = None
        if self.backend == "hip":
            from . import learner_hip as LH

            self._host = (LH.ExploreMember * S)()
            for h, m in zip(self._host, self.members):
                h.seed, h.start_steps, h.max_total_steps = m.seed & U64, m.start_steps, m.max_total_steps
                h.init_scale, h.min_scale, h.anneal, h.noise = m.init_scale, m.min_scale, ANNEAL[m.anneal], NOISE[m.noise]
                h.theta, h.dt, h.sqrt_dt = m.theta, m.dt, math.sqrt(m.dt)
            self._dev = LH.upload(self._host, dev)
        self._new_blocks()

    # ------------------------------------------------------------------ noise state
    def _new_blocks(self):
        if not self._pink:
            return
        if self.block is None:
            self.block = torch.zeros((self.N, 4, self.seq_len), dtype=torch.float32, device=self.device)
        for j in self._pink:
            self.block[j * self.n:(j + 1) * self.n] = pink_block(self.n, 4, self.seq_len, self.device,
                                                                 self._gens[j]).float()
        self.t = 0

    def reset_noise(self):
        """``agent.reset()`` at an episode start for every member: OU state back to 0, fresh pink blocks (each member's
        from its own generator, seeded by the member)."""
        self.x.zero_()
        self._new_blocks()

    def total_steps(self):
        """The members' ``total_steps`` as a list of ints: the one read-back, for the end of a round."""
        return self.total.cpu().tolist()

    def sync(self, agents):
        """At a round's end: every agent's ``total_steps`` from the device counters (one read-back) and its
        ``current_noise_scale`` as ``TD3.act`` would have left it (updated by every step past the all-random phase)."""
        for ag, t in zip(agents, self.total_steps()):
            ag.total_steps = int(t)
            if ag.total_steps >= ag.cfg.start_steps:
                ag.current_noise_scale = ag.noise_scale()

    def _ext_view(self, ext):
        """(tensor, row stride, column stride) of this call's external unit noise, or None."""
        if self._pink:
            if self.t >= self.seq_len:
                self._new_blocks()
            v = self.block[:, :, self.t]
            self.t += 1
            return v
        if not self._needs_ext:
            return None
        if (ext is None or ext.shape != (self.N, 4) or ext.dtype != torch.float32 or ext.device != self.device):
            raise ValueError(f"an external member needs ext: float32 [{self.N}, 4] on {self.device}")
        return ext

    # ------------------------------------------------------------------ one call
    @torch.no_grad()
    def explore(self, obs, out, out_col=0, count=None, ext=None):
        """Actions with exploration for a batch: row i of ``obs`` ([N, >= 18] float32) -> ``out[i, out_col : out_col +
        4]``.  count: int32 [S] on the device, the members' arenas still running (default: all).  ext: the unit noise
        of "external" members, float32 [N, 4] (any strides).  Advances ``total`` by count and ``calls`` by one, on the
        device.  Returns ``out``."""
        return self.bank.explore(self, obs, out, out_col, count, ext)

    def _count(self, count):
        if count is None:
            return self.full
        if count.shape != (self.S,) or count.dtype != torch.int32 or count.device != self.device:
            raise ValueError(f"count must be int32 [{self.S}] on {self.device}")
        return count.contiguous()

    def _run_hip(self, act_io, count, ext):
        """``hkl_explore`` on the bank's filled hkl_act_io."""
        from . import learner_hip as LH

        io = LH.ExploreIO()
        io.act = act_io
        io.rows_per_member = self.n
        io.members = self._dev.data_ptr()
        cnt = self._count(count)
        io.total, io.calls, io.count = self.total.data_ptr(), self.calls.data_ptr(), cnt.data_ptr()
        io.x = self.x.data_ptr()
        e = self._ext_view(ext)
        if e is not None:
            io.ext, io.ext_ld, io.ext_cs = e.data_ptr(), e.stride(0), e.stride(1)
        io.scale_out = self.scale.data_ptr()
        if self.z is not None:
            io.z_out = self.z.data_ptr()
        self._keep = (cnt, e)  # alive until the next call: the launch is asynchronous
        LH.check(LH.lib().hkl_explore(ctypes.byref(io), self._host, LH.stream_ptr(self.device)), "hkl_explore")

    def _run_torch(self, a, acting, out, out_col, count, ext, z=None):
        """The law on the actor's actions ``a`` [N, 4]; rows with acting False keep everything they held."""
        e = self._ext_view(ext)
        r = law(self.members, self.n, self.total.cpu().numpy(), self.calls.cpu().numpy(),
                self._count(count).cpu().numpy(), a.detach().cpu().numpy(), self.x.cpu().numpy(),
                None if e is None else e.detach().cpu().numpy(), None if z is None else z.detach().cpu().numpy())
        dev = self.device
        new = {k: torch.from_numpy(r[k]).to(dev) for k in ("out", "x", "z", "scale", "total", "calls")}
        dst = out[:, out_col:out_col + 4]
        if acting is None:
            dst.copy_(new["out"])
            self.x.copy_(new["x"])
            if self.z is not None:
                self.z.copy_(new["z"])
        else:
            keep = ~acting[:, None]
            dst.copy_(torch.where(keep, dst, new["out"]))
            self.x.copy_(torch.where(keep, self.x, new["x"]))
            if self.z is not None:
                self.z.copy_(torch.where(keep, self.z, new["z"]))
        self.scale.copy_(new["scale"])
        self.total.copy_(new["total"])
        self.calls.copy_(new["calls"])


sync_agents = Explorer.sync  # sync_agents(explorer, agents)

__all__ = ["Explorer", "Member", "law", "philox4x32_10", "sync_agents", "KEY_NOISE", "KEY_RANDOM"]
