"""The value of a trained TD3 agent outside the learner: Q_k(s, a) of its twin critics and
V(s) = min(Q1, Q2)(s, actor(s)), on whole batches in one call.

    vf = ValueFn(agent)                      # or a checkpoint dict / path, or an (actor, twin_q) pair
    q1, q2 = vf.q(obs, act)                  # [n] each; act in the env's range (TwinQ unscales it)
    v, a = vf.v(obs, return_action=True)     # V(s) and the actor's action it was taken at

``ValueFn`` copies the three networks (actor 18 -> 256 -> 256 -> 4, critics 22 -> 256 -> 256 -> 1; rl/td3/networks.py)
into flat buffers of its own, as ``PolicyBank`` does, so a fused ``Learner`` attached to the agent is not disturbed and
later training does not move the values until ``refresh()``.  The critic's ``action_low`` / ``action_range`` buffers
give the action map.

backend="hip" is ``hkl_value`` (include/hockey_learner.h, csrc/hkl_value.h): one launch, 64 rows per workgroup
through the learner's fp32 MFMA layer routines, the action of V mode kept in registers between the actor and the
critics; asynchronous on torch's current stream, graph-capturable, no host synchronisation, a row's result independent
of the other rows bit for bit.  backend="torch" is the reference path: the same expressions through
``torch.nn.functional.linear`` on the ValueFn's own buffers, on any device.  backend="auto" takes "hip" on a GPU when
the learner library is built and "torch" otherwise.  The two differ by fp32 summation order and the kernels' tanh
(tests/test_gpu_value.py holds the kernel to a float64 forward).
"""
import ctypes

import torch

from . import _native
from .learner_hip import PACK_FLOATS, Net, ValueIO, check, lib, ptr, stream_ptr
from .policy_bank import _hip_ready, resolve_backend

_LAYERS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias")


def _shapes(n_in, n_out):
    return ((256, n_in), (256,), (256, 256), (256,), (n_out, 256), (n_out,))


class _FlatNet:
    """One MLP's weights in one flat fp32 buffer (torch layout, _LAYERS order) and its MFMA operand pack."""

    def __init__(self, n_in, n_out, device):
        self.n_in, self.n_out = n_in, n_out
        self.shapes = _shapes(n_in, n_out)
        sizes = [int(torch.Size(s).numel()) for s in self.shapes]
        assert all(s % 4 == 0 for s in sizes[:-1])  # every tensor starts on 16 bytes (the kernels read float4)
        self.flat = torch.zeros(sum(sizes), dtype=torch.float32, device=device)
        self.p, o = {}, 0
        for name, shape, n in zip(_LAYERS, self.shapes, sizes):
            self.p[name] = self.flat[o:o + n].view(shape)
            o += n
        self.pack = None

    def load(self, sd, what):
        for name, shape in zip(_LAYERS, self.shapes):
            if name not in sd or tuple(sd[name].shape) != shape:
                got = tuple(sd[name].shape) if name in sd else None
                raise ValueError(f"ValueFn: {what} is {self.n_in} -> 256 -> 256 -> {self.n_out}: {name} must be "
                                 f"{shape}, got {got}")
        with torch.no_grad():
            for name in _LAYERS:
                self.p[name].copy_(torch.as_tensor(sd[name]).detach())

    def net(self):
        if self.pack is None:
            self.pack = torch.zeros(PACK_FLOATS, dtype=torch.float32, device=self.flat.device)
        return Net(*[ptr(self.p[k]) for k in _LAYERS], ptr(self.pack), self.n_in, self.n_out)

    def forward(self, x):
        p, lin = self.p, torch.nn.functional.linear
        h = torch.tanh(lin(x, p["fc1.weight"], p["fc1.bias"]))
        h = torch.tanh(lin(h, p["fc2.weight"], p["fc2.bias"]))
        return lin(h, p["fc3.weight"], p["fc3.bias"])


def _state_dicts(source):
    """(actor state dict, critic state dict) of a TD3 agent, a checkpoint dict / path or an (actor, twin_q) pair."""
    if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__"):
        from .td3 import load_checkpoint

        source = load_checkpoint(source)
    if isinstance(source, dict):
        if "policy" not in source or "critic" not in source:
            raise ValueError("ValueFn: a checkpoint needs the keys 'policy' and 'critic'")
        pair = (source["policy"], source["critic"])
    elif isinstance(source, (tuple, list)) and len(source) == 2:
        pair = tuple(source)
    elif hasattr(source, "actor") and hasattr(source, "critic"):
        pair = (source.actor, source.critic)
    else:
        raise ValueError("ValueFn: source must be a TD3 agent, a checkpoint dict or path, or an (actor, twin_q) pair")
    return tuple(m.state_dict() if hasattr(m, "state_dict") else dict(m) for m in pair)


class ValueFn:
    """Q and V of one TD3 agent on batches (module docstring)."""

    def __init__(self, source, device="cuda:0"):
        self.device = torch.device(device)
        self.actor = _FlatNet(18, 4, self.device)
        self.critics = (_FlatNet(22, 1, self.device), _FlatNet(22, 1, self.device))
        self.action_low = torch.zeros(4, dtype=torch.float32, device=self.device)
        self.action_range = torch.zeros(4, dtype=torch.float32, device=self.device)
        self._low = self._range = None  # host copies for the kernel's struct
        self._source = source
        self.refresh()

    def refresh(self, source=None):
        """Copy the weights again (from ``source``, or the source given last) and re-pack them: call after the
        agent trained on or a checkpoint changed."""
        if source is not None:
            self._source = source
        actor, critic = _state_dicts(self._source)
        self.actor.load(actor, "the actor")
        for k, net in enumerate(self.critics):
            pre = f"q{k + 1}."
            net.load({n[len(pre):]: v for n, v in critic.items() if n.startswith(pre)}, f"critic {k + 1}")
        for name, dst in (("action_low", self.action_low), ("action_range", self.action_range)):
            if name not in critic or tuple(critic[name].shape) != (4,):
                raise ValueError(f"ValueFn: the critic's state needs the buffer {name} [4]")
            dst.copy_(torch.as_tensor(critic[name]).detach().float())
        self._low, self._range = self.action_low.cpu().tolist(), self.action_range.cpu().tolist()
        if _hip_ready(self.device):
            nets = (Net * 3)(self.actor.net(), self.critics[0].net(), self.critics[1].net())
            check(lib().hkl_pack(nets, 3, None, stream_ptr(self.device)), "hkl_pack")
        return self

    # ------------------------------------------------------------------ arguments
    def _rows(self, t, name, cols, n=None):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] < cols or t.dtype != torch.float32:
            got = f"{t.dtype} {tuple(t.shape)}" if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"{name} must be float32 [n, >= {cols}], got {got}")
        if t.device != self.device:
            raise ValueError(f"{name} is on {t.device}, the value function on {self.device}")
        if n is not None and t.shape[0] != n:
            raise ValueError(f"{name} must have obs's {n} rows, got {t.shape[0]}")
        if t.stride(1) != 1 or t.stride(0) < cols:
            t = t.contiguous()
        return t

    # ------------------------------------------------------------------ hip
    def _hip(self, obs, act, q1=False, q2=False, qmin=False, act_out=False):
        """One hkl_value call; returns the requested outputs (None for the others) as (q1, q2, qmin, act_out)."""
        if self.device.type != "cuda":
            raise _native.HockeyNativeError("ValueFn backend='hip' runs on the GPU only")
        if self.actor.pack is None:
            raise _native.HockeyNativeError("ValueFn backend='hip': the learner library was not built when the "
                                            "weights were packed")
        n = obs.shape[0]
        new = lambda want, *shape: torch.empty(shape, dtype=torch.float32, device=self.device) if want else None  # noqa: E731
        out = (new(q1, n), new(q2, n), new(qmin, n), new(act_out, n, 4))
        if n == 0:  # nothing to launch (an empty tensor has no storage to point at)
            return out
        io = ValueIO()
        io.n_rows = n
        io.actor, io.q[0], io.q[1] = self.actor.net(), self.critics[0].net(), self.critics[1].net()
        io.obs, io.obs_ld = obs.data_ptr(), obs.stride(0)
        if act is not None:
            io.act, io.act_ld = act.data_ptr(), act.stride(0)
        for c in range(4):
            io.act_low[c], io.act_range[c] = self._low[c], self._range[c]
        io.q1, io.q2, io.qmin, io.act_out = (None if t is None else t.data_ptr() for t in out)
        io.act_out_ld = 4
        check(lib().hkl_value(ctypes.byref(io), stream_ptr(self.device)), "hkl_value")
        return out

    # ------------------------------------------------------------------ torch (the reference path)
    def _q_torch(self, obs, act):
        a = ((act[:, :4] - self.action_low) / self.action_range) * 2 - 1.0  # TwinQNetwork._unscale_action
        x = torch.cat([obs[:, :18], a], dim=-1)
        return tuple(c.forward(x).squeeze(-1) for c in self.critics)

    def _act_torch(self, obs):
        return torch.tanh(self.actor.forward(obs[:, :18]))

    # ------------------------------------------------------------------ values
    @torch.no_grad()
    def q(self, obs, act, backend="auto"):
        """(q1, q2), [n] each: both critics on ``obs`` ([n, >= 18] float32, the first 18 columns are the
        observation) and ``act`` ([n, >= 4] float32, the first 4 columns an action in the env's range).  Both need
        unit column stride; their row strides are passed on (views such as ``act8[:, :4]`` are read in place)."""
        backend = resolve_backend(backend, self.device)
        obs = self._rows(obs, "obs", 18)
        act = self._rows(act, "act", 4, obs.shape[0])
        if backend == "torch":
            return self._q_torch(obs, act)
        return self._hip(obs, act, q1=True, q2=True)[:2]

    @torch.no_grad()
    def qmin(self, obs, act, backend="auto"):
        """min(q1, q2) of ``q`` [n]."""
        backend = resolve_backend(backend, self.device)
        obs = self._rows(obs, "obs", 18)
        act = self._rows(act, "act", 4, obs.shape[0])
        if backend == "torch":
            return torch.minimum(*self._q_torch(obs, act))
        return self._hip(obs, act, qmin=True)[2]

    @torch.no_grad()
    def v(self, obs, backend="auto", return_action=False):
        """V(s) = min(Q1, Q2)(s, actor(s)) [n]; with return_action also the actor's action [n, 4]."""
        backend = resolve_backend(backend, self.device)
        obs = self._rows(obs, "obs", 18)
        if backend == "torch":
            a = self._act_torch(obs)
            v = torch.minimum(*self._q_torch(obs, a))
        else:
            _, _, v, a = self._hip(obs, None, qmin=True, act_out=return_action)
        return (v, a) if return_action else v
