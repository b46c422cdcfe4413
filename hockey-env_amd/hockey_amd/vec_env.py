"""VecHockeyEnv: N independent arenas resident in HBM, stepped by the gfx950 kernel.

This is the batched form of ``HockeyEnv`` (hockey/hockey_env.py:83-779): every call maps one-to-one
onto the reference's per-env call, vectorised over a leading arena axis and kept on the device:

  ========================================  ================================================
  reference (one env, numpy, host)          VecHockeyEnv (N arenas, torch tensors on cuda)
  ========================================  ================================================
  reset(seed=s)            :345              reset_seeded(seeds) (PCG64 draws on the device) / reset(seeds=[...])
                                             (the same on the host) / reset() (device Philox placement)
  step(a[8]) -> obs,r,d,_,info :658          step(actions[N,8]) -> obs[N,18], r[N], d[N], info
  obs_agent_two()          :500              obs_agent_two()  (or step(..., with_agent_two=True))
  get_info_agent_two()/get_reward_agent_two  returned by step(..., with_agent_two=True)
  set_state(s[18])         :594              set_state(state[N,18] raw, aux[N,5])
  (none: set_state leaves contacts alone)    snapshot(indices) / restore(snap) / fork(src, dst, source): exact
  render("rgb_array")      :697              render(indices) -> uint8 [m,480,600,3] (any size, or palette indices)
  BasicOpponent.act        :787              policy=('external'|'random'|'weak'|'strong') per player
  ========================================  ================================================

Torch is plumbing only (device memory + the current HIP stream); the compute is libhockey_hip.so.
"""
import ctypes

import numpy as np
import torch

from . import _native as N

from .constants import Mode, parse_mode
from .placement import np_random, placement

_host_placement = placement  # reset() has a keyword of the same name

# torch's private accessor for the current raw stream (no Stream object per call); the public form is the fallback,
# and tests/test_gpu_facade.py holds the two equal inside and outside a torch.cuda.stream context
_getraw = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _raw_stream(index):
    """torch's current stream on device ``index`` as an integer hipStream_t."""
    if _getraw is not None:
        return _getraw(index)
    return torch.cuda.current_stream(index).cuda_stream


_POLICIES = {"external": N.POLICY_EXTERNAL, "random": N.POLICY_RANDOM, "weak": N.POLICY_BASIC_WEAK,
             "strong": N.POLICY_BASIC_STRONG}


def _policy_id(p):
    if isinstance(p, int):
        return p
    return _POLICIES[p]


class StepResult:
    __slots__ = ("obs", "reward", "done", "info", "obs2", "reward2", "info2", "actions", "final_obs", "record")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


class VecHockeyEnv:
    """Batched hockey arenas on one MI355X (one context per device and stream)."""

    def __init__(self, n_arenas, keep_mode=True, mode=Mode.NORMAL, device=None, policies=("external", "external"),
                 auto_reset=False, seed=0, vel_ref_semantics=False, arena_offset=0, diag_flags=0):
        if not torch.cuda.is_available():
            raise N.HockeyNativeError("VecHockeyEnv needs a ROCm GPU (gfx950); the hot path has no CPU fallback")
        self.L = N.lib()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.n = int(n_arenas)
        self.keep_mode = bool(keep_mode)
        self.mode = parse_mode(mode)
        self.auto_reset = bool(auto_reset)
        self.vel_ref_semantics = bool(vel_ref_semantics)
        cfg = N.Config()
        cfg.keep_mode = int(self.keep_mode)
        cfg.mode = self.mode.value
        cfg.auto_reset = int(self.auto_reset)
        cfg.vel_ref_semantics = int(bool(vel_ref_semantics))
        cfg.policy[0] = _policy_id(policies[0])
        cfg.policy[1] = _policy_id(policies[1])
        cfg.seed = int(seed) & ((1 << 64) - 1)
        cfg.arena_offset = int(arena_offset)
        cfg.diag_flags = int(diag_flags)
        self.arena_offset = int(arena_offset)
        self.policies = [cfg.policy[0], cfg.policy[1]]
        ctx = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self.L.hk_create(self.device.index, self.n, ctypes.byref(cfg), ctypes.byref(ctx)), "hk_create")
        self._ctx = ctx
        self.one_starts = np.ones(self.n, bool)  # HockeyEnv.__init__ resets with one_starting=True
        self._alloc()

    # ------------------------------------------------------------------ buffers
    def _alloc(self):
        d, n = self.device, self.n
        self.obs_buf = torch.zeros((n, N.OBS_DIM), dtype=torch.float32, device=d)
        self.obs2_buf = torch.zeros((n, N.OBS_DIM), dtype=torch.float32, device=d)
        self.reward_buf = torch.zeros((n,), dtype=torch.float32, device=d)
        self.reward2_buf = torch.zeros((n,), dtype=torch.float32, device=d)
        self.done_buf = torch.zeros((n,), dtype=torch.uint8, device=d)
        self.info_buf = torch.zeros((n, N.INFO_DIM), dtype=torch.float32, device=d)
        self.info2_buf = torch.zeros((n, N.INFO_DIM), dtype=torch.float32, device=d)
        self.actions_buf = torch.zeros((n, N.ACT_DIM), dtype=torch.float32, device=d)
        self.final_obs_buf = torch.zeros((n, N.OBS_DIM), dtype=torch.float32, device=d)
        self.record_buf = torch.zeros((n, N.RECORD_DIM), dtype=torch.float64, device=d)

    def _stream(self):
        # torch's current stream on this device as a raw hipStream_t: the C accessor, without building a
        # torch.cuda.Stream object (the single-env facade reads it on every step)
        return ctypes.c_void_p(_raw_stream(self._dev_index))

    def close(self):
        if getattr(self, "_ctx", None):
            self.L.hk_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def set_policy(self, player, policy):
        pid = _policy_id(policy)
        N.check(self.L.hk_set_policy(self._ctx, int(player), pid), "hk_set_policy")
        self.policies[player] = pid

    # ------------------------------------------------------------------ reset
    def _mirror_one_starts(self, mask, one_starting):
        """Advance the host mirror ``self.one_starts`` as a reset of the arenas ``mask`` selects does (NORMAL mode:
        toggle, or take ``one_starting``); returns the selection as a bool array."""
        n = self.n
        sel = np.ones(n, bool) if mask is None else np.asarray(mask.cpu() if torch.is_tensor(mask) else mask, bool)
        if self.mode == Mode.NORMAL:
            if one_starting is None:
                self.one_starts = np.where(sel, ~self.one_starts, self.one_starts)
            else:
                self.one_starts = np.where(sel, np.broadcast_to(np.asarray(one_starting, bool), (n,)), self.one_starts)
        return sel

    def _seed_tensor(self, seeds):
        """``seeds`` (int, sequence, numpy array or device int64 / uint64 tensor) as the [N] device words
        hk_seeded_params / hk_reset_seeded read: uint64 seeds, which a non-negative int64 tensor already is byte for
        byte.  Negative seeds raise ValueError, as gymnasium's np_random does (a device int64 tensor is checked with
        one reduction, a host synchronisation, except under stream capture); None and seeds >= 2**64 have no device
        form and raise too."""
        n = self.n
        if torch.is_tensor(seeds):
            t = seeds.to(self.device)
            if t.dtype not in (torch.int64, torch.uint64):
                raise ValueError(f"seeds tensor must be int64 or uint64, got {t.dtype}")
            t = t.expand(n) if t.dim() == 0 else t
            if t.shape != (n,):
                raise ValueError(f"seeds must have shape ({n},), got {tuple(t.shape)}")
            if t.dtype == torch.int64 and not torch.cuda.is_current_stream_capturing() and bool((t < 0).any()):
                raise ValueError("seeds must be non-negative")
            return t.contiguous()
        arr = np.asarray(seeds)
        if arr.dtype.kind not in "iu":  # Python ints past int64 (object arrays), None, mixed input: one by one
            vals = list(np.broadcast_to(np.asarray(seeds, dtype=object), (n,)))
            if any(s is None for s in vals):
                raise ValueError("device placement needs explicit seeds (seed=None draws OS entropy on the host)")
            vals = [int(s) for s in vals]
            if any(s >= 1 << 64 for s in vals):
                raise ValueError("device placement takes seeds below 2**64")
            arr = np.array(vals, dtype=object)
        if (arr < 0).any():
            raise ValueError("seeds must be non-negative")
        arr = np.array(np.broadcast_to(arr, (n,)), dtype=np.uint64)  # a copy: contiguous and writable
        # the uint64 bytes travel as an int64 tensor (torch's uint64 support is partial); the kernel reads uint64
        return torch.as_tensor(arr.view(np.int64), device=self.device)

    def seeded_params(self, seeds, one_starting=None):
        """The placement ``HockeyEnv.reset(seed=seeds[a])`` draws for arena a in this env's mode, drawn on the
        device (hk_seeded_params): (params [N,6] float32, max_t [N] int32), byte-equal to
        ``hockey_amd.placement.placement``.  one_starting: the puck side per arena (bool / bool array); None = each
        arena's stored flag as it stands.  Touches no arena and not the ``one_starts`` mirror."""
        st = self._seed_tensor(seeds)
        one_t = None
        if one_starting is not None:
            one = np.broadcast_to(np.asarray(one_starting.cpu() if torch.is_tensor(one_starting) else one_starting,
                                             bool), (self.n,))
            one_t = torch.as_tensor(one.astype(np.uint8), device=self.device)
        params = torch.empty((self.n, N.PARAM_DIM), dtype=torch.float32, device=self.device)
        max_t = torch.empty((self.n,), dtype=torch.int32, device=self.device)
        N.check(self.L.hk_seeded_params(self._ctx, N.ptr(st), N.ptr(one_t), N.ptr(params), N.ptr(max_t),
                                        self._stream()), "hk_seeded_params")
        return params, max_t

    def reset_seeded(self, seeds, mask=None, one_starting=None, max_t=None):
        """``HockeyEnv.reset(seed=seeds[a])`` for the selected arenas with the reference's PCG64 placement drawn on
        the device (hk_reset_seeded): the state ``reset(seeds=...)`` leaves, with no host draw and no upload.
        seeds: see _seed_tensor.  one_starting: None toggles like the reference (NORMAL mode), a bool / bool array
        forces the puck side; the ``one_starts`` mirror follows exactly as in reset().  max_t ([N] int32,
        optional) overrides the mode's max_timesteps and makes the call synchronous (range check).  With a device
        seeds tensor and no mask, one_starting or max_t, nothing is uploaded and the call is fire-and-forget: legal
        inside a torch.cuda.graph capture (the mirror advances once, at capture, not per replay).
        Returns observe()."""
        st = self._seed_tensor(seeds)
        sel = self._mirror_one_starts(mask, one_starting)
        mask_t = None if mask is None else torch.as_tensor(sel.astype(np.uint8), device=self.device)
        one_t = None
        if one_starting is not None:
            one_t = torch.as_tensor(self.one_starts.astype(np.uint8), device=self.device)
        mt = None if max_t is None else torch.as_tensor(max_t, dtype=torch.int32, device=self.device).contiguous()
        N.check(self.L.hk_reset_seeded(self._ctx, N.ptr(mask_t), N.ptr(st), N.ptr(mt), N.ptr(one_t), self._stream()),
                "hk_reset_seeded")
        return self.observe()

    def reset(self, seeds=None, mask=None, one_starting=None, placement="host"):
        """HockeyEnv.reset for the selected arenas.

        seeds: None -> device Philox placement; int / sequence -> the reference's PCG64 draws per arena
        (bit-identical placement to ``HockeyEnv.reset(seed=s)``).  one_starting: None toggles like the
        reference (NORMAL mode), a bool / bool array forces the puck side.  placement: where explicit seeds are
        drawn -- "host" (numpy, one Generator per arena, then uploaded) or "device" (reset_seeded: the same
        placement from the kernel; every seed must be an int in [0, 2**64)).
        Returns (obs[N,18], info[N,4]) tensors (agent-1 frame) for all arenas.
        """
        if placement not in ("host", "device"):
            raise ValueError("placement must be 'host' or 'device'")
        if placement == "device" and seeds is not None:
            return self.reset_seeded(seeds, mask=mask, one_starting=one_starting)
        n = self.n
        sel = self._mirror_one_starts(mask, one_starting)
        one_t = torch.as_tensor(self.one_starts.astype(np.uint8), device=self.device)
        mask_t = None if mask is None else torch.as_tensor(sel.astype(np.uint8), device=self.device)
        params_t = None
        if seeds is not None:
            seeds = np.broadcast_to(np.asarray(seeds, dtype=object), (n,))
            params = np.zeros((n, N.PARAM_DIM), np.float32)
            for i in np.nonzero(sel)[0]:
                rng, _ = np_random(None if seeds[i] is None else int(seeds[i]))
                params[i], _ = _host_placement(self.mode, bool(self.one_starts[i]), rng)
            params_t = torch.as_tensor(params, device=self.device)
        N.check(self.L.hk_reset(self._ctx, N.ptr(mask_t), N.ptr(params_t), None, N.ptr(one_t), self._stream()),
                "hk_reset")
        return self.observe()

    def reset_params(self, params, mask=None, max_t=None):
        """Reset from explicit placement vectors [N,6] (float32 on device)."""
        mask_t = None if mask is None else torch.as_tensor(mask, dtype=torch.uint8, device=self.device)
        mt = None if max_t is None else torch.as_tensor(max_t, dtype=torch.int32, device=self.device)
        params = torch.as_tensor(params, dtype=torch.float32, device=self.device).contiguous()
        N.check(self.L.hk_reset(self._ctx, N.ptr(mask_t), N.ptr(params), N.ptr(mt), None, self._stream()), "hk_reset")

    # ------------------------------------------------------------------ step
    def step(self, actions=None, with_agent_two=False, opp_inc=None, debug=None, skip_physics=False,
             record_actions=False, final_obs=False, policy2=None, record=False):
        """HockeyEnv.step for every arena.  actions: [N,8] float (clipped in-kernel), may be None when no
        player is external.  Returns a StepResult of device tensors (views of persistent buffers).

        With auto_reset, an arena that is done after this step is reset at its end: done / reward / info are
        the terminal step's, obs / obs2 the new episode's first state, and ``final_obs`` (when requested) the
        terminal observation (== obs for arenas that did not reset).

        policy2 ([N] uint8 / policy ids, optional): player 2's policy of each arena for this step, overriding
        the context's (rl/training/opponent_manager.py draws the opponent per step); 'external' arenas read
        actions[:, 4:8].

        record: also return the [N,16] float64 step record (include/hockey.h hk_step_io.record: info, info2,
        reward, reward2 in float64 and has_puck1/2, time, done, winner after the step)."""
        a = None
        if actions is not None:
            a = torch.as_tensor(actions, dtype=torch.float32, device=self.device)
            if a.shape != (self.n, N.ACT_DIM):
                raise ValueError(f"actions must have shape ({self.n}, {N.ACT_DIM}), got {tuple(a.shape)}")
            a = a.contiguous()
        inc = None
        if opp_inc is not None:
            inc = torch.as_tensor(opp_inc, dtype=torch.float64, device=self.device).contiguous()
        io = N.StepIO()
        io.actions = None if a is None else a.data_ptr()
        io.opp_inc = None if inc is None else inc.data_ptr()
        io.obs = self.obs_buf.data_ptr()
        io.reward = self.reward_buf.data_ptr()
        io.done = self.done_buf.data_ptr()
        io.info = self.info_buf.data_ptr()
        if with_agent_two:
            io.obs2 = self.obs2_buf.data_ptr()
            io.reward2 = self.reward2_buf.data_ptr()
            io.info2 = self.info2_buf.data_ptr()
        if record_actions:
            io.actions_out = self.actions_buf.data_ptr()
        if debug is not None:
            io.debug = debug.data_ptr()
        if final_obs:
            io.final_obs = self.final_obs_buf.data_ptr()
        if record:
            io.record = self.record_buf.data_ptr()
        io.flags = N.STEP_SKIP_PHYSICS if skip_physics else 0
        p2 = None
        if policy2 is not None:
            p2 = torch.as_tensor(policy2, dtype=torch.uint8, device=self.device).contiguous()
            if p2.shape != (self.n,):
                raise ValueError(f"policy2 must have shape ({self.n},), got {tuple(p2.shape)}")
            io.policy2 = p2.data_ptr()
        N.check(self.L.hk_step(self._ctx, ctypes.byref(io), self._stream()), "hk_step")
        return StepResult(obs=self.obs_buf, reward=self.reward_buf, done=self.done_buf, info=self.info_buf,
                          obs2=self.obs2_buf if with_agent_two else None,
                          reward2=self.reward2_buf if with_agent_two else None,
                          info2=self.info2_buf if with_agent_two else None,
                          actions=self.actions_buf if record_actions else None,
                          final_obs=self.final_obs_buf if final_obs else None,
                          record=self.record_buf if record else None)

    def step_raw(self, io):
        """Launch one step with a prepared StepIO (no Python-side allocation; for benchmarks)."""
        N.check(self.L.hk_step(self._ctx, ctypes.byref(io), self._stream()), "hk_step")

    def rollout(self, n_steps, actions=None, with_agent_two=False, record_actions=False, final_obs=False):
        """``n_steps`` consecutive steps in one launch (hk_rollout).  Returns a StepResult whose tensors carry a
        leading [n_steps] dimension.  ``actions`` ([n_steps, N, 8]) is needed only for external players."""
        k, n = int(n_steps), self.n
        d = self.device
        a = None
        if actions is not None:
            a = torch.as_tensor(actions, dtype=torch.float32, device=d)
            if a.shape != (k, n, N.ACT_DIM):
                raise ValueError(f"actions must have shape ({k}, {n}, {N.ACT_DIM}), got {tuple(a.shape)}")
            a = a.contiguous()
        obs = torch.empty((k, n, N.OBS_DIM), dtype=torch.float32, device=d)
        rew = torch.empty((k, n), dtype=torch.float32, device=d)
        done = torch.empty((k, n), dtype=torch.uint8, device=d)
        info = torch.empty((k, n, N.INFO_DIM), dtype=torch.float32, device=d)
        io = N.StepIO()
        io.actions = None if a is None else a.data_ptr()
        io.obs, io.reward, io.done, io.info = obs.data_ptr(), rew.data_ptr(), done.data_ptr(), info.data_ptr()
        obs2 = rew2 = info2 = acts = None
        if with_agent_two:
            obs2 = torch.empty_like(obs)
            rew2 = torch.empty_like(rew)
            info2 = torch.empty_like(info)
            io.obs2, io.reward2, io.info2 = obs2.data_ptr(), rew2.data_ptr(), info2.data_ptr()
        if record_actions:
            acts = torch.empty((k, n, N.ACT_DIM), dtype=torch.float32, device=d)
            io.actions_out = acts.data_ptr()
        fobs = None
        if final_obs:
            fobs = torch.empty_like(obs)
            io.final_obs = fobs.data_ptr()
        N.check(self.L.hk_rollout(self._ctx, k, ctypes.byref(io), self._stream()), "hk_rollout")
        return StepResult(obs=obs, reward=rew, done=done, info=info, obs2=obs2, reward2=rew2, info2=info2,
                          actions=acts, final_obs=fobs)

    def rollout_raw(self, n_steps, io):
        """hk_rollout with a prepared StepIO whose arrays have a leading [n_steps] dimension."""
        N.check(self.L.hk_rollout(self._ctx, int(n_steps), ctypes.byref(io), self._stream()), "hk_rollout")

    # ------------------------------------------------------------------ state / obs
    def observe(self):
        N.check(self.L.hk_observe(self._ctx, N.ptr(self.obs_buf), N.ptr(self.obs2_buf), self._stream()), "hk_observe")
        return self.obs_buf, self.obs2_buf

    def info(self):
        """(info[N,4], info2[N,4], reward[N], reward2[N]) float64 of the current state (hk_info): _get_info,
        get_info_agent_two and the matching get_reward / get_reward_agent_two of hockey_env.py:518-591."""
        d, n = self.device, self.n
        i1 = torch.empty((n, N.INFO_DIM), dtype=torch.float64, device=d)
        i2 = torch.empty((n, N.INFO_DIM), dtype=torch.float64, device=d)
        r1 = torch.empty((n,), dtype=torch.float64, device=d)
        r2 = torch.empty((n,), dtype=torch.float64, device=d)
        N.check(self.L.hk_info(self._ctx, N.ptr(i1), N.ptr(i2), N.ptr(r1), N.ptr(r2), self._stream()), "hk_info")
        return i1, i2, r1, r2

    def obs_agent_two(self):
        return self.observe()[1]

    def get_state(self):
        st = torch.zeros((self.n, N.STATE_DIM), dtype=torch.float32, device=self.device)
        aux = torch.zeros((self.n, N.AUX_DIM), dtype=torch.int32, device=self.device)
        N.check(self.L.hk_get_state(self._ctx, N.ptr(st), N.ptr(aux), self._stream()), "hk_get_state")
        return st, aux

    def render(self, indices=None, height=480, width=600, format="rgb", out=None):
        """HockeyEnv.render("rgb_array") (hockey_env.py:697-744) for the arenas ``indices`` (all when None), at any
        size: a uint8 device tensor [m, height, width, 3], or [m, height, width] palette indices with
        format="index" (hockey_amd.render).  The frames show the current state; rendering does not touch it."""
        from .render import render_states

        st, _ = self.get_state()
        return render_states(st, indices, height, width, format, out=out)

    def set_state(self, state=None, aux=None, mask=None):
        st = None if state is None else torch.as_tensor(state, dtype=torch.float32, device=self.device).contiguous()
        ax = None if aux is None else torch.as_tensor(aux, dtype=torch.int32, device=self.device).contiguous()
        mk = None if mask is None else torch.as_tensor(mask, dtype=torch.uint8, device=self.device).contiguous()
        N.check(self.L.hk_set_state(self._ctx, N.ptr(mk), N.ptr(st), N.ptr(ax), self._stream()), "hk_set_state")

    # ------------------------------------------------------------------ exact snapshots / restore / fork
    def snapshot(self, indices=None, assume_valid=False):
        """The exact state of arenas ``indices`` (all when None) as an ArenaSnapshot on this device (hk_snapshot):
        unlike get_state it carries contacts with their warm-start impulses, sleep times, the puck's pending force,
        the BasicOpponent phases and the episode / step words that key the device draws, so a restore continues bit
        for bit.  Counters and the host-side ``one_starts`` mirror that reset() toggles are not part of it.
        Index checks run in torch (a host synchronisation) unless ``assume_valid``."""
        from . import snapshot as S

        idx = S.index_tensor(indices, self.device)
        m = self.n if idx is None else idx.numel()
        if not assume_valid:
            S.check_indices(None, m, idx, self.n, m, what="snapshot")
        # zeros: the sections' padding bytes are then defined, and equal arenas give equal blobs
        blob = torch.zeros(S.snapshot_bytes(m), dtype=torch.uint8, device=self.device)
        N.check(self.L.hk_snapshot(self._ctx, N.ptr(idx), m, N.ptr(blob), self._stream()), "hk_snapshot")
        return S.ArenaSnapshot(blob, m, S.library_version(), S.library_layout(), self.keep_mode,
                               self.vel_ref_semantics)

    def restore(self, snap, indices=None, rows=None, assume_valid=False):
        """Arena ``indices[e]`` (e when None) = row ``rows[e]`` (e when None) of ``snap`` (hk_restore).  A restore to
        the index the row was taken from continues the identical device random stream; at another index the arena
        continues with that index's stream (include/hockey.h).  A snapshot on another device is moved here first."""
        from . import snapshot as S

        snap.check(what="restore")
        if snap.keep_mode != self.keep_mode or snap.vel_ref != self.vel_ref_semantics:
            raise N.HockeyNativeError(
                f"restore: snapshot written with keep_mode={snap.keep_mode}, vel_ref={snap.vel_ref}; this env has "
                f"keep_mode={self.keep_mode}, vel_ref={self.vel_ref_semantics}")
        if snap.device != self.device:
            snap = snap.to(self.device)
        idx, row = S.index_tensor(indices, self.device), S.index_tensor(rows, self.device)
        m = idx.numel() if idx is not None else (row.numel() if row is not None else snap.count)
        if not assume_valid:
            S.check_indices(idx, self.n, row, snap.count, m, what="restore")
        blob = snap.blob.contiguous()
        N.check(self.L.hk_restore(self._ctx, N.ptr(idx), m, N.ptr(blob), snap.count, N.ptr(row), self._stream()),
                "hk_restore")

    def fork(self, src, dst=None, source=None, assume_valid=False):
        """Copy arenas ``src`` of env ``source`` (default: this env) into arenas ``dst`` of this env (0..m-1 when
        None), exactly (hk_copy_arenas).  A source index may repeat (one arena into K destinations); destinations
        must be distinct and, within one env, disjoint from the sources.  Both envs share device, keep_mode and
        vel_ref_semantics; mode and auto_reset may differ.  With ``assume_valid`` no check runs and the call is
        fire-and-forget (legal inside a torch.cuda.graph capture when the index lists are device int64 tensors)."""
        from . import snapshot as S

        source = self if source is None else source
        s, d = S.index_tensor(src, self.device), S.index_tensor(dst, self.device)
        m = s.numel() if s is not None else (d.numel() if d is not None else min(self.n, source.n))
        if not assume_valid:
            S.check_indices(d, self.n, s, source.n, m, same_env=source is self, what="fork")
        N.check(self.L.hk_copy_arenas(self._ctx, N.ptr(d), source._ctx, N.ptr(s), m, self._stream()),
                "hk_copy_arenas")

    def opponent_phase(self, new_phase=None, rows=2):
        """Return the BasicOpponent phases [N,rows] (float64, device); optionally overwrite them.  rows=2:
        player 1 / player 2 (hk_opponent_phase); rows=3 adds player 2's weak bot under a policy2 override
        (hk_opponent_phase3, include/hockey.h states which step walks which row)."""
        if rows not in (2, 3):
            raise ValueError("rows must be 2 or 3")
        out = torch.zeros((self.n, rows), dtype=torch.float64, device=self.device)
        ph = None if new_phase is None else torch.as_tensor(new_phase, dtype=torch.float64,
                                                            device=self.device).contiguous()
        if ph is not None and ph.shape != (self.n, rows):
            raise ValueError(f"new_phase must have shape ({self.n}, {rows})")
        fn = self.L.hk_opponent_phase if rows == 2 else self.L.hk_opponent_phase3
        N.check(fn(self._ctx, N.ptr(out), N.ptr(ph), self._stream()), "hk_opponent_phase")
        return out

    def counters(self):
        out = (ctypes.c_int64 * N.NUM_COUNTERS)()
        N.check(self.L.hk_counters(self._ctx, out, self._stream()), "hk_counters")
        return np.array(out[:], np.int64)

    def reset_counters(self):
        N.check(self.L.hk_reset_counters(self._ctx, self._stream()), "hk_reset_counters")

    def bytes_per_step(self):
        a, b = ctypes.c_int64(), ctypes.c_int64()
        N.check(self.L.hk_bytes_per_step(self._ctx, ctypes.byref(a), ctypes.byref(b)), "hk_bytes_per_step")
        return a.value, b.value
