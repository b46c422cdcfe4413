"""ctypes binding of the fused fp32 MFMA TD3 learner (include/hockey_learner.h; the C ABI in csrc/hk_learner.hip, its
kernels in csrc/hkl_mlp.h, hkl_td3.h, hkl_per.h, hkl_act.h, hkl_explore.h and hkl_value.h).

``FusedLearner(agent, ring, batch)`` performs ``agent``'s learner updates (rl/td3/learner.py:55-218: clipped
double-Q target with policy smoothing, weighted smooth-L1 critic loss, delayed actor update, Polyak averaging, Adam
with the config's lr / eps 1e-6 / weight decay) on ``ring`` with a handful of HIP kernels per update instead of a few
hundred PyTorch ops.  The agent's modules stay the parameter owners (checkpoints, evaluation and acting use them
unchanged); their parameters are re-pointed into one flat buffer per network so that Polyak averaging is one launch.

Randomness is drawn by torch in the eager update's order -- the sampled slots (``ring.sample_indices``) and then the
target noise ``torch.randn_like`` of shape [B, 4] -- so from the same generator state a fused update consumes exactly
the eager update's random numbers (tests/test_gpu_learner.py compares the two).  The optimiser state is the
learner's own (Adam moments in fp32 device buffers): ``agent.opt_critic`` / ``opt_actor`` are not used.

On a ``hockey_amd.td3.DevicePrioritizedRing`` the prioritized slots, importance weights and the priority write-back are
the hkl_per_* kernels (per-block float64 sums; the slots come from the Philox stream under rng="device").

``ActIO`` / ``hkl_act`` (actor inference over a bank of policies) and ``ActWideIO`` / ``hkl_act_wide`` (the same over up
to 4 096 policies) are bound here and driven by ``hockey_amd.policy_bank.PolicyBank``; ``ValueIO`` / ``hkl_value`` (twin-critic inference) by
``hockey_amd.value.ValueFn``; ``ExploreIO`` / ``hkl_explore`` (acting with exploration) by ``hockey_amd.explore.Explorer``; ``OppDrawIO`` /
``hkl_opp_draw`` and ``CollectIO`` / ``hkl_collect`` (the opponent draw and the replay store of a collection step) by
``hockey_amd.collect.Collector``; ``EvalIO`` / ``hkl_eval_begin`` / ``hkl_eval_step`` / ``hkl_eval_fold`` (the evaluation
loop's accounting) by ``hockey_amd.evaluator.Evaluator``.  The ``hkl_*_group`` forms (up to 64 independent learners per launch, each bit for bit
its single call), ``hkl_per_*_group`` among them, are bound here and driven by
``hockey_amd.population.PopulationLearner`` and ``PopulationPrioritizedRing``.

Every call is asynchronous on torch's current stream and graph-capturable (fixed buffers, device step counters).
There is no CPU path: construction fails loudly without the library or a GPU.
"""
import ctypes
import os

import torch

from . import _native

LIB_PATH = os.environ.get("HK_LEARNER_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib",
                                                            "libhockey_learner.so")
PACK_FLOATS = 16 * 64 * 8 + 2 * 16 * 16 * 64 * 4 + 16 * 64 * 4 + 256 * 4
MAX_SEG = 12
CHUNK = 256  # batch granularity (include/hockey_learner.h)
XP = 32
ACT_MAX_POLICIES = 64  # HKL_ACT_MAX_POLICIES
ACT_WIDE_MAX_POLICIES = 4096  # HKL_ACT_WIDE_MAX_POLICIES
GROUP_MAX = 64  # HKL_GROUP_MAX: members of one grouped learner launch (hockey_amd.population)
ACT_PARAM_FLOATS = 256 * 18 + 256 + 256 * 256 + 256 + 4 * 256 + 4  # HKL_ACT_PARAM_FLOATS: one bank slot's weights

vp = ctypes.c_void_p


class Net(ctypes.Structure):
    _fields_ = [("w1", vp), ("b1", vp), ("w2", vp), ("b2", vp), ("w3", vp), ("b3", vp), ("pack", vp),
                ("n_in", ctypes.c_int32), ("n_out", ctypes.c_int32)]


class CriticIO(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int64), ("idx", vp), ("ring_s", vp), ("ring_a", vp), ("ring_r", vp),
                ("ring_s2", vp), ("ring_d", vp), ("noise", vp), ("iw", vp), ("target_actor", Net),
                ("target_q", Net * 2), ("q", Net * 2), ("gamma", ctypes.c_float), ("act_low", ctypes.c_float * 4),
                ("act_range", ctypes.c_float * 4), ("x0", vp), ("h1", vp * 2), ("dz1", vp * 2), ("dz2", vp * 2),
                ("p_db1", vp * 2), ("p_db2", vp * 2), ("p_dw3", vp * 2), ("p_db3", vp * 2), ("p_loss", vp),
                ("td", vp), ("sample_counter", vp)]


class SampleIO(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int64), ("seed", ctypes.c_uint64), ("counter", vp), ("size", vp), ("idx", vp),
                ("noise", vp), ("scale", ctypes.c_float), ("clip", ctypes.c_float)]


class ActorIO(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int64), ("idx", vp), ("ring_s", vp), ("actor", Net), ("q1", Net),
                ("act_low", ctypes.c_float * 4), ("act_range", ctypes.c_float * 4), ("x0", vp), ("h1", vp),
                ("h2", vp), ("dz1", vp), ("dz2", vp), ("p_db1", vp), ("p_db2", vp), ("p_dw3", vp), ("p_db3", vp),
                ("p_loss", vp)]


class WgJob(ctypes.Structure):
    _fields_ = [("dz", vp), ("x", vp), ("slab", vp), ("bias_slab", vp)]


class Seg(ctypes.Structure):
    _fields_ = [("param", vp), ("m", vp), ("v", vp), ("src", vp), ("rows", ctypes.c_int32), ("cols", ctypes.c_int32),
                ("ld", ctypes.c_int64), ("chunks", ctypes.c_int32), ("stride", ctypes.c_int64), ("target", vp)]


class AdamIO(ctypes.Structure):
    _fields_ = [("seg", Seg * MAX_SEG), ("n_seg", ctypes.c_int32), ("lr", ctypes.c_float), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("eps", ctypes.c_float), ("wd", ctypes.c_float), ("step", vp),
                ("loss_src", vp), ("loss_chunks", ctypes.c_int32), ("loss_scale", ctypes.c_float),
                ("loss_sum", vp), ("loss_count", vp), ("polyak", ctypes.c_int32), ("polyak_rho", ctypes.c_float),
                ("polyak_tau", ctypes.c_float)]


class PackIO(ctypes.Structure):
    """hkl_pack_io: up to four networks to re-pack and the optimiser step counter the pack advances."""
    _fields_ = [("net", Net * 4), ("step", vp)]


class Per(ctypes.Structure):
    _fields_ = [("cap", ctypes.c_int64), ("w", vp), ("size", vp), ("bsum", vp), ("bmax", vp), ("bpre", vp),
                ("last", vp), ("bown", vp)]


class PerSampleIO(ctypes.Structure):
    _fields_ = [("per", Per), ("batch", ctypes.c_int64), ("seed", ctypes.c_uint64), ("counter", vp), ("u", vp),
                ("idx", vp), ("noise", vp), ("scale", ctypes.c_float), ("clip", ctypes.c_float), ("iw", vp),
                ("beta", ctypes.c_double)]


class PerUpdateIO(ctypes.Structure):
    _fields_ = [("per", Per), ("batch", ctypes.c_int64), ("idx", vp), ("td", vp)]


class ActIO(ctypes.Structure):
    """hkl_act_io: actor inference over a bank of policies (hockey_amd.policy_bank)."""
    _fields_ = [("n_policies", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("params", vp), ("packs", vp),
                ("obs", vp), ("obs_ld", ctypes.c_int64), ("policy", vp), ("out", vp), ("out_ld", ctypes.c_int64),
                ("out_col", ctypes.c_int32), ("order", vp), ("counts", vp), ("offsets", vp)]


class ActWideIO(ctypes.Structure):
    """hkl_act_wide_io: hkl_act over a bank of up to ACT_WIDE_MAX_POLICIES policies (hockey_amd.policy_bank)."""
    _fields_ = [("n_policies", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("params", vp), ("packs", vp),
                ("obs", vp), ("obs_ld", ctypes.c_int64), ("policy", vp), ("out", vp), ("out_ld", ctypes.c_int64),
                ("out_col", ctypes.c_int32), ("order", vp), ("counts", vp), ("offsets", vp), ("tiles", vp)]


class ExploreMember(ctypes.Structure):
    """hkl_explore_member: one member's exploration parameters (hockey_amd.explore)."""
    _fields_ = [("seed", ctypes.c_uint64), ("start_steps", ctypes.c_int64), ("max_total_steps", ctypes.c_int64),
                ("init_scale", ctypes.c_double), ("min_scale", ctypes.c_double), ("anneal", ctypes.c_int32),
                ("noise", ctypes.c_int32), ("theta", ctypes.c_float), ("dt", ctypes.c_float),
                ("sqrt_dt", ctypes.c_float), ("reserved", ctypes.c_int32)]


class ExploreIO(ctypes.Structure):
    """hkl_explore_io: hkl_act with the exploration epilogue (hockey_amd.explore)."""
    _fields_ = [("act", ActIO), ("rows_per_member", ctypes.c_int32), ("members", vp), ("total", vp), ("calls", vp),
                ("count", vp), ("x", vp), ("ext", vp), ("ext_ld", ctypes.c_int64), ("ext_cs", ctypes.c_int64),
                ("z_out", vp), ("scale_out", vp)]


class OppDrawIO(ctypes.Structure):
    """hkl_opp_draw_io: player 2's opponent draw, one lane per arena (hockey_amd.collect)."""
    _fields_ = [("n_rows", ctypes.c_int32), ("rows_per_member", ctypes.c_int32), ("pmax", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("seeds", vp), ("calls", vp), ("probs", vp), ("len", vp), ("scores", vp),
                ("slots", vp), ("alive", vp), ("policy2", vp), ("policy", vp), ("snap", vp), ("opp_inc", vp),
                ("counts", vp), ("snap_counts", vp)]


class CollectIO(ctypes.Structure):
    """hkl_collect_io: the replay store and the step's bookkeeping (hockey_amd.collect)."""
    _fields_ = [("n_rows", ctypes.c_int32), ("rows_per_member", ctypes.c_int32), ("pmax", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("obs", vp), ("act", vp), ("act_ld", ctypes.c_int64), ("obs_next", vp),
                ("obs2_next", vp), ("reward", vp), ("done", vp), ("snap", vp), ("alive", vp), ("s", vp), ("a", vp),
                ("r", vp), ("s2", vp), ("d", vp), ("cap", ctypes.c_int64), ("pos", vp), ("size", vp),
                ("ep_reward", vp), ("tally", vp), ("push_pos", vp), ("push_n", vp), ("count", vp), ("steps", vp),
                ("live", vp), ("keep_obs", vp), ("keep_obs2", vp), ("scratch", vp)]


class EvalIO(ctypes.Structure):
    """hkl_eval_io: the evaluation loop's accounting and its fold (hockey_amd.evaluator)."""
    _fields_ = [("n_rows", ctypes.c_int32), ("rows_per_cell", ctypes.c_int32), ("info_ld", ctypes.c_int64),
                ("seeds", vp), ("step", vp), ("reward", vp), ("done", vp), ("info", vp), ("live", vp), ("ret", vp),
                ("length", vp), ("winner", vp), ("count", vp), ("opp_inc", vp), ("outcomes", vp), ("length_sum", vp),
                ("return_sum", vp)]


def act_wide_max_tiles(n_rows, n_policies):
    """The bound on the non-empty 64-row tiles of hkl_act_wide: its ``tiles`` scratch holds 3 int32 per tile."""
    return min(n_rows, -(-n_rows // 64) + n_policies)


class ValueIO(ctypes.Structure):
    """hkl_value_io: twin-critic inference, Q(obs, act) or V(obs) = min Q(obs, actor(obs)) (hockey_amd.value)."""
    _fields_ = [("n_rows", ctypes.c_int32), ("actor", Net), ("q", Net * 2), ("obs", vp), ("obs_ld", ctypes.c_int64),
                ("act", vp), ("act_ld", ctypes.c_int64), ("act_low", ctypes.c_float * 4),
                ("act_range", ctypes.c_float * 4), ("q1", vp), ("q2", vp), ("qmin", vp), ("act_out", vp),
                ("act_out_ld", ctypes.c_int64)]


EXPORTS = ["hkl_last_error", "hkl_pack_floats", "hkl_pack", "hkl_critic_step", "hkl_actor_step", "hkl_wgrad",
           "hkl_wgrad_pair",
           "hkl_adam", "hkl_polyak", "hkl_tanh_probe", "hkl_sample", "hkl_per_block", "hkl_per_refresh",
           "hkl_per_push", "hkl_per_sample", "hkl_per_weights", "hkl_per_update", "hkl_act", "hkl_act_io_size", "hkl_act_wide",
           "hkl_act_wide_io_size", "hkl_value",
           "hkl_value_io_size", "hkl_sample_group", "hkl_critic_step_group", "hkl_actor_step_group",
           "hkl_wgrad_pair_group", "hkl_adam_group", "hkl_pack_group", "hkl_per_sample_group",
           "hkl_per_weights_group", "hkl_per_update_group", "hkl_per_refresh_group", "hkl_per_push_group"]


# include/hockey_explore.h (exploration acting), a header of its own beside hockey_learner.h's entry points above
EXPLORE_EXPORTS = ["hkl_explore", "hkl_explore_io_size", "hkl_explore_member_size"]

# include/hockey_collect.h (the opponent draw and the replay store), likewise
COLLECT_EXPORTS = ["hkl_opp_draw", "hkl_opp_draw_io_size", "hkl_collect", "hkl_collect_io_size",
                   "hkl_collect_scratch_ints"]

# include/hockey_eval.h (the evaluation loop's accounting and its fold), likewise
EVAL_EXPORTS = ["hkl_eval_begin", "hkl_eval_step", "hkl_eval_fold", "hkl_eval_io_size"]

_lib = None


def lib():
    """The loaded learner library; raises HockeyNativeError if it is missing (no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise _native.HockeyNativeError(
                f"{LIB_PATH} not found: build it with `make -C hockey-env_amd/csrc` (hipcc, gfx950)")
        L = ctypes.CDLL(LIB_PATH)
        L.hkl_last_error.restype = ctypes.c_char_p
        L.hkl_pack.argtypes = [ctypes.POINTER(Net), ctypes.c_int, vp, vp]
        L.hkl_critic_step.argtypes = [ctypes.POINTER(CriticIO), vp]
        L.hkl_actor_step.argtypes = [ctypes.POINTER(ActorIO), vp]
        L.hkl_wgrad.argtypes = [ctypes.POINTER(WgJob), ctypes.c_int, ctypes.c_int, ctypes.c_int64, vp]
        L.hkl_wgrad_pair.argtypes = [ctypes.POINTER(WgJob), ctypes.c_int, ctypes.POINTER(WgJob), ctypes.c_int,
                                     ctypes.c_int64, vp]
        L.hkl_adam.argtypes = [ctypes.POINTER(AdamIO), vp]
        L.hkl_polyak.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_float, ctypes.c_float, vp]
        L.hkl_tanh_probe.argtypes = [vp, vp, ctypes.c_int64, vp]
        L.hkl_sample.argtypes = [ctypes.POINTER(SampleIO), vp]
        L.hkl_per_refresh.argtypes = [ctypes.POINTER(Per), ctypes.c_int64, ctypes.c_int64, vp]
        L.hkl_per_push.argtypes = [ctypes.POINTER(Per), ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, vp]
        L.hkl_per_sample.argtypes = [ctypes.POINTER(PerSampleIO), vp]
        L.hkl_per_weights.argtypes = [ctypes.POINTER(PerSampleIO), vp]
        L.hkl_per_update.argtypes = [ctypes.POINTER(PerUpdateIO), vp]
        L.hkl_act.argtypes = [ctypes.POINTER(ActIO), vp]
        L.hkl_act_wide.argtypes = [ctypes.POINTER(ActWideIO), vp]
        L.hkl_value.argtypes = [ctypes.POINTER(ValueIO), vp]
        L.hkl_explore.argtypes = [ctypes.POINTER(ExploreIO), ctypes.POINTER(ExploreMember), vp]
        L.hkl_opp_draw.argtypes = [ctypes.POINTER(OppDrawIO), vp]
        L.hkl_collect.argtypes = [ctypes.POINTER(CollectIO), vp]
        L.hkl_collect_scratch_ints.argtypes = [ctypes.c_int32, ctypes.c_int32]
        L.hkl_collect_scratch_ints.restype = ctypes.c_int64
        for name in ("hkl_eval_begin", "hkl_eval_step", "hkl_eval_fold"):
            getattr(L, name).argtypes = [ctypes.POINTER(EvalIO), vp]
        # grouped forms: (host array, the same bytes on the device, ..., n_members, stream)
        L.hkl_sample_group.argtypes = [ctypes.POINTER(SampleIO), vp, ctypes.c_int, vp]
        L.hkl_critic_step_group.argtypes = [ctypes.POINTER(CriticIO), vp, ctypes.c_int, vp]
        L.hkl_actor_step_group.argtypes = [ctypes.POINTER(ActorIO), vp, ctypes.c_int, vp]
        L.hkl_wgrad_pair_group.argtypes = [ctypes.POINTER(WgJob), vp, ctypes.c_int, ctypes.POINTER(WgJob), vp,
                                           ctypes.c_int, ctypes.c_int64, ctypes.c_int, vp]
        L.hkl_adam_group.argtypes = [ctypes.POINTER(AdamIO), vp, ctypes.c_int, vp]
        L.hkl_pack_group.argtypes = [ctypes.POINTER(PackIO), vp, ctypes.c_int, ctypes.c_int, vp]
        L.hkl_per_sample_group.argtypes = [ctypes.POINTER(PerSampleIO), vp, ctypes.c_int, vp]
        L.hkl_per_weights_group.argtypes = [ctypes.POINTER(PerSampleIO), vp, ctypes.c_int, vp]
        L.hkl_per_update_group.argtypes = [ctypes.POINTER(PerUpdateIO), vp, ctypes.c_int, vp]
        L.hkl_per_refresh_group.argtypes = [ctypes.POINTER(Per), vp, ctypes.c_int, vp]
        # (host, dev, pos, n, size_after: device int64[n_members], max_n, n_members, stream)
        L.hkl_per_push_group.argtypes = [ctypes.POINTER(Per), vp, vp, vp, vp, ctypes.c_int64, ctypes.c_int, vp]
        if L.hkl_pack_floats() != PACK_FLOATS:
            raise _native.HockeyNativeError("libhockey_learner.so pack size differs from hockey_amd.learner_hip")
        if L.hkl_act_io_size() != ctypes.sizeof(ActIO):
            raise _native.HockeyNativeError("libhockey_learner.so hkl_act_io differs from hockey_amd.learner_hip")
        if L.hkl_act_wide_io_size() != ctypes.sizeof(ActWideIO):
            raise _native.HockeyNativeError("libhockey_learner.so hkl_act_wide_io differs from hockey_amd.learner_hip")
        if L.hkl_value_io_size() != ctypes.sizeof(ValueIO):
            raise _native.HockeyNativeError("libhockey_learner.so hkl_value_io differs from hockey_amd.learner_hip")
        if (L.hkl_explore_io_size() != ctypes.sizeof(ExploreIO)
                or L.hkl_explore_member_size() != ctypes.sizeof(ExploreMember)):
            raise _native.HockeyNativeError("libhockey_learner.so hkl_explore_io differs from hockey_amd.learner_hip")
        if (L.hkl_opp_draw_io_size() != ctypes.sizeof(OppDrawIO)
                or L.hkl_collect_io_size() != ctypes.sizeof(CollectIO)):
            raise _native.HockeyNativeError("libhockey_learner.so hkl_collect_io differs from hockey_amd.learner_hip")
        if L.hkl_eval_io_size() != ctypes.sizeof(EvalIO):
            raise _native.HockeyNativeError("libhockey_learner.so hkl_eval_io differs from hockey_amd.learner_hip")
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        raise _native.HockeyNativeError(f"{what} failed ({rc}): {lib().hkl_last_error().decode()}")


ptr = _native.ptr  # raw device pointer of a tensor (None -> NULL)


def stream_ptr(device):
    """torch's current stream on ``device``, as the stream argument of every native call."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def upload(arr, device):
    """The bytes of a ctypes array in device memory (uint8 tensor; the allocator's alignment exceeds any struct's)."""
    return torch.frombuffer(bytearray(arr), dtype=torch.uint8).to(device)


_check, _p = check, ptr  # the names older callers and the tests use


def tanh_probe(x):
    """The fused kernels' tanh of a device float32 tensor (accuracy check)."""
    x = x.contiguous().float()
    y = torch.empty_like(x)
    _check(lib().hkl_tanh_probe(_p(x), _p(y), x.numel(), stream_ptr(x.device)), "hkl_tanh_probe")
    return y


def flatten_(module):
    """Re-point every parameter of ``module`` into one contiguous fp32 buffer (values unchanged); returns it."""
    params = list(module.parameters())
    flat = torch.cat([p.detach().reshape(-1) for p in params]).contiguous()
    o = 0
    for p in params:
        n = p.numel()
        p.data = flat[o:o + n].view_as(p)
        o += n
    return flat


def _mlp_layers(m):
    """(fc1, fc2, fc3) of an Actor / _QNet."""
    return m.fc1, m.fc2, m.fc3


class _NetBufs:
    """One MLP's parameter pointers and its MFMA operand pack."""

    def __init__(self, m, device):
        self.m = m
        self.pack = torch.zeros(PACK_FLOATS, dtype=torch.float32, device=device)
        f1, f2, f3 = _mlp_layers(m)
        self.net = Net(_p(f1.weight), _p(f1.bias), _p(f2.weight), _p(f2.bias), _p(f3.weight), _p(f3.bias),
                       _p(self.pack), f1.in_features, f3.out_features)


class FusedLearner:
    """Learner updates of ``agent`` (hockey_amd.td3.TD3) on ``ring`` at batch ``batch`` (a multiple of 256) with the
    fused kernels; same interface as the eager path: ``update(train_actor, acc)``."""

    def __init__(self, agent, ring, batch, rng="device", seed=None):
        L = lib()
        if rng not in ("device", "torch"):
            raise ValueError("rng must be 'device' or 'torch'")
        self.rng = rng
        self.L = L
        self.agent, self.ring, self.B = agent, ring, int(batch)
        if getattr(agent, "_fused_learner", None) is not None:
            raise RuntimeError("FusedLearner: this agent already has a fused learner (one owns its Adam state)")
        dev = agent.device
        if dev.type != "cuda":
            raise _native.HockeyNativeError("the fused learner runs on the GPU only")
        if self.B <= 0 or self.B % CHUNK:
            raise ValueError(f"fused learner batch must be a positive multiple of {CHUNK}, got {self.B}")
        if agent.actor.fc1.out_features != 256:
            raise ValueError("fused learner: hidden width 256 only (rl/td3/networks.py h)")
        B, G = self.B, self.B // 64
        C = self.B // (512 if self.B % 512 == 0 else 256)  # hkl_wgrad's split-K chunks: the critics' dW2 (2 jobs)
        CA = self.B // 256  # the actor's dW2 (one k-width-256 job: 256-sample chunks, include/hockey_learner.h)
        C1 = self.B // 256  # dW1 (k width 32)
        c = agent.cfg
        self.cfg = c
        self.flat = {k: flatten_(getattr(agent, k)) for k in ("actor", "critic", "target_actor", "target_critic")}
        self.m = {k: torch.zeros_like(self.flat[k]) for k in ("actor", "critic")}
        self.v = {k: torch.zeros_like(self.flat[k]) for k in ("actor", "critic")}
        self.step = {k: torch.zeros((), dtype=torch.int64, device=dev) for k in ("actor", "critic")}
        self.nets = {"actor": _NetBufs(agent.actor, dev), "target_actor": _NetBufs(agent.target_actor, dev),
                     "q1": _NetBufs(agent.critic.q1, dev), "q2": _NetBufs(agent.critic.q2, dev),
                     "tq1": _NetBufs(agent.target_critic.q1, dev), "tq2": _NetBufs(agent.target_critic.q2, dev)}
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
        self.buf = {"x0": z(B, XP), "x0a": z(B, XP), "td": z(B), "noise": z(B, 4), "loss_c": z(G), "loss_a": z(G)}
        for k in ("h1", "dz1", "dz2"):
            self.buf[k] = [z(B, 256), z(B, 256)]
            self.buf[k + "a"] = z(B, 256)
        self.buf["h2a"] = z(B, 256)
        for k in ("db1", "db2", "dw3"):
            self.buf["p_" + k] = [z(G, 256), z(G, 256)]
        self.buf["p_db3"] = [z(G), z(G)]
        self.buf["pa_db1"], self.buf["pa_db2"] = z(G, 256), z(G, 256)
        self.buf["pa_dw3"], self.buf["pa_db3"] = z(G, 4, 256), z(G, 4)
        self.buf["s_w2"] = [z(C, 256, 256), z(C, 256, 256)]
        self.buf["s_w1"] = [z(C1, 256, XP), z(C1, 256, XP)]
        self.buf["s_b2"], self.buf["s_b1"] = [z(C, 256), z(C, 256)], [z(C1, 256), z(C1, 256)]
        self.buf["sa_w2"], self.buf["sa_w1"] = z(CA, 256, 256), z(C1, 256, XP)
        self.buf["sa_b2"], self.buf["sa_b1"] = z(CA, 256), z(C1, 256)
        self.idx = torch.zeros(B, dtype=torch.int64, device=dev)
        self.sample_counter = torch.zeros((), dtype=torch.int64, device=dev)
        sio = SampleIO()
        sio.batch = B
        sio.seed = (int(agent.seed if seed is None else seed) * 0x9E3779B97F4A7C15 + 0x4C4541524E) % (1 << 64)
        sio.counter, sio.size, sio.idx, sio.noise = (_p(self.sample_counter), _p(ring.size_t), _p(self.idx),
                                                     _p(self.buf["noise"]))
        sio.scale, sio.clip = c.target_action_noise_scale, c.target_action_noise_clip
        self.sio = sio
        self.iw = z(B) if ring.prioritized else None
        # a DevicePrioritizedRing (hockey_amd.td3) samples, weighs and writes back through the hkl_per_* kernels:
        # psio draws from the learner's Philox stream, psio_u from torch uniforms (rng="torch": noise by torch too)
        self.psio = self.psio_u = self.puio = None
        if getattr(ring, "device_sampler", False):
            self._u = torch.zeros(B, dtype=torch.float64, device=dev)
            self.psio = PerSampleIO(ring.per, B, sio.seed, sio.counter, None, sio.idx, sio.noise, sio.scale, sio.clip,
                                    _p(self.iw), ring.beta)
            self.psio_u = PerSampleIO(ring.per, B, 0, None, _p(self._u), sio.idx, None, 0.0, 0.0, _p(self.iw),
                                      ring.beta)
            self.puio = PerUpdateIO(ring.per, B, sio.idx, _p(self.buf["td"]))
        low = agent.critic.action_low.float().cpu().tolist()
        rng = agent.critic.action_range.float().cpu().tolist()
        self._build_io(low, rng, G, C, C1, CA)
        # Adam adds each step's loss into a device accumulator: a private one until the caller sets its own, so
        # that an update never runs with the loss pointers unset
        self.set_loss_accumulator(torch.zeros(4, dtype=torch.float64, device=dev))
        st = self._stream()
        for group in (("actor", "target_actor"), ("q1", "q2"), ("tq1", "tq2")):
            self._pack([self.nets[k] for k in group], None, st)
        agent._fused_learner = self  # TD3.update / TD3.load now fail loudly (TD3._no_fused)

    # ------------------------------------------------------------------ structs (fixed pointers)
    def _build_io(self, low, rng, G, C, C1, CA):
        b, n = self.buf, self.nets
        cio = CriticIO()
        cio.batch, cio.idx = self.B, _p(self.idx)
        r = self.ring
        cio.ring_s, cio.ring_a, cio.ring_r, cio.ring_s2, cio.ring_d = _p(r.s), _p(r.a), _p(r.r), _p(r.s2), _p(r.d)
        cio.noise, cio.iw = _p(b["noise"]), _p(self.iw)
        cio.target_actor = n["target_actor"].net
        cio.target_q[0], cio.target_q[1] = n["tq1"].net, n["tq2"].net
        cio.q[0], cio.q[1] = n["q1"].net, n["q2"].net
        cio.gamma = self.cfg.gamma
        for i in range(4):
            cio.act_low[i], cio.act_range[i] = low[i], rng[i]
        cio.x0 = _p(b["x0"])
        for k in range(2):
            cio.h1[k], cio.dz1[k], cio.dz2[k] = _p(b["h1"][k]), _p(b["dz1"][k]), _p(b["dz2"][k])
            cio.p_db1[k], cio.p_db2[k] = _p(b["p_db1"][k]), _p(b["p_db2"][k])
            cio.p_dw3[k], cio.p_db3[k] = _p(b["p_dw3"][k]), _p(b["p_db3"][k])
        cio.p_loss, cio.td = _p(b["loss_c"]), _p(b["td"])
        cio.sample_counter = _p(self.sample_counter)
        self.cio = cio

        aio = ActorIO()
        aio.batch, aio.idx, aio.ring_s = self.B, _p(self.idx), _p(r.s)
        aio.actor, aio.q1 = n["actor"].net, n["q1"].net
        for i in range(4):
            aio.act_low[i], aio.act_range[i] = low[i], rng[i]
        aio.x0, aio.h1, aio.h2, aio.dz1, aio.dz2 = (_p(b["x0a"]), _p(b["h1a"]), _p(b["h2a"]), _p(b["dz1a"]),
                                                    _p(b["dz2a"]))
        aio.p_db1, aio.p_db2, aio.p_dw3, aio.p_db3 = _p(b["pa_db1"]), _p(b["pa_db2"]), _p(b["pa_dw3"]), _p(b["pa_db3"])
        aio.p_loss = _p(b["loss_a"])
        self.aio = aio
        # Adam segments: torch parameter order of each network (fc1.w, fc1.b, fc2.w, fc2.b, fc3.w, fc3.b)
        self.adam = {}
        for name, nets, lr, wd, tau in (
                ("critic", [("q1", 0, "tq1"), ("q2", 1, "tq2")], self.cfg.lr_q, self.cfg.wd_q, self.cfg.tau_critic),
                ("actor", [("actor", None, "target_actor")], self.cfg.lr_pol, self.cfg.wd_pol, self.cfg.tau_actor)):
            io = AdamIO()
            segs = []
            flat, m, v = self.flat[name], self.m[name], self.v[name]
            tflat = self.flat["target_" + name]
            off = 0
            for key, k, tkey in nets:
                f1, f2, f3 = _mlp_layers(n[key].m)
                t1, t2, t3 = _mlp_layers(n[tkey].m)
                tparams = (t1.weight, t1.bias, t2.weight, t2.bias, t3.weight, t3.bias)
                if k is None:
                    srcs = [(b["sa_w1"], XP, C1, 256 * XP), (b["sa_b1"], 256, C1, 256), (b["sa_w2"], 256, CA, 65536),
                            (b["sa_b2"], 256, CA, 256), (b["pa_dw3"], 256, G, 1024), (b["pa_db3"], 4, G, 4)]
                else:
                    srcs = [(b["s_w1"][k], XP, C1, 256 * XP), (b["s_b1"][k], 256, C1, 256), (b["s_w2"][k], 256, C, 65536),
                            (b["s_b2"][k], 256, C, 256), (b["p_dw3"][k], 256, G, 256), (b["p_db3"][k], 1, G, 1)]
                for p, tp, (src, ld, chunks, stride) in zip((f1.weight, f1.bias, f2.weight, f2.bias, f3.weight,
                                                             f3.bias), tparams, srcs):
                    rows, cols = (p.shape[0], p.shape[1]) if p.dim() == 2 else (1, p.shape[0])
                    assert p.data_ptr() == flat.data_ptr() + off * 4, "parameters not in the flat buffer's order"
                    assert tp.data_ptr() == tflat.data_ptr() + off * 4 and tp.shape == p.shape, "target layout differs"
                    segs.append(Seg(_p(p), ctypes.c_void_p(m.data_ptr() + off * 4),
                                    ctypes.c_void_p(v.data_ptr() + off * 4), _p(src), rows, cols, ld, chunks, stride,
                                    _p(tp)))
                    off += p.numel()
            assert off == flat.numel()
            for i, s in enumerate(segs):
                io.seg[i] = s
            io.n_seg = len(segs)
            io.lr, io.beta1, io.beta2, io.eps, io.wd = lr, 0.9, 0.999, 1e-6, wd
            io.step = _p(self.step[name])
            io.loss_src = _p(b["loss_c"] if name == "critic" else b["loss_a"])
            io.loss_chunks = G
            io.loss_scale = (0.5 if name == "critic" else 1.0) / self.B
            # soft_update folded into the Adam launch (set per call: the critic's only on actor updates)
            io.polyak, io.polyak_rho, io.polyak_tau = 0, 1.0 - tau, tau
            self.adam[name] = io
        # weight-gradient jobs (one launch per k width): critics' dW2 / dW1 (+ b2 / b1), actor's
        J = lambda dz, x, sl, bs: WgJob(_p(dz), _p(x), _p(sl), _p(bs))  # noqa: E731
        self.wg = {"c256": (WgJob * 2)(*[J(b["dz2"][k], b["h1"][k], b["s_w2"][k], b["s_b2"][k]) for k in range(2)]),
                   "c32": (WgJob * 2)(*[J(b["dz1"][k], b["x0"], b["s_w1"][k], b["s_b1"][k]) for k in range(2)]),
                   "a256": (WgJob * 1)(J(b["dz2a"], b["h1a"], b["sa_w2"], b["sa_b2"])),
                   "a32": (WgJob * 1)(J(b["dz1a"], b["x0a"], b["sa_w1"], b["sa_b1"]))}

    def _stream(self):
        return stream_ptr(self.agent.device)

    def _pack(self, bufs, step, st):
        arr = (Net * len(bufs))(*[x.net for x in bufs])
        _check(self.L.hkl_pack(arr, len(bufs), _p(step), st), "hkl_pack")

    def set_loss_accumulator(self, acc):
        """acc: float64 [4] = (sum critic loss, sum actor loss, critic updates, actor updates) on the device."""
        base = acc.data_ptr()
        self.adam["critic"].loss_sum, self.adam["critic"].loss_count = base, base + 16
        self.adam["actor"].loss_sum, self.adam["actor"].loss_count = base + 8, base + 24
        self._acc = acc

    # ------------------------------------------------------------------ one update
    def update(self, train_actor, idx=None, noise=None):
        """learner.update on a batch sampled from the ring: critic step, then (train_actor) the actor step and the
        Polyak averaging of both targets.  The batch's slots and target noise come from the device Philox stream
        (rng="device": one kernel), or from torch's generator in the eager learner's order (rng="torch": the slots
        via ring.sample_indices, then N(0, scale) [B, 4]), or (tests) from idx / noise: the slots and the UNCLIPPED
        N(0, scale) noise.  On a DevicePrioritizedRing one hkl_per_sample draws the prioritized slots (from the Philox
        stream, or under rng="torch" from torch.rand(B, float64)) and writes the importance weights, and one
        hkl_per_update writes the TD errors back; with idx given, hkl_per_weights weighs those slots."""
        L, st, b = self.L, self._stream(), self.buf
        c = self.cfg
        prioritized = self.ring.prioritized
        dev_per = self.psio is not None
        iw_done = False
        if idx is None and noise is None and self.rng == "device" and (dev_per or not prioritized):
            if dev_per:  # slots, target noise and importance weights in one call
                _check(L.hkl_per_sample(ctypes.byref(self.psio), st), "hkl_per_sample")
                iw_done = True
            else:
                _check(L.hkl_sample(ctypes.byref(self.sio), st), "hkl_sample")
            i = self.idx
        else:
            if idx is None and dev_per:  # torch's generator in the eager order: the slots' uniforms, then the noise
                self._u.copy_(torch.rand(self.B, device=self.agent.device, dtype=torch.float64))
                _check(L.hkl_per_sample(ctypes.byref(self.psio_u), st), "hkl_per_sample")
                i, iw_done = self.idx, True
            else:
                i = self.ring.sample_indices(self.B) if idx is None else idx
                self.idx.copy_(i)
            if noise is None:
                noise = torch.randn((self.B, 4), device=self.agent.device) * c.target_action_noise_scale
            b["noise"].copy_(torch.clamp(noise, -c.target_action_noise_clip, c.target_action_noise_clip))
        if dev_per and not iw_done:  # slots given by the caller
            _check(L.hkl_per_weights(ctypes.byref(self.psio), st), "hkl_per_weights")
        elif self.iw is not None and not iw_done:
            wb = self.ring.w[i]
            p = wb / wb.sum()
            iw = (1.0 / (p * self.ring.size_t)) ** self.ring.beta
            self.iw.copy_(iw / iw.max())
        _check(L.hkl_critic_step(ctypes.byref(self.cio), st), "hkl_critic_step")
        _check(L.hkl_wgrad_pair(self.wg["c256"], 2, self.wg["c32"], 2, self.B, st), "hkl_wgrad_pair")
        # on an actor update the critic's soft_update runs here, with its Adam step: nothing later in the update
        # reads the target critic or changes the critic, so the values are those of soft_update at the end
        self.adam["critic"].polyak = 1 if train_actor else 0
        _check(L.hkl_adam(ctypes.byref(self.adam["critic"]), st), "hkl_adam")
        self._pack([self.nets["q1"], self.nets["q2"]], self.step["critic"], st)
        if dev_per:
            self.ring.last = self.idx
            _check(L.hkl_per_update(ctypes.byref(self.puio), st), "hkl_per_update")
        elif self.ring.prioritized:
            self.ring.last = i
            self.ring.update_priorities(b["td"])
        if not train_actor:
            return
        _check(L.hkl_actor_step(ctypes.byref(self.aio), st), "hkl_actor_step")
        _check(L.hkl_wgrad_pair(self.wg["a256"], 1, self.wg["a32"], 1, self.B, st), "hkl_wgrad_pair")
        self.adam["actor"].polyak = 1  # the actor's soft_update with its Adam step
        _check(L.hkl_adam(ctypes.byref(self.adam["actor"]), st), "hkl_adam")
        self._pack([self.nets["actor"], self.nets["target_actor"], self.nets["tq1"], self.nets["tq2"]],
                   self.step["actor"], st)


def update_flops(batch, h=256, n_obs=18, n_act=4, policy_freq=2):
    """Algorithmic fp32 FLOPs of one learner update at ``batch`` (2 per multiply-add; averaged over the delayed actor
    update), counted from the layer shapes of rl/td3/networks.py: an MLP n_in -> h -> h -> n_out costs
    F(n_in, n_out) = n_in h + h h + h n_out MACs per sample forward; a backward to the first layer's input-side
    gradients costs h n_out + h h (data) and every weight gradient its forward MACs again.
      critic step: target actor + 2 target critics forward, 2 critics forward, 2 critics backward (data: W3^T, W2^T;
                   weights: dW1, dW2, dW3);
      actor step (every policy_freq-th): actor forward, Q1 forward, Q1 backward to its input (W3^T, W2^T, W1^T
                   action columns), actor backward (data and weights)."""
    fa, fc = n_obs * h + h * h + h * n_act, (n_obs + n_act) * h + h * h + h
    critic = fa + 2 * fc + 2 * fc + 2 * ((h + h * h) + fc)
    actor = fa + fc + ((h + h * h) + h * n_act) + ((h * n_act + h * h) + fa)
    return 2.0 * batch * (critic + actor / policy_freq)
