"""Each kernel of the fused TD3 learner (csrc/hk_learner.hip) against the float64 references of tests/learner_ref.py.

tests/test_gpu_learner.py sees the kernels' gradients only after Adam, which normalises a gradient's scale away; here
every gradient and every per-row intermediate is compared directly, at the smallest legal batches (256: one split-K
chunk; 768: three 256-sample chunks, the critics' dW2 falling back from 512; 1024: two 512-sample critic chunks and
four 256-sample actor chunks), with and without importance weights, at the identity action map and at a non-identity
one.  hkl_adam, hkl_polyak and hkl_sample are launched on their own.  Every output buffer is filled with NaN before a
launch, so an element the kernel leaves unwritten fails its comparison.

Tolerance.  err(T) = max|T_kernel - T_64| / max|T_64|.  The same expressions are evaluated by torch in float32 on the
GPU (learner_ref's functions at dtype float32: the eager TD3 path's operations, tests/test_learner_ref.py; and
torch.optim.Adam in float32 for hkl_adam), which gives err_fp32_eager(T); the bound is
err(T) <= max(4 err_fp32_eager(T), 4 * 2^-24) (learner_ref.bound).  Nothing is fitted to the kernels' own error.
X0 is a copy plus one unscale: the state columns are compared bit for bit and the padding must be exactly 0; an
action column may differ from the float64 value by 2 ulp, an ulp being float32's spacing at the magnitude of the
value before unscale's final `- 1` (never below 1): the subtraction cancels, so it keeps the absolute error of the
chain's larger intermediates, not a relative one.  hkl_sample's slots are exact; its noise is bounded the same way
from a float32 numpy evaluation of the same formula.

Measured on an MI355X: per tensor the largest err over the parametrised cases with err_fp32_eager of that case,
and the largest err / bound over the cases (the action columns of X0 were at most 0.33 ulp off):

    tensor                 err      err_fp32_eager  err / bound  comparisons
    td                     1.24e-07 1.09e-07        0.28         12
    critic.h1              4.25e-07 3.47e-07        0.34         24
    critic.dz2             9.25e-07 8.09e-07        0.37         24
    critic.dz1             7.85e-07 9.57e-07        0.29         24
    critic.d_fc1.weight    6.41e-07 6.41e-07        0.37         24
    critic.d_fc1.bias      7.50e-07 6.80e-07        0.35         24
    critic.d_fc2.weight    8.92e-07 1.45e-06        0.29         24
    critic.d_fc2.bias      7.85e-07 5.48e-07        0.36         24
    critic.d_fc3.weight    3.88e-07 1.10e-06        0.26         24
    critic.d_fc3.bias      1.86e-06 9.20e-07        0.83         24
    critic.loss            2.99e-08 8.74e-08        0.11         12
    actor.h1               3.30e-07 3.85e-07        0.27         6
    actor.h2               8.53e-07 7.92e-07        0.27         6
    actor.dz2              6.94e-07 6.27e-07        0.29         6
    actor.dz1              9.84e-07 9.09e-07        0.27         6
    actor.d_fc1.weight     6.66e-07 6.13e-07        0.27         6
    actor.d_fc1.bias       1.41e-07 1.41e-07        0.29         6
    actor.d_fc2.weight     7.50e-07 5.79e-07        0.32         6
    actor.d_fc2.bias       9.18e-08 7.15e-08        0.32         6
    actor.d_fc3.weight     2.62e-07 2.85e-07        0.23         6
    actor.d_fc3.bias       5.43e-08 1.40e-07        0.20         6
    actor.loss             1.58e-07 1.78e-07        0.31         6
    adam.p                 2.58e-06 2.89e-06        0.35         84
    adam.m                 1.57e-07 1.21e-07        0.35         84
    adam.v                 3.31e-07 2.55e-07        0.48         84
    adam.loss_sum          1.01e-07 2.53e-09        0.42         84
    adam.target            1.99e-07 1.99e-07        0.25         42
    polyak.target          6.67e-08 6.67e-08        0.25         1
    sample.noise           1.31e-06 1.31e-06        0.25         8

Two tensors missed the bound when these tests were first run, and the kernels were changed, not the bound:
* the bias gradients d_fc1.bias / d_fc2.bias (up to 1.46 x the bound): hkl_wgrad's column sum of DZ ran one float32
  sum over a chunk's 256 or 512 signed terms; it now sums each 32-row sub-chunk as four interleaved partial sums;
* adam.v (54 x the bound, 1.3e-5 on every element) and adam.m (1.17 x): the kernel took 1 - beta in float32 from
  the float32 beta (1.0f - 0.999f = 0.00099998713); hkl_adam_io now carries the betas as doubles and the kernel
  rounds 1 - beta from the double, as torch does from its Python scalars.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import learner_ref as R  # noqa: E402
from hockey_amd.td3 import TD3, PrioritizedRing, ReplayRing, TD3Config  # noqa: E402

DEV = "cuda:0"
BATCHES = [b for b, _ in R.GPU_CASES]
SEED = dict(R.GPU_CASES)


# ---------------------------------------------------------------------------------------------------- fixtures
@functools.lru_cache(maxsize=None)
def _case(B, per, aff):
    """The case and its references, computed once: float64 on the CPU and torch's float32 on the GPU."""
    c = R.make_case(B, SEED[B], per, aff)
    args = (c["nets"], c["ring"], c["idx"], c["noise"], c["iw"], c["gamma"], c["act_low"], c["act_range"])
    aargs = (c["nets"], c["ring"], c["idx"], c["act_low"], c["act_range"])
    return {"case": c, "critic64": R.critic_reference(*args),
            "critic32": R.critic_reference(*args, dtype=torch.float32, device=DEV),
            "actor64": R.actor_reference(*aargs),
            "actor32": R.actor_reference(*aargs, dtype=torch.float32, device=DEV)}


def _learner(c):
    """A FusedLearner on the case's networks and ring, its buffers holding the case's slots, noise and weights."""
    from hockey_amd.learner_hip import FusedLearner

    agent = TD3(TD3Config(gamma=c["gamma"]), device=DEV, seed=0)
    n = c["nets"]
    agent.actor.load_state_dict(n["actor"])
    agent.target_actor.load_state_dict(n["target_actor"])
    for tw, k1, k2 in ((agent.critic, "q1", "q2"), (agent.target_critic, "tq1", "tq2")):
        tw.q1.load_state_dict(n[k1])
        tw.q2.load_state_dict(n[k2])
    cap = c["ring"]["s"].shape[0]
    ring = PrioritizedRing(cap, device=DEV) if c["per"] else ReplayRing(cap, device=DEV)
    ring.push(*(c["ring"][k].to(DEV) for k in ("s", "a", "r", "s2", "d")))
    fl = FusedLearner(agent, ring, c["B"], rng="torch")
    for io in (fl.cio, fl.aio):
        for i in range(4):
            io.act_low[i], io.act_range[i] = c["act_low"][i], c["act_range"][i]
    fl.idx.copy_(c["idx"])
    fl.buf["noise"].copy_(c["noise"])
    if c["per"]:
        fl.iw.copy_(c["iw"])
    torch.cuda.synchronize()
    return fl


CRITIC_OUT = ("x0", "td", "loss_c", "h1", "dz1", "dz2", "p_dw3", "p_db3", "s_w2", "s_w1", "s_b2", "s_b1")
ACTOR_OUT = ("x0a", "h1a", "h2a", "dz1a", "dz2a", "pa_dw3", "pa_db3", "loss_a", "sa_w2", "sa_w1", "sa_b2", "sa_b1")


def _tensors(fl, keys):
    out = []
    for k in keys:
        v = fl.buf[k]
        out += list(v) if isinstance(v, list) else [v]
    return out


def _launch(fl, which):
    """NaN into every output buffer, then the step kernel and its weight-gradient launch; returns copies."""
    from hockey_amd.learner_hip import _check

    keys = CRITIC_OUT if which == "critic" else ACTOR_OUT
    for t in _tensors(fl, keys):
        t.fill_(float("nan"))
    st, L, B = fl._stream(), fl.L, fl.B
    if which == "critic":
        _check(L.hkl_critic_step(ctypes.byref(fl.cio), st), "hkl_critic_step")
        _check(L.hkl_wgrad_pair(fl.wg["c256"], 2, fl.wg["c32"], 2, B, st), "hkl_wgrad_pair")
    else:
        _check(L.hkl_actor_step(ctypes.byref(fl.aio), st), "hkl_actor_step")
        _check(L.hkl_wgrad_pair(fl.wg["a256"], 1, fl.wg["a32"], 1, B, st), "hkl_wgrad_pair")
    torch.cuda.synchronize()
    return [t.clone() for t in _tensors(fl, keys)]


class _Report:
    """Collects err / err_fp32_eager per tensor, prints each figure, and fails at the end with every miss."""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def check(self, name, got, ref64, ref32):
        err, eager = R.rel_err(got, ref64), R.rel_err(ref32, ref64)
        print(f"ERR {self.tag} {name} {err:.3e} {eager:.3e}")
        if not err <= R.bound(eager):  # NaN (an unwritten element) fails
            self.bad.append((name, err, eager, R.bound(eager)))

    def exact(self, name, ok):
        if not ok:
            self.bad.append((name, "not exact"))

    def done(self):
        assert not self.bad, (self.tag, self.bad)


def _check_x0(rep, x0, ref64, n_state, n_in):
    """state columns bit for bit (the ring's float32 values), action columns within 2 ulp, padding exactly 0."""
    x0, ref = x0.cpu(), ref64.cpu()
    rep.exact("x0 state", torch.equal(x0[:, :n_state], ref[:, :n_state].float()))
    rep.exact("x0 pad", bool((x0[:, n_in:] == 0).all()))
    if n_in > n_state:
        a, want = x0[:, n_state:n_in].double(), ref[:, n_state:n_in]
        ulp = torch.from_numpy(np.spacing(np.maximum((want + 1.0).abs().numpy(), 1.0).astype(np.float32))).double()
        worst = float(((a - want).abs() / ulp).max())
        print(f"ERR {rep.tag} x0_action_ulp {worst:.3f} -")
        rep.exact("x0 action within 2 ulp", worst <= 2.0)


# ---------------------------------------------------------------------------------------------------- critic step
@pytest.mark.parametrize("aff", [False, True], ids=["identity", "affine"])
@pytest.mark.parametrize("per", [False, True], ids=["uniform", "per"])
@pytest.mark.parametrize("B", BATCHES)
def test_critic_step_and_weight_gradients_against_float64(B, per, aff):
    k = _case(B, per, aff)
    c, r64, r32 = k["case"], k["critic64"], k["critic32"]
    fl = _learner(c)
    _launch(fl, "critic")
    b = fl.buf
    rep = _Report(f"critic b{B} {'per' if per else 'uniform'} {'affine' if aff else 'identity'}")
    _check_x0(rep, b["x0"], r64["x0"], 18, 22)
    rep.check("td", b["td"], r64["td"], r32["td"])
    for q in range(2):
        g64, g32 = r64["grads"][q], r32["grads"][q]
        for name, got in (("h1", b["h1"][q]), ("dz2", b["dz2"][q]), ("dz1", b["dz1"][q])):
            rep.check(f"critic.{name}", got, r64[name][q], r32[name][q])
        w1 = b["s_w1"][q].double().sum(0)
        rep.exact("dW1 pad", bool((b["s_w1"][q][:, :, 22:] == 0).all()))
        for name, got in (("fc1.weight", w1[:, :22]), ("fc1.bias", b["s_b1"][q].double().sum(0)),
                          ("fc2.weight", b["s_w2"][q].double().sum(0)), ("fc2.bias", b["s_b2"][q].double().sum(0)),
                          ("fc3.weight", b["p_dw3"][q].double().sum(0)[None]),
                          ("fc3.bias", b["p_db3"][q].double().sum()[None])):
            rep.check(f"critic.d_{name}", got, g64[name], g32[name])
    rep.check("critic.loss", b["loss_c"].double().sum() * 0.5 / B, r64["loss"], r32["loss"])
    rep.done()


# ---------------------------------------------------------------------------------------------------- actor step
@pytest.mark.parametrize("aff", [False, True], ids=["identity", "affine"])
@pytest.mark.parametrize("B", BATCHES)
def test_actor_step_and_weight_gradients_against_float64(B, aff):
    k = _case(B, False, aff)
    c, r64, r32 = k["case"], k["actor64"], k["actor32"]
    fl = _learner(c)
    _launch(fl, "actor")
    b = fl.buf
    rep = _Report(f"actor b{B} {'affine' if aff else 'identity'}")
    _check_x0(rep, b["x0a"], r64["x0"], 18, 18)
    for name in ("h1", "h2", "dz2", "dz1"):
        rep.check(f"actor.{name}", b[name + "a"], r64[name], r32[name])
    rep.exact("dW1 pad", bool((b["sa_w1"][:, :, 18:] == 0).all()))
    g64, g32 = r64["grads"], r32["grads"]
    for name, got in (("fc1.weight", b["sa_w1"].double().sum(0)[:, :18]), ("fc1.bias", b["sa_b1"].double().sum(0)),
                      ("fc2.weight", b["sa_w2"].double().sum(0)), ("fc2.bias", b["sa_b2"].double().sum(0)),
                      ("fc3.weight", b["pa_dw3"].double().sum(0)), ("fc3.bias", b["pa_db3"].double().sum(0))):
        rep.check(f"actor.d_{name}", got, g64[name], g32[name])
    rep.check("actor.loss", b["loss_a"].double().sum() / B, r64["loss"], r32["loss"])
    rep.done()


# ---------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("B", BATCHES)
def test_step_kernels_are_bit_deterministic(B):
    """Fixed-order reductions, no atomics: the same launches on identical inputs write identical bits (what
    test_fused_graph_replay_equals_fused_eager leans on)."""
    fl = _learner(_case(B, True, True)["case"])
    for which in ("critic", "actor"):
        first, second = _launch(fl, which), _launch(fl, which)
        for i, (x, y) in enumerate(zip(first, second)):
            assert not bool(torch.isnan(x).any()), (which, i)
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (which, i)


# ---------------------------------------------------------------------------------------------------- hkl_adam
# (rows, cols, ld) of the 12 segments of one call, shaped like the real ones: first-layer weights read from a slab
# padded to 32 columns, biases, a [4, 256] head with stride 1024, [1, 4], [1, 1]; 38 149 elements in all, which
# leaves 5 in the last 256-thread block
ADAM_SEGS = ((256, 22, 32), (1, 256, 256), (48, 256, 256), (1, 256, 256), (4, 256, 256), (1, 4, 4),
             (256, 22, 32), (1, 256, 256), (48, 256, 256), (1, 256, 256), (1, 256, 256), (1, 1, 1))
LR, B1, B2, EPS = 4e-4, 0.9, 0.999, 1e-6


@pytest.mark.parametrize("polyak", [0, 1])
@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("chunks", [1, 15, 16, 17, 47, 64, 125])
def test_adam_alone_against_float64(chunks, wd, polyak):
    """Three consecutive hkl_adam calls (the device step bumped by hand) on synthetic slabs: every reduction loop (64,
    32, 16 chunks at a time and the remainder: 125 = 64 + 32 + 16 + 13), ld != cols (the slab's padding columns hold
    NaN: reading one poisons the parameter), a last block that is not full, gradients over six decades with exact
    zeros, weight decay, the folded Polyak averaging and the loss accumulator."""
    from hockey_amd import learner_hip as LH

    n_tot = sum(r * c for r, c, _ in ADAM_SEGS)
    assert n_tot % 256 != 0 and len(ADAM_SEGS) == LH.MAX_SEG
    g = torch.Generator(device=DEV).manual_seed(1000 * chunks + 10 * polyak + (wd > 0))
    rand = lambda *s: torch.rand(*s, device=DEV, generator=g)  # noqa: E731
    randn = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    p, tgt = randn(n_tot) * 0.1, randn(n_tot) * 0.1
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step = torch.zeros((), dtype=torch.int64, device=DEV)
    acc = torch.zeros(2, dtype=torch.float64, device=DEV)
    zero = rand(n_tot) < 0.2  # elements whose gradient is exactly 0 in every chunk of every call
    n_loss = 3 * chunks - 1
    slabs = [torch.full((chunks, r, ld), float("nan"), device=DEV) for r, _, ld in ADAM_SEGS]
    loss_src = torch.zeros(n_loss, device=DEV)
    io = LH.AdamIO()
    off = 0
    for i, ((r, c, ld), slab) in enumerate(zip(ADAM_SEGS, slabs)):
        at = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * off)  # noqa: E731
        io.seg[i] = LH.Seg(at(p), at(m), at(v), LH._p(slab), r, c, ld, chunks, r * ld, at(tgt))
        off += r * c
    io.n_seg = len(ADAM_SEGS)
    io.lr, io.beta1, io.beta2, io.eps, io.wd = LR, B1, B2, EPS, wd
    io.step, io.loss_src, io.loss_chunks, io.loss_scale = LH._p(step), LH._p(loss_src), n_loss, 0.5 / 777
    io.loss_sum, io.loss_count = acc.data_ptr(), acc.data_ptr() + 8
    io.polyak, io.polyak_rho, io.polyak_tau = polyak, 1.0 - 0.005, 0.005
    rho, tau, scale = float(io.polyak_rho), float(io.polyak_tau), float(io.loss_scale)  # as the kernel reads them

    p0, t0 = p.clone(), tgt.clone()
    r_p, r_m, r_v, r_t, r_loss = p.double().cpu(), m.double().cpu(), v.double().cpu(), tgt.double().cpu(), 0.0
    e_p = p.clone().requires_grad_(True)  # torch's float32: optim.Adam on the float32 sum of the same slabs
    e_t, e_loss = tgt.clone(), 0.0
    opt = torch.optim.Adam([e_p], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd)
    rep = _Report(f"adam chunks{chunks} wd{wd} polyak{polyak}")
    for call in range(3):
        g64, g32, o = [], [], 0
        for (r, c, ld), slab in zip(ADAM_SEGS, slabs):
            val = randn(chunks, r, c) * 10.0 ** (-6.0 * rand(chunks, r, c))
            val[:, zero[o:o + r * c].view(r, c)] = 0.0
            slab[:, :, :c] = val
            g64.append(val.double().sum(0).reshape(-1))
            g32.append(val.sum(0).reshape(-1))
            o += r * c
        loss_src.copy_(rand(n_loss) + 0.1)
        LH._check(LH.lib().hkl_adam(ctypes.byref(io), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                  "hkl_adam")
        torch.cuda.synchronize()
        r_p, r_m, r_v = R.adam_reference(r_p, r_m, r_v, torch.cat(g64), call, LR, B1, B2, EPS, wd)
        r_loss += float(loss_src.double().sum()) * scale
        e_p.grad = torch.cat(g32)
        opt.step()
        e_loss += float(loss_src.sum() * scale)  # a float32 product, like the kernel's
        if polyak:
            r_t = R.polyak_reference(r_t, r_p, rho, tau)
            with torch.no_grad():
                e_t.mul_(rho).add_(e_p, alpha=tau)
        step += 1
        st = opt.state[e_p]
        rep.check(f"adam.p[{call}]", p, r_p, e_p)
        rep.check(f"adam.m[{call}]", m, r_m, st["exp_avg"])
        rep.check(f"adam.v[{call}]", v, r_v, st["exp_avg_sq"])
        if polyak:
            rep.check(f"adam.target[{call}]", tgt, r_t, e_t)
        rep.check(f"adam.loss_sum[{call}]", acc[0], torch.tensor(r_loss, dtype=torch.float64),
                  torch.tensor(e_loss, dtype=torch.float64))
        rep.exact("loss_count", float(acc[1]) == call + 1.0)
    if not polyak:
        rep.exact("target untouched", torch.equal(tgt, t0))
    if wd == 0.0:  # g == 0: m = v = 0 and the parameter unchanged
        rep.exact("zero gradient", bool((m[zero] == 0).all()) and bool((v[zero] == 0).all()) and
                  torch.equal(p[zero], p0[zero]))
    rep.exact("finite", bool(torch.isfinite(torch.cat([p, m, v, tgt])).all()))
    rep.done()


def test_polyak_alone_against_float64():
    """hkl_polyak at n = 1000 (the last block is not full): elements past n stay as they were."""
    from hockey_amd import learner_hip as LH

    g = torch.Generator(device=DEV).manual_seed(4)
    t, p = torch.randn(1024, device=DEV, generator=g), torch.randn(1024, device=DEV, generator=g)
    t0 = t.clone()
    rho, tau = float(ctypes.c_float(1.0 - 0.005).value), float(ctypes.c_float(0.005).value)
    LH._check(LH.lib().hkl_polyak(LH._p(t), LH._p(p), 1000, rho, tau,
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "hkl_polyak")
    torch.cuda.synchronize()
    rep = _Report("polyak n1000")
    rep.check("polyak.target", t[:1000], R.polyak_reference(t0[:1000], p[:1000], rho, tau),
              t0[:1000] * rho + tau * p[:1000])
    rep.exact("past n", torch.equal(t[1000:], t0[1000:]))
    rep.done()


# ---------------------------------------------------------------------------------------------------- hkl_sample
def _sample(fl, size, ctr):
    from hockey_amd.learner_hip import _check

    fl.ring.size_t.fill_(size)  # sampling reads only the fill level
    fl.sample_counter.fill_(ctr)
    fl.idx.fill_(-1)
    fl.buf["noise"].fill_(float("nan"))
    _check(fl.L.hkl_sample(ctypes.byref(fl.sio), fl._stream()), "hkl_sample")
    torch.cuda.synchronize()
    return fl.idx.cpu().numpy().copy(), fl.buf["noise"].cpu().numpy().copy()


@pytest.mark.parametrize("ctr", [0, (1 << 32) + 7], ids=["ctr0", "ctr_hi"])
@pytest.mark.parametrize("size", [1, 1000, 2 ** 24 + 1, 2 ** 33 + 5])
def test_sample_matches_the_philox_reference(size, ctr):
    """hkl_sample's slots are floor(u * size) of the 53-bit Philox4x32-10 u (counter words (e lo, e hi, ctr lo,
    ctr hi)), exactly; its noise is the Box-Muller reference within the float32 margin, never past the clip; and
    hkl_sample does not advance the counter."""
    B = 768
    fl = _learner(_case(B, False, False)["case"])
    seed, scale, clip = int(fl.sio.seed), float(fl.sio.scale), float(fl.sio.clip)
    idx, noise = _sample(fl, size, ctr)
    assert int(fl.sample_counter) == ctr
    want = R.sample_slots(seed, B, ctr, size)
    assert np.array_equal(idx, want), int(np.argmax(idx != want))
    n64, n32 = R.sample_noise(seed, B, ctr, scale, clip), R.sample_noise(seed, B, ctr, scale, clip, np.float32)
    rep = _Report(f"sample size{size} ctr{ctr}")
    rep.check("sample.noise", torch.from_numpy(noise), torch.from_numpy(n64), torch.from_numpy(n32))
    rep.exact("clip", float(np.abs(noise).max()) <= clip and float(np.abs(noise).max()) == clip)
    rep.done()


def test_sample_counter_is_advanced_by_the_critic_step():
    from hockey_amd.learner_hip import _check

    B, ctr, size = 768, 41, 1000  # the ring's real fill level: the critic step reads the sampled slots
    fl = _learner(_case(B, False, False)["case"])
    seed = int(fl.sio.seed)
    idx, _ = _sample(fl, size, ctr)
    assert np.array_equal(idx, R.sample_slots(seed, B, ctr, size)) and int(fl.sample_counter) == ctr
    _check(fl.L.hkl_critic_step(ctypes.byref(fl.cio), fl._stream()), "hkl_critic_step")
    torch.cuda.synchronize()
    assert int(fl.sample_counter) == ctr + 1
    _check(fl.L.hkl_sample(ctypes.byref(fl.sio), fl._stream()), "hkl_sample")
    torch.cuda.synchronize()
    assert np.array_equal(fl.idx.cpu().numpy(), R.sample_slots(seed, B, ctr + 1, size))
