"""Plain references for the fused TD3 learner's kernels (csrc/hk_learner.hip, include/hockey_learner.h): torch on
the CPU in float64 for the critic step, the actor step, Adam and the Polyak averaging, and numpy (uint64 arithmetic)
for the Philox4x32-10 sampling.  Nothing here imports hockey_amd.learner_hip.

Test infrastructure only.  tests/test_learner_ref.py holds these references to the project's own eager code
(hockey_amd.td3) in float64 on the CPU; tests/test_gpu_learner_kernels.py holds the kernels to these references.

A network is its state dict ({"fc1.weight", "fc1.bias", ..., "fc3.bias"}, torch Linear layout [out][in]); ``nets`` is
a dict of the six MLPs: "actor", "target_actor", "q1", "q2", "tq1", "tq2".  ``ring`` is a dict of the replay columns
"s" [cap, 18], "a" [cap, 4], "r" [cap], "s2" [cap, 18], "d" [cap].  ``dtype`` / ``device`` (default float64 on the CPU)
let a test evaluate the very same expressions in float32: torch's own fp32 error, from which the kernels' bound is
taken (``bound``).
"""
import numpy as np
import torch

NETS = ("actor", "target_actor", "q1", "q2", "tq1", "tq2")
PARAMS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias")
XP = 32  # padded row of the stored first-layer inputs

# the (batch, seed) of every case the GPU tests build with make_case; test_learner_ref.py asserts the coverage
# conditions for each of them (with and without importance weights, identity and affine action map).  The batches
# are the smallest that take one split-K chunk (256), an odd number of 256-sample chunks (768: the critics' dW2
# falls back from 512-sample chunks) and two 512-sample critic chunks beside four 256-sample actor chunks (1024).
GPU_CASES = ((256, 11), (768, 12), (1024, 13))

ACT_AFFINE_LOW, ACT_AFFINE_RANGE = (-1.0, -2.0, 0.0, -0.5), (2.0, 4.0, 1.0, 3.0)


# ---------------------------------------------------------------------------------------------------- tolerances
def rel_err(got, ref):
    """err(T) = max|T - T_64| / max|T_64| (float64 arithmetic; a NaN anywhere in ``got`` gives NaN)."""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    return float((got - ref).abs().max() / ref.abs().max())


def bound(err_fp32_eager):
    """The kernels' bound for a tensor whose torch fp32 evaluation has error ``err_fp32_eager``: both sides are
    fp32 with a different summation order, and the factor 4 covers the kernels' tanh (absolute error 2e-7 against a
    correctly rounded fp32 tanh's 6e-8); the floor is for tensors torch happens to get nearly exactly."""
    return max(4.0 * err_fp32_eager, 4.0 * 2.0 ** -24)


# ---------------------------------------------------------------------------------------------------- networks
def _leaves(sd, dtype, device):
    return {k: sd[k].detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for k in PARAMS}


def _mlp(p, x, keep=False):
    """fc3(tanh(fc2(tanh(fc1(x))))) and, with keep, the pre-activations / activations (z1, h1, z2, h2), the
    pre-activations retaining their gradients."""
    z1 = torch.nn.functional.linear(x, p["fc1.weight"], p["fc1.bias"])
    h1 = torch.tanh(z1)
    z2 = torch.nn.functional.linear(h1, p["fc2.weight"], p["fc2.bias"])
    h2 = torch.tanh(z2)
    out = torch.nn.functional.linear(h2, p["fc3.weight"], p["fc3.bias"])
    if keep:
        if z1.requires_grad:
            z1.retain_grad()
            z2.retain_grad()
        return out, {"z1": z1, "h1": h1, "z2": z2, "h2": h2}
    return out


def unscale(a, low, rng):
    """TwinQNetwork._unscale_action: the critic's action input."""
    return ((a - low) / rng) * 2 - 1.0


def _smooth_l1(x, y, w):
    diff = x - y
    if w is None:
        return torch.where(diff.abs() < 1, 0.5 * diff ** 2, diff.abs() - 0.5)
    return torch.where(diff.abs() < 1, 0.5 * w * diff ** 2, (diff.abs() - 0.5) * w)


def _batch(ring, idx, dtype, device):
    i = torch.as_tensor(idx).long().cpu()
    return {k: ring[k].detach().cpu()[i].to(device=device, dtype=dtype) for k in ("s", "a", "r", "s2", "d")}


def _pad(x, dtype):
    return torch.cat([x, torch.zeros(x.shape[0], XP - x.shape[1], dtype=dtype, device=x.device)], 1)


def critic_reference(nets, ring, idx, noise, iw, gamma, act_low, act_range, dtype=torch.float64, device="cpu"):
    """TD3.compute_target and the critic half of TD3._update_tensors on the batch ring[idx] with the already clipped
    target noise [B, 4] and optional importance weights iw [B].

    Returns per row "y", "q1", "q2", "td" = (|q1 - y| + |q2 - y|) / 2 and "row_loss" (the row's term of
    smooth_l1(q1) + smooth_l1(q2): the loss is row_loss.sum() * 0.5 / B = "loss"); "x0" [B, 32] (s, unscale(a), 0);
    per critic k = 0, 1 "h1"[k], "dz2"[k], "dz1"[k] (the loss's gradients with respect to the two hidden
    pre-activations) and "grads"[k] (the six parameter gradients, keyed like the state dict); and the target's
    branch facts "min_is_q1" [B] and "clamped" [B, 4] (clamp(actor'(s2) + noise, -1, 1) active)."""
    b = _batch(ring, idx, dtype, device)
    low = torch.as_tensor(act_low, dtype=dtype, device=device)
    rng = torch.as_tensor(act_range, dtype=dtype, device=device)
    noise = torch.as_tensor(noise).detach().to(device=device, dtype=dtype)
    w = None if iw is None else torch.as_tensor(iw).detach().to(device=device, dtype=dtype)
    with torch.no_grad():
        ta = torch.tanh(_mlp(_leaves(nets["target_actor"], dtype, device), b["s2"]))
        raw = ta + noise
        a2 = torch.clamp(raw, -1.0, 1.0)
        x2 = torch.cat([b["s2"], unscale(a2, low, rng)], 1)
        tq1 = _mlp(_leaves(nets["tq1"], dtype, device), x2).squeeze(-1)
        tq2 = _mlp(_leaves(nets["tq2"], dtype, device), x2).squeeze(-1)
        y = b["r"] + gamma * (1 - b["d"]) * torch.minimum(tq1, tq2)
    x = torch.cat([b["s"], unscale(b["a"], low, rng)], 1)
    out = {"y": y, "x0": _pad(x, dtype), "min_is_q1": tq1 <= tq2, "clamped": raw.abs() > 1.0,
           "h1": [], "dz2": [], "dz1": [], "grads": []}
    params, caches, qs = [], [], []
    for key in ("q1", "q2"):
        p = _leaves(nets[key], dtype, device)
        q, c = _mlp(p, x, keep=True)
        params.append(p)
        caches.append(c)
        qs.append(q.squeeze(-1))
    rows = _smooth_l1(qs[0], y, w) + _smooth_l1(qs[1], y, w)
    loss = (_smooth_l1(qs[0], y, w).mean() + _smooth_l1(qs[1], y, w).mean()) * 0.5
    loss.backward()
    for p, c in zip(params, caches):
        out["h1"].append(c["h1"].detach())
        out["dz2"].append(c["z2"].grad)
        out["dz1"].append(c["z1"].grad)
        out["grads"].append({k: p[k].grad for k in PARAMS})
    out["q1"], out["q2"] = qs[0].detach(), qs[1].detach()
    out["td"] = ((out["q1"] - y).abs() + (out["q2"] - y).abs()) / 2
    out["row_loss"], out["loss"] = rows.detach(), loss.detach()
    return out


def actor_reference(nets, ring, idx, act_low, act_range, dtype=torch.float64, device="cpu"):
    """The actor half of TD3._update_tensors: loss = -mean Q1(s, unscale(actor(s))).  Returns "x0" [B, 32] (s, 0), the
    actor's "h1", "h2", "dz2", "dz1", the "loss" and the six actor gradients "grads"."""
    b = _batch(ring, idx, dtype, device)
    low = torch.as_tensor(act_low, dtype=dtype, device=device)
    rng = torch.as_tensor(act_range, dtype=dtype, device=device)
    p = _leaves(nets["actor"], dtype, device)
    pre, c = _mlp(p, b["s"], keep=True)
    a = torch.tanh(pre)
    q = _mlp(_leaves(nets["q1"], dtype, device), torch.cat([b["s"], unscale(a, low, rng)], 1)).squeeze(-1)
    loss = -q.mean()
    loss.backward(inputs=list(p.values()) + [c["z1"], c["z2"]])
    return {"x0": _pad(b["s"], dtype), "h1": c["h1"].detach(), "h2": c["h2"].detach(), "dz2": c["z2"].grad,
            "dz1": c["z1"].grad, "loss": loss.detach(), "grads": {k: p[k].grad for k in PARAMS},
            "action": a.detach()}


# ---------------------------------------------------------------------------------------------------- optimiser
def adam_reference(p, m, v, g, step, lr, b1=0.9, b2=0.999, eps=1e-6, wd=0.0):
    """torch.optim.Adam's update written out in float64: ``step`` optimiser steps were taken before this one; L2
    weight decay is added to g; bias-corrected moments, denom = sqrt(v) / sqrt(bc2) + eps.  Returns (p, m, v)."""
    p, m, v, g = (torch.as_tensor(t).detach().double().cpu() for t in (p, m, v, g))
    t = int(step) + 1
    if wd != 0.0:
        g = g + wd * p
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    denom = v.sqrt() / bc2 ** 0.5 + eps
    return p - (lr / bc1) * (m / denom), m, v


def polyak_reference(target, param, rho, tau):
    """soft_update: target * rho + tau * param in float64."""
    return torch.as_tensor(target).detach().double().cpu() * rho + tau * torch.as_tensor(param).detach().double().cpu()


# ---------------------------------------------------------------------------------------------------- sampling
_M0, _M1, _W0, _W1, _LO = (np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85),
                           np.uint64(0xFFFFFFFF))
_S32 = np.uint64(32)
NOISE_KEY = 0x6E6F697365


def philox4x32_10(key, counter):
    """Philox4x32-10 (Salmon et al., SC'11): key (uint64: low word k0, high word k1; scalar or [n]) and counter
    ([..., 4] uint32 words) -> [..., 4] uint32."""
    key = np.asarray(key, dtype=np.uint64)
    c = np.asarray(counter).astype(np.uint64)
    assert c.shape[-1] == 4
    k0, k1 = key & _LO, key >> _S32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def _sample_counters(batch, ctr):
    e = np.arange(batch, dtype=np.uint64)
    ctr = np.uint64(ctr)
    return np.stack([e & _LO, e >> _S32, np.full(batch, ctr & _LO), np.full(batch, ctr >> _S32)], -1)


def sample_slots(seed, batch, ctr, size):
    """hkl_sample's replay slots of update ``ctr``: floor(u * size) of the 53-bit u = ((x << 32 | y) >> 11) * 2^-53
    of Philox(seed, (e lo, e hi, ctr lo, ctr hi)), clamped to size - 1 (rl/replay/uniform_buffer.py's
    (rand * size).astype(int)); int64 [batch]."""
    r = philox4x32_10(np.uint64(seed), _sample_counters(batch, ctr)).astype(np.uint64)
    bits = ((r[:, 0] << _S32) | r[:, 1]) >> np.uint64(11)
    u = bits.astype(np.float64) * 2.0 ** -53
    i = (u * np.float64(size)).astype(np.uint64)
    return np.minimum(i, np.uint64(size - 1)).astype(np.int64)


def sample_noise(seed, batch, ctr, scale, clip, dtype=np.float64):
    """hkl_sample's clipped target-smoothing noise [batch, 4] of update ``ctr``: key seed ^ 0x6E6F697365, Box-Muller
    on the 24-bit uniforms u1 = ((w >> 8) + 0.5) 2^-24 and u2 = (w >> 8) 2^-24 of word pairs (x, y) and (z, w) --
    (rad cos, rad sin), rad = sqrt(-2 ln u1), angle 2 pi u2 -- times scale, clamped to +-clip.  ``dtype``: the
    arithmetic's precision (float32: the same formula as numpy evaluates it in single precision)."""
    f = np.dtype(dtype).type
    r = philox4x32_10(np.uint64(seed) ^ np.uint64(NOISE_KEY), _sample_counters(batch, ctr))
    z = np.zeros((batch, 4), dtype)
    for p in range(2):
        u1 = ((r[:, 2 * p] >> 8).astype(dtype) + f(0.5)) * f(2.0 ** -24)
        u2 = (r[:, 2 * p + 1] >> 8).astype(dtype) * f(2.0 ** -24)
        rad = np.sqrt(f(-2.0) * np.log(u1))
        ang = f(2.0 * np.pi) * u2
        z[:, 2 * p], z[:, 2 * p + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return np.clip(z * f(scale), f(-clip), f(clip))


# ---------------------------------------------------------------------------------------------------- cases
def _linear(g, n_out, n_in, gain=1.0):
    k = gain / n_in ** 0.5  # torch.nn.Linear's default range
    return (torch.rand(n_out, n_in, generator=g) * 2 - 1) * k, (torch.rand(n_out, generator=g) * 2 - 1) * k


def _net(g, n_in, n_out, h=256, gain=1.5):
    """torch.nn.Linear's default initialisation widened by ``gain``: at 1.5 the hidden units' rms is 0.57 (0.44 at the
    default), so 1 - h^2 of the tanh backward varies across units, and the target actor's scaled output saturates
    often enough for the action clamp to act in a fifth of the components."""
    sd = {}
    for name, (o, i) in (("fc1", (h, n_in)), ("fc2", (h, h)), ("fc3", (n_out, h))):
        sd[name + ".weight"], sd[name + ".bias"] = _linear(g, o, i, gain)
    return sd


def make_case(B, seed, per=False, act_affine=False, capacity=1000, noise_scale=0.2, noise_clip=0.3):
    """A ring of ``capacity`` transitions, six independent fp32 networks and a batch of B rows that reaches every
    branch of the critic step: rewards 2 randn (|q - y| on both sides of 1, both signs), d = 1 in ~30 % of the
    slots, idx unsorted with duplicates and both end slots, the target actor's fc3 scaled by 5 (tanh saturates, so
    clamp(. + noise, -1, 1) is active), noise already clipped with entries equal to +-clip, importance weights in
    (0.05, 1] when ``per``, and a non-identity action map when ``act_affine`` (stored actions lie in
    [low, low + range])."""
    g = torch.Generator().manual_seed(int(seed))
    low = torch.tensor(ACT_AFFINE_LOW if act_affine else (-1.0,) * 4)
    rng = torch.tensor(ACT_AFFINE_RANGE if act_affine else (2.0,) * 4)
    ring = {"s": torch.randn(capacity, 18, generator=g), "a": low + rng * torch.rand(capacity, 4, generator=g),
            "r": 2.0 * torch.randn(capacity, generator=g), "s2": torch.randn(capacity, 18, generator=g),
            "d": (torch.rand(capacity, generator=g) < 0.3).float()}
    nets = {"actor": _net(g, 18, 4), "target_actor": _net(g, 18, 4), "q1": _net(g, 22, 1), "q2": _net(g, 22, 1),
            "tq1": _net(g, 22, 1), "tq2": _net(g, 22, 1)}
    for k in ("fc3.weight", "fc3.bias"):
        nets["target_actor"][k] = nets["target_actor"][k] * 5.0
    idx = torch.randint(0, capacity, (B,), generator=g)
    idx[1], idx[B // 2], idx[B - 1], idx[B - 2] = 0, capacity - 1, idx[0], capacity - 1  # end slots, sure duplicates
    noise = torch.clamp(torch.randn(B, 4, generator=g) * noise_scale, -noise_clip, noise_clip)
    noise[0, 0], noise[0, 1] = noise_clip, -noise_clip
    iw = (0.05 + 0.95 * torch.rand(B, generator=g)).clamp(max=1.0) if per else None
    if iw is not None:
        iw[3] = 1.0
    return {"B": B, "seed": seed, "per": per, "act_affine": act_affine, "ring": ring, "nets": nets, "idx": idx,
            "noise": noise, "iw": iw, "gamma": 0.99, "act_low": tuple(low.tolist()), "act_range": tuple(rng.tolist()),
            "noise_clip": noise_clip}
