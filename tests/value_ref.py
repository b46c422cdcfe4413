"""The float64 restatement of hockey_amd.value.ValueFn / hkl_value, from learner_ref's pieces: Q_k(s, unscale(a)) of two
critics and, without an action, a = tanh(actor(s)) first.  Test infrastructure only; tests/test_value.py holds the torch
backend to it on the CPU, tests/test_gpu_value.py the kernel.  ``dtype`` / ``device`` evaluate the very same expressions
in float32: torch's own fp32 error, from which the bound is taken (learner_ref.bound)."""
import torch

import learner_ref as R


def value_nets(seed, gain=1.5):
    """{"actor": 18 -> 4, "q1": 22 -> 1, "q2": 22 -> 1} of learner_ref._net state dicts."""
    g = torch.Generator().manual_seed(int(seed))
    return {"actor": R._net(g, 18, 4, gain=gain), "q1": R._net(g, 22, 1, gain=gain), "q2": R._net(g, 22, 1, gain=gain)}


def critic_state(nets, low, rng):
    """A TwinQ state dict of nets["q1"], nets["q2"] and the action map."""
    low, rng = torch.as_tensor(low, dtype=torch.float32), torch.as_tensor(rng, dtype=torch.float32)
    sd = {"action_low": low, "action_high": low + rng, "action_range": rng}
    for k in ("q1", "q2"):
        sd.update({f"{k}.{name}": v for name, v in nets[k].items()})
    return sd


def value_reference(nets, obs, act, low, rng, dtype=torch.float64, device="cpu", keep=False):
    """{"a", "q1", "q2", "qmin"} of rows obs [n, >= 18] (and act [n, >= 4], or None: a = tanh(actor(obs))) in ``dtype``
    on ``device``; with keep also "hidden": every hidden activation of the networks that ran, flattened."""
    with torch.no_grad():
        x = obs[:, :18].detach().to(device=device, dtype=dtype)
        p = {k: {n: v.to(device=device, dtype=dtype) for n, v in nets[k].items()} for k in nets}
        low = torch.as_tensor(low, dtype=dtype, device=device)
        rng = torch.as_tensor(rng, dtype=dtype, device=device)
        hidden = []
        if act is None:
            pre, c = R._mlp(p["actor"], x, keep=True)
            a = torch.tanh(pre)
            hidden += [c["h1"], c["h2"]]
        else:
            a = act[:, :4].detach().to(device=device, dtype=dtype)
        xc = torch.cat([x, R.unscale(a, low, rng)], 1)
        out = {"a": a}
        for k in ("q1", "q2"):
            q, c = R._mlp(p[k], xc, keep=True)
            out[k] = q.squeeze(-1)
            hidden += [c["h1"], c["h2"]]
        out["qmin"] = torch.minimum(out["q1"], out["q2"])
        if keep:
            out["hidden"] = torch.cat([h.reshape(-1) for h in hidden])
    return out
