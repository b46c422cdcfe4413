"""hockey_amd.evaluator without a GPU: the three laws (the Evaluator's torch backend) against plain Python, the fold's
return sum against math.fsum within the bound of any summation order, the increments against the Philox words, the C
ABI's struct layout, exports and host-side refusals, and an Evaluator on the kernel source's host build against an
independent loop in evaluate()'s style."""
import ctypes
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from hockey_amd import _native as N
from hockey_amd import evaluator as E
from hockey_amd.collect import u53
from hockey_amd.explore import draw_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- the step law
@pytest.mark.parametrize("C,n", [(1, 1), (3, 5), (2, 65)])
def test_step_law_equals_a_per_row_loop(C, n):
    """Three calls on random reward / done / info (non-finite values among them) against a plain loop over the rows:
    live, length, winner, count and step as integers, ret as bits."""
    rng = np.random.default_rng(10 * C + n)
    seeds = [int(s) for s in rng.integers(0, 2 ** 63, C)]
    NN = C * n
    st = E.eval_begin_law(seeds, n)
    assert st["live"].all() and not st["ret"].any() and not np.signbit(st["ret"]).any()
    assert st["count"].tolist() == [n] * C and st["step"].tolist() == [0]
    live, ret, length, winner = [1] * NN, [0.0] * NN, [0] * NN, [0] * NN
    for call in range(3):
        reward = rng.standard_normal(NN).astype(np.float32)
        info = rng.integers(-1, 2, NN).astype(np.float32)
        done = (rng.random(NN) < 0.3).astype(np.uint8)
        reward[rng.integers(0, NN)] = np.nan
        info[rng.integers(0, NN)] = (np.nan, np.inf, -np.inf)[call]
        st = E.eval_step_law(seeds, n, st, reward, done, info)
        for i in range(NN):
            if live[i]:
                ret[i] = ret[i] + float(reward[i])
                length[i] += 1
                if done[i]:
                    winner[i] = 1 if info[i] > 0 else -1 if info[i] < 0 else 0
                    live[i] = 0
        assert st["live"].tolist() == live and st["length"].tolist() == length and st["winner"].tolist() == winner
        assert st["count"].tolist() == [sum(live[c * n:(c + 1) * n]) for c in range(C)]
        assert st["step"].tolist() == [call + 1]
        assert np.array_equal(st["ret"].view(np.uint64), np.array(ret, np.float64).view(np.uint64)), call
        for k, dt in (("live", np.uint8), ("length", np.int32), ("winner", np.int8), ("count", np.int32)):
            assert st[k].dtype == dt


@pytest.mark.parametrize("n", [1, 5, 255, 256, 257, 513])
def test_fold_law_counts_exact_and_return_sum_within_the_order_bound(n):
    """Counts and the length sum are exact; return_sum lies within (n - 1) 2^-53 sum|ret| of math.fsum over the
    finished rows -- the bound of recursive summation in any order, not tuned."""
    rng = np.random.default_rng(n)
    C = 3
    live = (rng.random(C * n) < 0.25).astype(np.uint8)
    ret = rng.standard_normal(C * n) * 10.0 ** rng.integers(-3, 4, C * n)
    length = rng.integers(1, 252, C * n).astype(np.int32)
    winner = rng.integers(-1, 2, C * n).astype(np.int8)
    outcomes, length_sum, return_sum = E.eval_fold_law(n, live, ret, length, winner)
    assert outcomes.dtype == np.int64 and length_sum.dtype == np.int64 and return_sum.dtype == np.float64
    for c in range(C):
        rows = [i for i in range(c * n, (c + 1) * n) if not live[i]]
        want = [sum(1 for i in rows if winner[i] == w) for w in (1, 0, -1)] + [n - len(rows)]
        assert outcomes[c].tolist() == want
        assert int(length_sum[c]) == sum(int(length[i]) for i in rows)
        exact = math.fsum(float(ret[i]) for i in rows)
        bound = (n - 1) * 2.0 ** -53 * math.fsum(abs(float(ret[i])) for i in rows)
        assert abs(float(return_sum[c]) - exact) <= bound, (c, float(return_sum[c]), exact, bound)
    # a live row's words reach nothing: non-finite returns of unfinished rows leave the sums alone
    ret2 = np.where(live != 0, np.nan, ret)
    again = E.eval_fold_law(n, live, ret2, length, winner)
    assert np.array_equal(again[2].view(np.uint64), return_sum.view(np.uint64))


def test_increments_are_the_cells_philox_words():
    """inc(c, local, t) = 0.2 u53 of the word pairs of draw_words(seed, KEY, n, t); begin holds t = 0, a step t + 1;
    the key is the header's and a cell's increments do not depend on the batch."""
    n, seeds = 70, [5, 2 ** 64 - 3, 77]
    assert E.KEY_PHASE == int.from_bytes(b"evalphas", "big")
    for t in (0, 1, 2 ** 33 + 1):
        w = draw_words(seeds[1], E.KEY_PHASE, n, t)
        want = np.stack([0.2 * u53(w[:, 0], w[:, 1]), 0.2 * u53(w[:, 2], w[:, 3])], 1)
        assert np.array_equal(E.eval_inc(seeds[1], n, t).view(np.uint64), want.view(np.uint64))
    st = E.eval_begin_law(seeds, n)
    assert np.array_equal(st["opp_inc"][n:2 * n], E.eval_inc(seeds[1], n, 0))
    z = np.zeros(3 * n)
    st = E.eval_step_law(seeds, n, st, z.astype(np.float32), z.astype(np.uint8), z.astype(np.float32))
    assert np.array_equal(st["opp_inc"][2 * n:], E.eval_inc(77, n, 1))
    solo = E.eval_step_law([77], n, E.eval_begin_law([77], n), z[:n].astype(np.float32), z[:n].astype(np.uint8),
                           z[:n].astype(np.float32))
    assert np.array_equal(solo["opp_inc"], st["opp_inc"][2 * n:])
    assert st["opp_inc"].min() >= 0 and st["opp_inc"].max() < 0.2


# ---------------------------------------------------------------------------------------------------- C ABI
def test_eval_abi_layout_exports_and_refusals(tmp_path):
    """include/hockey_eval.h as the C compiler lays it out against the ctypes struct; the library exports the entry
    points; each call refuses a malformed struct on the host (nothing is launched) with HKL_E_INVALID and a message
    that names it."""
    from hockey_amd import learner_hip as LH

    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hockey_learner.h"', "int main(void) {",
             '  printf("hkl_eval_io %zu\\n", sizeof(hkl_eval_io));']
    for f, _ in LH.EvalIO._fields_:
        lines.append(f'  printf("hkl_eval_io.{f} %zu\\n", offsetof(hkl_eval_io, {f}));')
    lines += ['  printf("key %llx\\n", (unsigned long long)HKL_EVAL_KEY_PHASE);',
              '  printf("cells %d\\n", HKL_EVAL_CELLS_MAX);', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    want = dict(line.split(None, 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert ctypes.sizeof(LH.EvalIO) == int(want["hkl_eval_io"])
    for f, _ in LH.EvalIO._fields_:
        assert getattr(LH.EvalIO, f).offset == int(want[f"hkl_eval_io.{f}"]), f
    assert want["key"] == f"{E.KEY_PHASE:x}" and int(want["cells"]) == E.CELLS_MAX

    L = LH.lib()
    assert all(hasattr(L, name) for name in LH.EVAL_EXPORTS)
    assert L.hkl_eval_io_size() == ctypes.sizeof(LH.EvalIO)
    for name, rows in refusal_cases(LH).items():
        for io, word in rows:
            assert L.hkl_tanh_probe(None, None, 0, None) == 1  # another entry point's message in between
            assert getattr(L, name)(None if io is None else ctypes.byref(io), None) == 1, (name, word)
            msg = L.hkl_last_error().decode()
            assert msg.startswith(name + ": ") and word in msg, (name, word, msg)


def refusal_cases(LH):
    """{entry point: [(io or None, a word of the message)]}: every HKL_E_INVALID case of include/hockey_eval.h."""
    def good(n_rows=40, rpc=20, **kw):
        io = LH.EvalIO()
        for f, t in LH.EvalIO._fields_:
            if t is ctypes.c_void_p:
                setattr(io, f, 256)
        io.n_rows, io.rows_per_cell, io.info_ld = n_rows, rpc, 4
        for k, v in kw.items():
            setattr(io, k, v)
        return io

    layout = [(None, "null"), (good(rpc=0), "rows_per_cell"), (good(rpc=-1), "rows_per_cell"),
              (good(n_rows=41), "multiple"), (good(n_rows=0), "multiple"), (good(n_rows=-20), "multiple"),
              (good(n_rows=65536, rpc=1), "n_cells"), (good(info_ld=0), "info_ld")]
    state = [(good(**{k: None}), k) for k in ("live", "ret", "length", "winner")]
    ctl = [(good(**{k: None}), k) for k in ("seeds", "step", "count")]
    return {"hkl_eval_begin": layout + state + ctl,
            "hkl_eval_step": layout + state + ctl + [(good(**{k: None}), k) for k in ("reward", "done", "info")],
            "hkl_eval_fold": layout + state + [(good(**{k: None}), k) for k in ("outcomes", "length_sum",
                                                                                "return_sum")]}


# ---------------------------------------------------------------------------------------------------- the host build
class HostEvalEnv:
    """VecHockeyEnv-shaped torch (CPU) view of hostcheck.HostVec that passes ``opp_inc`` through: what an Evaluator
    given ``env=`` calls."""

    def __init__(self, n):
        from hostcheck import HostVec

        self.n, self.h = n, HostVec(n, policies=("external", "external"))

    def reset_params(self, params, mask=None, max_t=None):
        self.h.reset_params(np.asarray(params, np.float32), mask, max_t)

    def set_state(self, state=None, aux=None, mask=None):
        self.h.set_state(state, None if aux is None else aux.numpy(), mask)

    def observe(self):
        o, o2 = self.h.observe()
        return torch.from_numpy(o), torch.from_numpy(o2)

    def step(self, actions=None, with_agent_two=False, policy2=None, opp_inc=None):
        r = self.h.step(actions.numpy(), with_agent_two=with_agent_two, policy2=policy2.numpy(),
                        opp_inc=opp_inc.numpy())
        return SimpleNamespace(**{k: torch.from_numpy(v) for k, v in vars(r).items()},
                               **({} if with_agent_two else {"obs2": None}))

    def close(self):
        self.h.close()


def _actors(k, seed=0):
    from hockey_amd.evaluate import Actor

    torch.manual_seed(seed)
    return [Actor().eval() for _ in range(k)]


@pytest.fixture(scope="module")
def host_case():
    """Cells (0, weak), (1, strong), (0, slot 1) of 4 episodes on the host build, played by a loop in evaluate()'s
    style: torch bookkeeping, the actors' own forwards, the reset_params placements, increments drawn here."""
    from hockey_amd.evaluate import reset_params
    from hockey_amd.policy_bank import PolicyBank

    actors = _actors(2, seed=3)
    bank = PolicyBank(2, "cpu")
    for a in actors:
        bank.add(a)
    p1, p2, seeds, n = [0, 1, 0], ["weak", "strong", 1], [42, 7, 1234], 4
    NN = 3 * n
    env = HostEvalEnv(NN)
    params = []
    for s in seeds:
        p, max_t, one = reset_params(n, s)
        assert one.tolist() == [False, True, False, True]
        params.append(p)
    env.reset_params(np.concatenate(params))
    policy2 = torch.tensor(np.repeat([N.POLICY_BASIC_WEAK, N.POLICY_BASIC_STRONG, N.POLICY_EXTERNAL], n).astype(np.uint8))
    who1 = np.repeat(p1, n)
    obs, obs2 = env.observe()
    ret = torch.zeros(NN, dtype=torch.float64)
    length = torch.zeros(NN, dtype=torch.int64)
    winner = torch.zeros(NN)
    live = torch.ones(NN, dtype=torch.bool)
    act = torch.zeros((NN, 8))
    with torch.no_grad():
        for t in range(max_t + 1):
            a = [actor(obs) for actor in actors]
            for i in range(NN):
                act[i, :4] = a[who1[i]][i]
            act[2 * n:, 4:] = actors[1](obs2)[2 * n:]
            inc = np.zeros((NN, 2))
            for c, s in enumerate(seeds):
                w = draw_words(s, 0x6576616C70686173, n, t)
                inc[c * n:(c + 1) * n, 0] = 0.2 * u53(w[:, 0], w[:, 1])
                inc[c * n:(c + 1) * n, 1] = 0.2 * u53(w[:, 2], w[:, 3])
            res = env.step(act, with_agent_two=True, policy2=policy2, opp_inc=torch.from_numpy(inc))
            ret += torch.where(live, res.reward.double(), torch.zeros_like(ret))
            length += live.long()
            d = res.done.bool()
            winner = torch.where(live & d, res.info[:, 0], winner)
            live &= ~d
            obs, obs2 = res.obs, res.obs2
            if not bool(live.any()):
                break
    env.close()
    assert not live.any()
    return SimpleNamespace(bank=bank, p1=p1, p2=p2, seeds=seeds, n=n, ret=ret.numpy(), length=length.numpy(),
                           winner=winner.numpy().astype(np.int8))


@pytest.mark.parametrize("poll_every", [16, 1, 1000])
def test_evaluator_on_the_host_build_equals_an_independent_loop(host_case, poll_every):
    """Evaluator(backend="torch", device="cpu", env=the host build): per-episode winner, length and return bits equal
    the independent loop's, whatever poll_every; the cell statistics are those arrays' means."""
    hc = host_case
    env = HostEvalEnv(3 * hc.n)
    ev = E.Evaluator(3, hc.n, device="cpu", backend="torch", poll_every=poll_every, env=env)
    r = ev.run(hc.bank, hc.p1, hc.p2, hc.seeds, per_episode=True)
    env.close()
    assert r["winner"].shape == r["returns"].shape == r["lengths"].shape == (3, 1, hc.n)
    assert r["winner"].dtype == np.int8 and r["returns"].dtype == np.float64 and r["lengths"].dtype == np.int32
    assert np.array_equal(r["winner"].reshape(-1), hc.winner)
    assert np.array_equal(r["lengths"].reshape(-1), hc.length)
    assert np.array_equal(r["returns"].reshape(-1).view(np.uint64), hc.ret.view(np.uint64))
    assert not r["unfinished"].any()
    w = hc.winner.reshape(3, hc.n)
    assert np.array_equal(r["win"], (w == 1).mean(1)) and np.array_equal(r["loss"], (w == -1).mean(1))
    assert np.array_equal(r["draw"], (w == 0).mean(1))
    assert np.array_equal(r["mean_length"], hc.length.reshape(3, hc.n).mean(1))
    assert np.allclose(r["mean_return"], hc.ret.reshape(3, hc.n).mean(1), rtol=1e-14, atol=0)
    if poll_every == 1:
        assert ev.steps == int(hc.length.max())
    elif poll_every == 1000:
        assert ev.steps == 251
    with pytest.raises(ValueError, match="one entry per cell"):
        ev.run(hc.bank, [0], hc.p2, hc.seeds)
    with pytest.raises(ValueError, match="slot"):
        ev.run(hc.bank, [0, 1, 5], hc.p2, hc.seeds)


def test_train_population_evaluator_hook_on_the_host_build():
    """train_population(evaluator=PopulationEval(...)) on the host build, 2 members x 4 arenas, two rounds at
    eval_interval 4: one batched call per due evaluation, one record per member and call; the first equals an
    Evaluator's on the members' actors (no update ran: the bank holds them throughout; the host build has no
    opponent_phase, so its bots' phases walk on into the second evaluation); eval_fn together with evaluator raises."""
    from hockey_amd.population import train_population
    from hockey_amd.td3 import TD3Config
    from hostcheck import HostTorchEnv

    cfg = TD3Config(batch_size=256, use_self_play=False, curriculum_name="noise_study", max_steps=20, start_steps=60,
                    noise_mode="gaussian", buffer_size=1000, eval_interval=4)
    members, calls = [(cfg, 3), (cfg, 4)], []
    pe = E.PopulationEval(members, episodes=2, backend="torch", env=HostEvalEnv(8))

    def evaluator(agents, bank, episodes):
        calls.append(episodes)
        return pe(agents, bank, episodes)

    kw = dict(n_arenas=4, rounds=2, device="cpu", explore="device", collect="device", graphs=False)
    agents, st = train_population(members, env=HostTorchEnv(8, policies=("external", "external")), evaluator=evaluator,
                                  **kw)
    assert calls == [4, 8]
    assert [[r["episode"] for r in s["evals"]] for s in st] == [[4, 8], [4, 8]]
    env = HostEvalEnv(8)
    r = E.Evaluator(4, 2, device="cpu", backend="torch", env=env).run(_bank(agents), [0, 0, 1, 1], ["strong", "weak"] * 2,
                                                                        [3, 3, 4, 4])
    env.close()
    for j in range(2):
        rec = st[j]["evals"][0]
        assert [rec["wr_strong"], rec["wr_weak"], rec["r_strong"], rec["r_weak"], rec["len_strong"], rec["len_weak"],
                rec["draw_strong"], rec["draw_weak"]] == [r[k][2 * j + o] for k in ("win", "mean_return", "mean_length",
                                                                                   "draw") for o in (0, 1)]
    with pytest.raises(ValueError, match="evaluator"):
        train_population(members, env=HostTorchEnv(8, policies=("external", "external")), evaluator=pe,
                         eval_fn=lambda ag, ep: {}, **kw)


def _bank(agents):
    from hockey_amd.policy_bank import PolicyBank

    bank = PolicyBank(len(agents), "cpu")
    for ag in agents:
        bank.add(ag.actor)
    return bank
