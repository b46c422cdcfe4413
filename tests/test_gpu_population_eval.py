"""train_population(evaluator=PopulationEval(...)) on the GPU: every due evaluation is one batched call on the training
bank, its records land per member, equal an Evaluator's on the final actors, and a member's records do not depend on the
population (explore="device", collect="device").  Sorts after tests/test_gpu_facade.py: training captures graphs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hockey_amd import evaluator as E  # noqa: E402
from hockey_amd import population as POP  # noqa: E402
from hockey_amd.td3 import TD3Config  # noqa: E402

DEV = "cuda:0"
ROUNDS, ARENAS, EPISODES = 3, 4, 4


def _cfg(noise, **kw):
    base = dict(batch_size=256, use_self_play=False, curriculum_name="noise_study", max_steps=30, start_steps=50,
                noise_mode=noise, buffer_size=2000, eval_interval=4)
    base.update(kw)
    return TD3Config(**base)


MEMBERS = [(_cfg("gaussian"), 21), (_cfg("uniform"), 34)]


def _train(members, **kw):
    ev = E.PopulationEval(episodes=EPISODES)
    agents, st = POP.train_population(members, n_arenas=ARENAS, rounds=ROUNDS, device=DEV, explore="device",
                                      collect="device", updates_per_round=2, replay_capacity=2000, evaluator=ev, **kw)
    torch.cuda.synchronize()
    return agents, st, ev


@pytest.fixture(scope="module")
def pair():
    agents, st, ev = _train(MEMBERS)
    yield agents, st
    ev.close()


def test_records_per_member_and_the_last_equals_an_evaluator_on_the_final_actors(pair):
    """2 members x 4 arenas x 3 rounds at eval_interval 4: an evaluation after every round, so three records each, at
    episodes 4, 8, 12; the last one equals Evaluator.run of a fresh bank holding the final actors."""
    from hockey_amd.policy_bank import PolicyBank

    agents, st = pair
    keys = {"episode", "wr_strong", "wr_weak", "r_strong", "r_weak", "draw_strong", "draw_weak", "len_strong",
            "len_weak"}
    for j in range(2):
        assert [r["episode"] for r in st[j]["evals"]] == [4, 8, 12]
        assert all(set(r) == keys for r in st[j]["evals"])
        assert st[j]["updates"] > 0  # the last evaluation saw trained weights
    bank = PolicyBank(2, DEV)
    for ag in agents:
        bank.add(ag.actor)
    ev = E.Evaluator(4, EPISODES, device=DEV)
    r = ev.run(bank, [0, 0, 1, 1], ["strong", "weak"] * 2, [21, 21, 34, 34])
    ev.close()
    for j in range(2):
        rec = st[j]["evals"][-1]
        for o, opp in enumerate(("strong", "weak")):
            c = 2 * j + o
            assert rec[f"wr_{opp}"] == r["win"][c] and rec[f"draw_{opp}"] == r["draw"][c]
            assert rec[f"r_{opp}"] == r["mean_return"][c] and rec[f"len_{opp}"] == r["mean_length"][c]
            assert np.isfinite(rec[f"r_{opp}"]) and 1 <= rec[f"len_{opp}"] <= 251


def test_a_members_records_do_not_depend_on_the_population(pair):
    """Member 0's records are the same bits in the pair and in a run of member 0 alone."""
    _, st = pair
    _, solo, ev = _train(MEMBERS[:1])
    ev.close()
    assert solo[0]["evals"] == st[0]["evals"] and len(solo[0]["evals"]) == 3


def test_eval_fn_together_with_evaluator_raises():
    with pytest.raises(ValueError, match="evaluator"):
        POP.train_population(MEMBERS, n_arenas=ARENAS, rounds=1, device=DEV,
                             eval_fn=lambda ag, ep: {}, evaluator=E.PopulationEval(episodes=EPISODES))
