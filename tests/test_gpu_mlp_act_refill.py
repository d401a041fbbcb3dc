"""The refill schedule of the MLP trainers (``RolloutMixin.rollout_jobs``, ``evaluate(schedule="refill")``) on the
lockstep act path (engine/act.py ``VecFastPolicy.step(restart=...)``): a slot whose episode has ended takes the next
episode id while the others step.  For CPQ (deterministic actor) and BCQ-Lag (decode noise drawn on the device, keyed by
(episode id, step): a restarted slot must restart its step count) every job equals, exactly, the same episode id run
alone through ``rollout_many`` on a fresh copy of its environment."""
import numpy as np
import pytest

from test_gpu_mlp_act_vec import _closed_loop_setup, _env

pytestmark = pytest.mark.gpu

SPECS = [(21, 50), (22, 7), (23, 13), (24, 7)]  # (seed, the environment's own length)


def _alone(tr, env_od, ad, slots, ids):
    """Job q alone: episode id ids[q] on a fresh copy of environment slots[q], in that environment's job order."""
    fresh = [_env(env_od, ad, s, el) for s, el in SPECS]
    return [tuple(x[0] for x in tr.rollout_many([fresh[e]], num_slots=1, episode_ids=np.array([i])))
            for e, i in zip(slots, ids)]


def _makespan(lengths, slots, N):
    busy = [0] * N
    for q, e in enumerate(slots):
        busy[e] += lengths[q]
    return max(busy)


@pytest.mark.parametrize("name", ["cpq_small", "bcql_small"])
def test_rollout_jobs_equal_each_episode_alone(name):
    c, m, tr, o, env_od = _closed_loop_setup(name)
    m.episode_len = 30
    make = lambda: [_env(env_od, c.ad, s, el) for s, el in SPECS]  # noqa: E731
    ids = np.array([70, 71, 72, 73, 74, 75, 76, 77, 78])
    res = tr.rollout_jobs(make(), 9, episode_ids=ids)
    np.testing.assert_array_equal(res.lengths[:4], [30, 7, 13, 7])
    np.testing.assert_array_equal(res.slots[:6], [0, 1, 2, 3, 1, 3])  # slots 1 and 3 end together: 1 takes job 4
    assert res.calls == _makespan(res.lengths, res.slots, 4) == 30  # in waves: 3 x 30, each waits for environment 0
    want = _alone(tr, env_od, c.ad, res.slots, ids)
    for q in range(9):
        assert (res.returns[q], res.lengths[q], res.costs[q]) == want[q], (name, q)
    if c.algo == "bcql":  # the episode id and the restarted step count are the noise key: same slot, other id, other run
        assert res.slots[1] == res.slots[4] and res.returns[1] != res.returns[4]
        other = tr.rollout_jobs(make(), 9, episode_ids=ids + 100)
        np.testing.assert_array_equal(other.slots, res.slots)
        assert (other.returns != res.returns).all()
    else:  # a deterministic actor on an environment that always starts alike repeats its episode
        assert res.returns[1] == res.returns[4]
    again = tr.rollout_jobs(make(), 9, episode_ids=ids)  # the default ids are the job numbers
    np.testing.assert_array_equal(again.returns, res.returns)
    dflt = tr.rollout_jobs(make(), 3)
    want = _alone(tr, env_od, c.ad, dflt.slots, np.arange(3))
    assert [(dflt.returns[q], dflt.lengths[q], dflt.costs[q]) for q in range(3)] == want


@pytest.mark.parametrize("name", ["cpq_small", "bcql_small"])
def test_evaluate_refill_is_the_mean_over_its_jobs(name):
    c, m, tr, o, env_od = _closed_loop_setup(name)
    m.episode_len = 30
    tr.reward_scale, tr.cost_scale = 2.0, 3.0
    make = lambda: [_env(env_od, c.ad, s, el) for s, el in SPECS]  # noqa: E731
    tr.env = make()
    m.train()
    got = tr.evaluate(7, schedule="refill")
    assert m.training
    res = tr.rollout_jobs(make(), 7)
    want = _alone(tr, env_od, c.ad, res.slots, np.arange(7))
    assert got == (np.mean([w[0] for w in want]) / 2.0, np.mean([w[2] for w in want]) / 3.0,
                   np.mean([w[1] for w in want]))
    with pytest.raises(ValueError, match='"waves" or "refill"'):
        tr.evaluate(7, schedule="fill")
    tr.env = []
    with pytest.raises(ValueError, match="empty"):
        tr.evaluate(3, schedule="refill")
