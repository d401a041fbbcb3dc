"""``check_terminal`` (engine/mpc.py): every refusal of ``planner(terminal=, value_reduce=)`` is raised on the host, before
any device allocation -- the stand-ins below never saw a device, anything past the check would be an AttributeError."""
from types import SimpleNamespace as NS

import pytest


def stubs(**over):
    """(model, venv, kind, terminal, gamma, value_reduce, extra_obs) of an acceptable call, with ``over`` applied."""
    from osrl_amd.algorithms.fqe import FQE, FQETrainer
    from osrl_amd.common.model_env import ModelVecEnv
    model = NS(device="cuda:0", action_dim=2)
    venv = ModelVecEnv.__new__(ModelVecEnv)
    venv.state_dim, venv._halt_thr = 5, over.pop("halt_threshold", None)
    fqe = FQE.__new__(FQE)
    fqe.__dict__.update(dict(policy=model, device="cuda:0", state_dim=5, action_dim=2, gamma=0.99, c_hidden_sizes=[32, 32],
                             num_q=2), **over.pop("fqe", {}))
    tr = FQETrainer.__new__(FQETrainer)
    tr.model, tr.reward_scale, tr.cost_scale = fqe, 0.5, 4.0
    which = over.pop("terminal", "trainer")
    terminal = {"trainer": tr, "fqe": fqe}.get(which, which) if isinstance(which, str) else which
    return dict(dict(model=model, venv=venv, kind="cpq", gamma=0.99, value_reduce="mean", extra_obs=None), **over,
                terminal=terminal)


def test_an_acceptable_terminal_brings_its_scales():
    from osrl_amd.engine.mpc import check_terminal
    t = check_terminal(**stubs())
    assert (t.reward_scale, t.cost_scale, t.reduce) == (0.5, 4.0, 0)
    t = check_terminal(**stubs(terminal="fqe", value_reduce="pessimistic", halt_threshold=0.5))
    assert (t.reward_scale, t.cost_scale, t.reduce) == (1.0, 1.0, 1)
    assert check_terminal(**stubs(terminal=None)) is None


@pytest.mark.parametrize("error,over", [
    (TypeError, dict(terminal=object())),                       # neither an FQE nor an FQETrainer
    (ValueError, dict(fqe=dict(policy=NS()))),                  # fitted for another policy object
    (ValueError, dict(fqe=dict(device="cuda:1"))),
    (ValueError, dict(fqe=dict(state_dim=6))),
    (ValueError, dict(fqe=dict(action_dim=3))),
    (ValueError, dict(gamma=0.9)),                              # not the FQE's discount
    (ValueError, dict(gamma=1.0, fqe=dict(gamma=1.0), halt_threshold=0.5)),
    (ValueError, dict(extra_obs=7.0)),                          # BC multi-task's appended column
    (TypeError, dict(kind="bcql")),
    (ValueError, dict(value_reduce="median")),
    (ValueError, dict(value_reduce="max", terminal=None)),
    (ValueError, dict(fqe=dict(state_dim=447, c_hidden_sizes=[272]), venv_state_dim=447)),  # wide critics, wide input
])
def test_refusals(error, over):
    from osrl_amd.engine.mpc import ModelPlanner, check_terminal
    od = over.pop("venv_state_dim", None)
    kw = stubs(**over)
    if od is not None:
        kw["venv"].state_dim = od
    with pytest.raises(error):
        check_terminal(**kw)
    kw["venv"].E = 20  # the constructor and the trainers judge the shape, then the terminal, then build
    if kw["kind"] == "cpq" and kw["extra_obs"] is None and od is None:
        from osrl_amd.algorithms import CPQTrainer
        with pytest.raises(error):  # (no model: the refusal comes first, or fqe.policy is not None)
            CPQTrainer.__new__(CPQTrainer).planner(kw["venv"], 4, 3, gamma=kw["gamma"], terminal=kw["terminal"],
                                                   value_reduce=kw["value_reduce"])
    with pytest.raises(error):
        ModelPlanner(kw["model"], kw["venv"], kw["kind"], extra_obs=kw["extra_obs"], num_envs=4, horizon=3,
                     gamma=kw["gamma"], terminal=kw["terminal"], value_reduce=kw["value_reduce"])
