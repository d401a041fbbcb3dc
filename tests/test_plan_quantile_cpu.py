"""``check_terminal`` with quantile critics and ``risk_alpha`` (engine/mpc.py), on the host: the stand-ins of
tests/test_plan_value_cpu.py never saw a device."""
import pytest

from test_plan_value_cpu import stubs

QUANTILE = dict(fqe=dict(num_quantiles=8))


def test_a_quantile_terminal_is_accepted_and_brings_its_tails():
    from osrl_amd.engine.mpc import check_risk_alpha, check_terminal
    assert check_terminal(**stubs(**QUANTILE)).risk_alpha == (1.0, 1.0)
    assert check_terminal(**stubs(**QUANTILE), risk_alpha=0.25).risk_alpha == (0.25, 0.25)
    assert check_terminal(**stubs(**QUANTILE), risk_alpha=(0.1, 0.5)).risk_alpha == (0.1, 0.5)
    assert check_terminal(**stubs()).risk_alpha is None
    # estimate_risk's rule: ceil(alpha M), an alpha M within 1e-9 of an integer is that integer, at least one
    assert check_risk_alpha((0.1, 0.5), 21)[1] == (3, 11) and check_risk_alpha(0.3, 10)[1] == (3, 3)
    assert check_risk_alpha(None, 64)[1] == (64, 64) and check_risk_alpha(0.001, 2)[1] == (1, 1)


@pytest.mark.parametrize("error,over,risk_alpha", [
    (ValueError, {}, 0.5),                       # a scalar FQE has no tail
    (ValueError, dict(terminal=None), 0.5),      # nor has no terminal at all
    (ValueError, QUANTILE, 0.0),
    (ValueError, QUANTILE, 1.5),
    (ValueError, QUANTILE, (0.5, 0.0)),
    (TypeError, dict(kind="bcql", **QUANTILE), None),
])
def test_refusals(error, over, risk_alpha):
    from osrl_amd.engine.mpc import ModelPlanner, check_terminal
    kw = stubs(**over)
    with pytest.raises(error):
        check_terminal(**kw, risk_alpha=risk_alpha)
    kw["venv"].E = 20  # (the constructor judges the shape, then the terminal, then builds: nothing here has a device)
    with pytest.raises(error):
        ModelPlanner(kw["model"], kw["venv"], kw["kind"], num_envs=4, horizon=3, gamma=kw["gamma"],
                     terminal=kw["terminal"], risk_alpha=risk_alpha)
