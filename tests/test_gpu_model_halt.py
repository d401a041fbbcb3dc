"""Model rollouts that halt on uncertainty, with a pessimistic cost (csrc/model_env.hip flag kPess: the ``_halt`` entry
points; csrc/compact.hip ``osrl_collect_compact``; ``ModelVecEnv(halt_threshold=, halt_reward=, halt_cost=,
cost_penalty=)``; ``ModelCollector`` / ``Trainer.collect_model`` with variable-length episodes; ``evaluate``).

Bounds.  Against the fp64 oracle (tests/model_halt_oracle.py): ``halt_step``, lengths, ``terminals`` and ``timeouts``
exactly -- tests/test_model_halt_cpu.py holds every u at least 20 parity bounds away from the case's threshold, so no halt
decision is left out; states, rewards, ``acc``, ``disc``, ``unc`` and the per-row u to 1e-4 of each tensor's scale (the
project's bound, tests/test_gpu_model_env.py ``BOUND``); the cost bit where the oracle's c + kappa u is farther than 1e-3
from 0.5, at most 2 % of the rows left out.  Everything else is exact: the defaults against the old entry points, an
episode against itself at another E or under a graph, dense rows against padded rows.
Shapes: tests/model_halt_cases.py (E = 19: two tiles, the second partial; 12 steps; od 37 > 32; width 24)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gauss_dynamics_cases as GC
import model_collect_cases as K
import model_env_cases as MC
import model_halt_cases as HC
from model_halt_oracle import KEYS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOUND = 1e-4
E, T, CS = HC.E, HC.T, HC.CS


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def dynamics(case):
    from osrl_amd.algorithms import Dynamics
    c = HC.CASES[case]
    torch.manual_seed(7)
    kw = dict(probabilistic=True, logvar_min=GC.LOGVAR_MIN, logvar_max=GC.LOGVAR_MAX) if case == "G" else {}
    m = Dynamics(c["od"], c["ad"], list(c["hidden"]), num_models=c["M"], device=DEV, **kw)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in HC.state_dict(case).items()})
    return m


def make_env(case, n=E, episode_len=T, pess=True, thr=None, **kw):
    """The case's environment: lambda, clamp, mode "mean" (and for G max_std with injected draws); ``pess``: the case's
    threshold (or ``thr``), halt reward and cost, kappa."""
    from osrl_amd.common.model_env import ModelVecEnv
    model = dynamics(case)
    if case == "G":
        kw = dict(dict(sample=True, uncertainty="max_std"), **kw)
    if pess:
        kw = dict(dict(halt_threshold=HC.threshold(case) if thr is None else thr, halt_reward=HC.HALT_REWARD,
                       halt_cost=HC.HALT_COST, cost_penalty=HC.KAPPA), **kw)
    v = ModelVecEnv(model, MC.init_states(model.state_dim), n, episode_len, max_action=MC.MAX_ACTION,
                    reward_penalty=HC.LAMBDA, clip_states=True, **kw)
    if case == "G" and v.sample:
        v.set_noise_in(GC.noise(n, model.state_dim + 1))
    return v


@functools.lru_cache(maxsize=None)
def policy(case, kind="zero", episode_len=T):
    """A BC actor: "zero" (all parameters 0: with sigma = 1 the injected noise IS the action), "const" (the case data's
    constant policy) or "random"."""
    from osrl_amd.algorithms import BC
    c = HC.CASES[case]
    torch.manual_seed(2)
    bc = BC(c["od"], c["ad"], MC.MAX_ACTION, [32, 32] if kind == "random" else K.POLICY_HIDDEN, episode_len, device=DEV)
    if kind != "random":
        sd = K.bc_const_state_dict(c["od"], c["ad"])
        if kind == "zero":
            sd = {k: np.zeros_like(v) for k, v in sd.items()}
        bc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return bc


def collector(case, venv, kind="zero", **kw):
    from osrl_amd.engine.collect import ModelCollector
    return ModelCollector(policy(case, kind), venv, "bc", CS, **kw)


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d, scale = float(np.abs(got - want).max()) if got.size else 0.0, float(np.abs(want).max()) if want.size else 0.0
    print(f"  {what}: max diff {d:.3e}, scale {scale:.3e}, ratio {d / max(scale, 1e-300):.2e}")
    assert d <= BOUND * scale, f"{what}: max diff {d:.3e} vs scale {scale:.3e}"


def cost_bits(eff, what):
    """The project's rule for the cost bit: compared where the oracle is farther than 1e-3 from 0.5, at most 2 % left out.
    Returns the mask of rows compared."""
    clear = np.abs(eff - 0.5) > 1e-3
    print(f"  {what}: {int((~clear).sum())} of {clear.size} cost rows within 1e-3 of the threshold")
    assert (~clear).sum() <= 0.02 * clear.size
    return clear


# ------------------------------------------------------------------------------------------------------------------ #
# 1. parity with the oracle
# ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("case", HC.NAMES)
def test_step_parity(case):
    ref = HC.halting_rollout(case)
    venv = make_env(case)
    od = venv.state_dim
    obs, so = torch.zeros(E, od, device=DEV), torch.zeros(E, 2, device=DEV)
    venv.reset(obs)
    desc = venv.desc(T, CS)
    acts = dev(HC.actions(case))
    pad, eff = ref["pad"], ref["cost_eff"]
    done = np.zeros(E, bool)
    for t in range(T):
        so.fill_(float("nan"))
        venv.step(desc, acts[t], obs, so)
        live = ~done
        assert torch.equal(obs, venv.state)
        s, o = venv.state.cpu().numpy(), so.cpu().numpy()
        assert np.isnan(o[done]).all()  # a finished episode's launch stores nothing
        if live.any():
            close(s[live], pad["next_observations"][live, t], f"step {t} s'")
            close(o[live, 0], pad["rewards"][live, t], f"step {t} reward")
            halted = pad["terminals"][live, t] == 1
            np.testing.assert_array_equal(o[live, 0][halted], np.float32(HC.HALT_REWARD))
            np.testing.assert_array_equal(o[live, 1][halted], np.float32(HC.HALT_COST))
            clear = np.abs(eff[live, t] - 0.5) > 1e-3  # (the 2 % cap is held over the whole run, below)
            np.testing.assert_array_equal(o[live, 1][clear], pad["costs"][live, t][clear])
        done = ref["lengths"] <= t + 1
    np.testing.assert_array_equal(venv.halted(), ref["halt_step"])
    acc, unc = venv.acc.cpu().numpy(), venv.unc.cpu().numpy()
    np.testing.assert_array_equal(acc[:, 2], ref["lengths"])
    assert (acc[:, 3] == 1).all()
    clear = cost_bits(ref["dense_cost_eff"], case)
    close(acc[:, 0], ref["acc"][:, 0], "returns")
    all_clear = np.array([clear[a:b].all() for a, b in zip(ref["offsets"][:-1], ref["offsets"][1:])])
    np.testing.assert_array_equal(acc[all_clear, 1], ref["acc"][all_clear, 1])
    close(unc, ref["unc"], "unc")
    close(venv.state.cpu().numpy(), ref["state"], "final state (a halted episode's is its halting step's s')")
    # every episode is finished: further launches move nothing
    keep = [t.clone() for t in (venv.state, venv.acc, venv.unc, venv.halt_step)]
    for t in range(3):
        venv.step(desc, acts[t], obs, so)
    for a, b in zip(keep, (venv.state, venv.acc, venv.unc, venv.halt_step)):
        assert torch.equal(a, b)


@functools.lru_cache(maxsize=None)
def halting_run(case, n=E, thr=None):
    """``collect_model``'s run with the oracle rollout's actions: the zero policy, sigma = 1, the actions injected as the
    noise (clip(fmaf(1, a, 0)) = clip(a)); gamma = 0.9."""
    venv = make_env(case, n, thr=thr)
    col = collector(case, venv)
    res = col.run(noise_std=1.0, gamma=0.9, noise=HC.actions(case, n))
    assert col.guards_intact()
    return res, col, venv


@pytest.mark.parametrize("case", HC.NAMES)
def test_collect_parity(case):
    ref = HC.halting_rollout(case)
    res, col, venv = halting_run(case, E, None)
    n = int(ref["offsets"][-1])
    np.testing.assert_array_equal(venv.halted(), ref["halt_step"])
    np.testing.assert_array_equal(res.lengths, ref["lengths"])
    np.testing.assert_array_equal(col.row_offsets.cpu().numpy(), ref["offsets"])
    d = {k: v.cpu().numpy() for k, v in res.dataset.items()}
    assert all(v.shape[0] == n for v in d.values()) and col.row_disagreement.shape == (n,)
    np.testing.assert_array_equal(d["terminals"], ref["dense"]["terminals"])
    np.testing.assert_array_equal(d["timeouts"], ref["dense"]["timeouts"])
    assert d["terminals"].sum() == (ref["halt_step"] >= 0).sum()
    for k in ("observations", "actions", "next_observations", "rewards"):
        close(d[k], ref["dense"][k], k)
    close(col.row_disagreement.cpu().numpy(), ref["dense_row_u"], "row_disagreement")
    clear = cost_bits(ref["dense_cost_eff"], case)
    np.testing.assert_array_equal(d["costs"][clear], ref["dense"]["costs"][clear])
    halted = ref["dense"]["terminals"] == 1
    np.testing.assert_array_equal(d["rewards"][halted], np.float32(HC.HALT_REWARD))
    np.testing.assert_array_equal(d["costs"][halted], np.float32(HC.HALT_COST))
    close(res.returns, ref["acc"][:, 0], "returns")
    close(res.disc_returns, ref["disc"][:, 0], "discounted returns")
    all_clear = np.array([clear[a:b].all() for a, b in zip(ref["offsets"][:-1], ref["offsets"][1:])])
    np.testing.assert_array_equal(res.cost_returns[all_clear], ref["acc"][all_clear, 1])
    close(res.disc_cost_returns[all_clear], ref["disc"][all_clear, 1], "discounted cost returns")
    close(venv.unc.cpu().numpy(), ref["unc"], "unc")
    close(venv.state.cpu().numpy(), ref["state"], "final state")
    # the step path and the recording path are the same body: the same bits
    step = make_env(case)
    obs = torch.zeros(E, step.state_dim, device=DEV)
    step.reset(obs)
    desc, acts = step.desc(T, CS), dev(HC.actions(case))
    for t in range(T):
        step.step(desc, acts[t], obs)
    for a, b in ((step.state, venv.state), (step.acc, venv.acc), (step.unc, venv.unc), (step.halt_step, venv.halt_step)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ #
# 2. the defaults are the old bits
# ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("case", ["B", "G"])
def test_defaults_are_the_old_step(case):
    from osrl_amd import _lib as L
    from osrl_amd.engine.core import cur_stream
    old, new = make_env(case, pess=False), make_env(case, pess=False)
    desc = old.desc(T, CS)
    assert type(desc) is (L.ModelEnvGaussT if case == "G" else L.ModelEnvT) and not old.can_halt
    pess = L.ModelEnvPessT()
    pess.halt_threshold, pess.halt_reward, pess.halt_cost, pess.cost_penalty = float("inf"), -7.0, 1.0, 0.0
    pess.halt_step = new.halt_step.data_ptr()
    name = "osrl_model_env_step_gauss_halt" if case == "G" else "osrl_model_env_step_halt"
    od = old.state_dim
    obs = [torch.zeros(E, od, device=DEV) for _ in range(2)]
    so = [torch.zeros(E, 2, device=DEV) for _ in range(2)]
    old.reset(obs[0])
    new.reset(obs[1])
    acts = dev(HC.actions(case))
    for t in range(T + 2):  # (two launches past the end: both freeze)
        a = acts[t % T]
        old.step(desc, a, obs[0], so[0])
        L.check(getattr(L.load(), name)(C.byref(desc), C.byref(pess), a.data_ptr(), new.state.data_ptr(),
                                        obs[1].data_ptr(), obs[1].stride(0), new.acc.data_ptr(), new.unc.data_ptr(),
                                        so[1].data_ptr(), E, cur_stream()), name)
        for x, y in ((old.state, new.state), (obs[0], obs[1]), (old.acc, new.acc), (old.unc, new.unc), (so[0], so[1])):
            assert torch.equal(x, y), t
    assert (new.halt_step == -1).all() and (old.acc[:, 2] == T).all()
    # the C ABI's refusals
    for field, bad in (("halt_threshold", float("nan")), ("halt_cost", 0.5), ("cost_penalty", -1.0)):
        p2 = L.ModelEnvPessT.from_buffer_copy(pess)
        setattr(p2, field, bad)
        assert getattr(L.load(), name)(C.byref(desc), C.byref(p2), acts[0].data_ptr(), new.state.data_ptr(),
                                       obs[1].data_ptr(), obs[1].stride(0), new.acc.data_ptr(), new.unc.data_ptr(),
                                       so[1].data_ptr(), E, cur_stream()) == -1, field


@pytest.mark.parametrize("case", ["B", "G"])
def test_defaults_are_the_old_collect(case):
    """threshold +inf, penalty 0 through ``osrl_model_env_collect[_gauss]_halt`` (and the compaction, here the identity)
    against the plain entry point: every table, ``disc``, ``acc``, ``unc``, the state and the per-row u."""
    from osrl_amd import _lib as L
    old = make_env(case, pess=False)
    new = make_env(case, pess=False, halt_threshold=float("inf"))
    assert isinstance(new.desc(T, CS), L.ModelEnvGaussHaltT if case == "G" else L.ModelEnvHaltT) and new.can_halt
    noise = MC.actions(E, HC.CASES[case]["ad"], seed=11)
    runs = []
    for v in (old, new):
        col = collector(case, v, "const")
        res = col.run(noise_std=K.sigma(), gamma=0.9, noise=noise)
        assert col.guards_intact()
        runs.append((res, col, v))
    (r0, c0, v0), (r1, c1, v1) = runs
    assert c0.row_offsets is None and c0._dense is None
    np.testing.assert_array_equal(c1.row_offsets.cpu().numpy(), np.arange(E + 1) * T)
    for k in KEYS:
        assert torch.equal(c0.tables[k], c1.tables[k]) and torch.equal(r0.dataset[k], r1.dataset[k]), k
    for x, y in ((c0.disc, c1.disc), (v0.acc, v1.acc), (v0.unc, v1.unc), (v0.state, v1.state), (c0._row_unc, c1._row_unc),
                 (c0.row_disagreement, c1.row_disagreement)):
        assert torch.equal(x, y)
    assert (v1.halt_step == -1).all() and not r1.dataset["terminals"].any()


def test_defaults_hand_out_the_old_descriptors():
    from osrl_amd import _lib as L
    for case, plain, halt in (("A", L.ModelEnvT, L.ModelEnvHaltT), ("G", L.ModelEnvGaussT, L.ModelEnvGaussHaltT)):
        v = make_env(case, pess=False)
        assert type(v.desc(T, CS)) is plain and v.extra_state[1] is v.halt_step and (v.halted() == -1).all()
        e0 = v.launch_epoch
        v.cost_penalty = 0.5
        d = v.desc(T, CS)
        assert type(d) is halt and d.pess.halt_threshold == float("inf") and not v.can_halt and v.launch_epoch == e0 + 1
        assert d.episode_len == T and d.launch_epoch == v.launch_epoch
        v.cost_penalty = 0.0
        v.halt_threshold = 0.25
        d = v.desc(T, CS)
        assert type(d) is halt and d.pess.halt_threshold == 0.25 and d.pess.halt_step == v.halt_step.data_ptr() and v.can_halt
        v.halt_threshold = None
        assert type(v.desc(T, CS)) is plain and v.launch_epoch == e0 + 4
    with pytest.raises(ValueError):
        make_env("A", thr=float("nan"))
    with pytest.raises(ValueError):
        make_env("A", halt_cost=0.5)
    with pytest.raises(ValueError):
        make_env("A", cost_penalty=-1.0)


# ------------------------------------------------------------------------------------------------------------------ #
# 3. independence of E, of the graph, of what follows a halt
# ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("case", ["A", "B"])
def test_an_episode_does_not_depend_on_E(case):
    base, bcol, bvenv = halting_run(case, 40, None)
    boff, bh = bcol.row_offsets.cpu().numpy(), bvenv.halted()
    assert (bh >= 0).any() and (bh < 0).any()
    for n in (3, 19):
        res, col, venv = halting_run(case, n, None)
        off = col.row_offsets.cpu().numpy()
        np.testing.assert_array_equal(off, boff[:n + 1])
        np.testing.assert_array_equal(venv.halted(), bh[:n])
        for k in KEYS:
            assert torch.equal(res.dataset[k], base.dataset[k][:off[-1]]), (k, n)
        assert torch.equal(col.row_disagreement, bcol.row_disagreement[:off[-1]])
        for x, y in ((venv.state, bvenv.state), (venv.acc, bvenv.acc), (venv.unc, bvenv.unc)):
            assert torch.equal(x, y[:n])


@pytest.mark.parametrize("case", ["A", "G"])
def test_graph_and_eager_runs_agree(case):
    """Noise drawn on device (keyed by episode id and step), so that the run is captured: one 12-launch graph, in which
    an episode that halted at step t is launched 11 - t more times."""
    runs = []
    for use_graph in (True, False):
        venv = make_env(case)
        col = collector(case, venv, "random", use_graph=use_graph)
        res = col.run(noise_std=0.3, gamma=0.9, seed=4)
        assert (col.graph is not None) == use_graph and col.guards_intact()
        again = col.run(noise_std=0.3, gamma=0.9, seed=4)  # the replayed graph, halt_step and the tables used again
        for k in KEYS:
            assert torch.equal(res.dataset[k], again.dataset[k]), k
        runs.append((res, col.row_offsets.clone(), venv.halt_step.clone(), venv.state.clone(), venv.acc.clone(),
                     venv.unc.clone(), col.row_disagreement.clone()))
    h = runs[0][2].cpu().numpy()
    print(f"case {case}: halts at {sorted(h[h >= 0].tolist())}, {int((h < 0).sum())} episodes run to the end")
    assert (h >= 0).any() and (h < 0).any()
    for k in KEYS:
        assert torch.equal(runs[0][0].dataset[k], runs[1][0].dataset[k]), k
    for x, y in zip(runs[0][1:], runs[1][1:]):
        assert torch.equal(x, y)
    np.testing.assert_array_equal(runs[0][0].lengths, np.where(h >= 0, h + 1, T))


def test_evaluate_overshoots_a_halted_episode_without_moving_it():
    """``BatchedRollout`` replays 20-step chunks over 12-step episodes: 8 launches past the end of every episode, up to 19
    past a halt.  Graph and eager agree bit for bit."""
    from osrl_amd.engine.rollout import BatchedRollout
    out = []
    for use_graph in (True, False):
        venv = make_env("B")
        ro = BatchedRollout(policy("B", "random"), venv, "bc", CS, use_graph=use_graph)
        tot = ro.run()
        out.append((tot, venv.state.clone(), venv.acc.clone(), venv.unc.clone(), venv.halt_step.clone()))
    for x, y in zip(out[0][1:], out[1][1:]):
        assert torch.equal(x, y)
    h = out[0][4].cpu().numpy()
    assert (h >= 0).any() and (h < 0).any()
    np.testing.assert_array_equal(out[0][0][2], np.where(h >= 0, h + 1, T))
    thr, umax = np.float32(HC.threshold("B")), out[0][3][:, 0].cpu().numpy()  # (the launch argument is fp32)
    assert (umax[h >= 0] > thr).all() and (umax[h < 0] <= thr).all()


# ------------------------------------------------------------------------------------------------------------------ #
# 4. compaction
# ------------------------------------------------------------------------------------------------------------------ #
def _sentinel_rows(t, n):
    from osrl_amd.engine.collect import _SENTINEL
    return bool((t[n:].contiguous().view(torch.int32) == _SENTINEL).all())


@pytest.mark.parametrize("case,thr", [("A", None), ("B", None), ("G", None), ("A", 0.0), ("B", 1e9)])
def test_dense_rows_are_the_padded_live_rows(case, thr):
    res, col, venv = halting_run(case, E, thr)
    L = venv.acc[:, 2].cpu().numpy().astype(np.int64)
    off = np.concatenate([[0], np.cumsum(L)])
    n = int(off[-1])
    np.testing.assert_array_equal(col.row_offsets.cpu().numpy(), off)
    assert col.row_offsets.dtype == torch.int64 and col.guards_intact()
    if thr == 0.0:
        assert n == E and (venv.halted() == 0).all() and res.dataset["terminals"].all()
    elif thr == 1e9:
        assert n == E * T and (venv.halted() == -1).all() and not res.dataset["terminals"].any()
    else:
        assert E < n < E * T
    live = torch.from_numpy(np.arange(T)[None, :] < L[:, None]).reshape(-1).to(DEV)
    for k in KEYS:
        assert res.dataset[k].shape[0] == n
        assert torch.equal(res.dataset[k], col.tables[k][live]), k
        assert _sentinel_rows(col._dense.tables[k], n), k  # nothing at or past offsets[E] is written
    assert torch.equal(col.row_disagreement, col._row_unc[live]) and _sentinel_rows(col._dense._row_unc, n)
    assert torch.isfinite(res.dataset["rewards"]).all()


def _store(case, n, **kw):
    from osrl_amd.common.replay import ReplayStore
    c = HC.CASES[case]
    return ReplayStore(K.store_rows(n, c["od"], c["ad"]), DEV, seed=3, **kw)


def test_into_a_store_appends_exactly_the_live_rows():
    from osrl_amd.algorithms import BCTrainer
    case, p, cap = "A", 40, 400
    menv = make_env(case)
    tr = BCTrainer(policy(case, "random"), env=menv)
    store = _store(case, p, capacity=cap, pinned_rows=p)
    res = tr.collect_model(menv, horizon=T, start=store, noise_std=0.3, seed=5, into=store)
    col = tr.model_collector(menv)
    n = int(col.row_offsets[-1].item())
    h = menv.halted()
    assert res.dataset is None and (h >= 0).any() and (h < 0).any() and n == int(res.lengths.sum()) < E * T
    np.testing.assert_array_equal(res.lengths, np.where(h >= 0, h + 1, T))
    assert store.n_rows == p + n and int(store._live.item()) == p + n
    assert torch.equal(store.tables[0][p:p + n], col._dense.tables["observations"][:n])
    assert torch.equal(store.tables[0][p + col.row_offsets[:-1]], store.tables[0][col.start_rows])  # the branch starts
    assert (col.start_rows < p).all() and col.guards_intact()
    # the same run as a dataset: the same rows
    again = tr.collect_model(menv, horizon=T, start=store, noise_std=0.3, seed=5)
    assert torch.equal(again.dataset["observations"], store.tables[0][p:p + n])
    # a weighted store takes the scalar; a per-row vector is refused before anything runs
    ws = _store(case, p, capacity=cap, pinned_rows=p, sample_prob=np.ones(p))
    tr.collect_model(menv, horizon=T, start=ws, noise_std=0.3, seed=5, into=ws, sample_prob=3.0)
    assert ws.n_rows == p + n
    with pytest.raises(ValueError, match="can halt"):
        tr.collect_model(menv, horizon=T, start=ws, noise_std=0.3, seed=5, into=ws, sample_prob=np.full(E * T, 3.0))
    assert ws.n_rows == p + n


# ------------------------------------------------------------------------------------------------------------------ #
# 5. trainers
# ------------------------------------------------------------------------------------------------------------------ #
def test_evaluate_of_the_constant_policy_equals_the_oracle():
    from osrl_amd.algorithms import BCTrainer
    case = "B"
    ref = HC.halting_rollout(case, acts="const", cost_scale=1.0)
    menv = make_env(case, thr=HC.threshold(case, "const"))
    r, c, n = BCTrainer(policy(case, "const"), env=menv).evaluate(E)
    np.testing.assert_array_equal(menv.halted(), ref["halt_step"])
    acc = menv.acc.cpu().numpy()
    np.testing.assert_array_equal(acc[:, 2], ref["lengths"])
    close(acc[:, 0], ref["acc"][:, 0], "returns")
    np.testing.assert_array_equal(acc[:, 1], ref["acc"][:, 1])  # (no cost row within 1e-3: tests/test_model_halt_cpu.py)
    close(menv.unc.cpu().numpy(), ref["unc"], "unc")
    assert n == ref["lengths"].mean() and c == ref["acc"][:, 1].mean()
    assert abs(r - ref["acc"][:, 0].mean()) <= BOUND * np.abs(ref["acc"][:, 0]).max()


def test_cdt_evaluate_on_a_halting_environment():
    """The push kernel advances by a global cursor and keeps pushing a halted episode's stale step into that episode's
    own window: the done latch freezes ``acc``, and the other episodes do not see it."""
    from osrl_amd.algorithms import CDT, CDTTrainer
    c = HC.CASES["A"]
    torch.manual_seed(4)
    cdt = CDT(c["od"], c["ad"], 1.0, seq_len=4, episode_len=T, embedding_dim=16, num_layers=1, num_heads=2, device=DEV)
    menv = make_env("A", pess=False)
    tr = CDTTrainer(cdt, env=menv)
    tr.evaluate(E, 10.0, 2.0)
    acc0, unc0, st0 = menv.acc.clone(), menv.unc.clone(), menv.state.clone()
    assert (menv.halted() == -1).all() and (acc0[:, 2] == T).all()
    # (the start rows repeat every 7 episodes and the policy is deterministic: 7 distinct trajectories)
    mx = np.unique(unc0[:, 0].cpu().numpy().astype(np.float64))
    k = mx.size // 2
    thr = float(0.5 * (mx[k - 1] + mx[k]))  # between two per-episode maxima of the free run: about half the episodes halt
    assert mx.size >= 2 and np.float32(mx[k - 1]) < np.float32(thr) < np.float32(mx[k])
    menv.halt_threshold, menv.halt_reward = thr, HC.HALT_REWARD
    r, cost, n = tr.evaluate(E, 10.0, 2.0)
    h = menv.halted()
    free = torch.from_numpy(h < 0).to(DEV)
    assert 0 < int(free.sum()) < E
    for x, y in ((menv.acc, acc0), (menv.unc, unc0), (menv.state, st0)):
        assert torch.equal(x[free], y[free])
    acc = menv.acc.cpu().numpy()
    np.testing.assert_array_equal(acc[h >= 0, 2], h[h >= 0] + 1)
    assert (menv.unc[:, 0].cpu().numpy()[h >= 0] > np.float32(thr)).all() and (acc[:, 3] == 1).all()
    assert n == acc[:, 2].mean() and np.isfinite([r, cost]).all()
    grid = tr.evaluate_targets(E, [(10.0, 2.0)])  # the grid is the same rollout
    assert len(grid) == 1 and np.isfinite(grid[0]).all() and grid[0][2] == n
