"""Planning at act time: policy-guided shooting on the learned model (MBOP's rule; DESIGN.md "Planning at act time").

``ModelPlanner`` is a ``ModelCollector`` (engine/collect.py) whose run starts at N REAL states instead of the environment's
own: every state ("slot") fans out into K imagined episodes (csrc/plan.hip ``osrl_plan_fanout``; episode ``n * K + k`` is
candidate k of slot n), the collector's recorded step runs H times -- the policy's launches, ``a = clip(pi(s) + sigma_e *
eps)``, the recording ``osrl_model_env_step`` with whatever pessimism the environment carries (``reward_penalty``, ``cost_penalty``,
``halt_threshold``) -- and ``osrl_plan_select`` picks one candidate per slot from the discounted sums the recorder keeps:
the best penalised return among those whose discounted cost stays inside the slot's remaining budget, the cheapest one
when none does, or with ``temperature > 0`` the softmax average of the feasible first actions (MPPI).

``terminal=`` (an ``FQE`` or ``FQETrainer`` fitted for the same policy) closes the H-step sums with a value at the horizon:
one more launch, ``osrl_plan_terminal`` (csrc/plan_value.hip), between the last recorded step and the select adds
``gamma^H Q_r(s_H, pi(s_H))`` to every candidate's return and ``gamma^H Q_c(s_H, pi(s_H))`` to its cost, so that ``C_k <=
budget`` compares like with like: the whole remaining episode (DESIGN.md "Terminal value at the horizon").  A quantile
FQE (``FQE(num_quantiles=M)``) takes ``osrl_plan_terminal_quantile`` (csrc/plan_value_quantile.hip) in that launch's place:
with ``risk_alpha=(alpha_reward, alpha_cost)`` the return is closed with the mean of the ``ceil(alpha_reward M)`` LOWEST
quantiles of each candidate's own end state and the cost with the mean of the ``ceil(alpha_cost M)`` HIGHEST -- the budget
then bounds the upper-tail CVaR of the cost-to-go (DESIGN.md "A distributional terminal value").

Candidate 0 of every slot has sigma = 0: the policy's own proposal is always among the candidates.  The noise is the
collectors' (Philox stream 13, keyed by seed word, episode id ``base_seed + n * K + k``, the episode's step and the action
column) and the model's steps do not depend on their tile neighbours, so a slot's action is a function of its own state
and budget, the weights, the seed and the call number -- not of N, the slot's position aside, nor of the other slots.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from .. import _lib as L
from .collect import ModelCollector
from .core import cur_stream
from .rollout import _CHUNK


def check_plan(venv, num_envs, horizon, noise_std=0.0, temperature=0.0) -> int:
    """A planner's shape, judged on the host before anything is built or launched: the candidates per slot K.  TypeError
    for anything but a ``ModelVecEnv``; ValueError unless ``venv.E == num_envs * K`` with ``1 <= K <=
    PLAN_MAX_CANDIDATES``, ``horizon >= 1``, and ``noise_std`` / ``temperature`` are finite and not negative."""
    from ..common.model_env import ModelVecEnv
    if not isinstance(venv, ModelVecEnv):
        raise TypeError(f"a planner imagines on a learned model: a ModelVecEnv, not {type(venv).__name__}")
    N, H = int(num_envs), int(horizon)
    if N < 1:
        raise ValueError(f"num_envs {N}: at least one slot")
    if H < 1:
        raise ValueError(f"horizon {H}: at least one step")
    if venv.E % N != 0:
        raise ValueError(f"the model environment holds {venv.E} episodes, no multiple of num_envs = {N}: build it with "
                         f"episodes = num_envs * candidates")
    K = venv.E // N
    if K > L.PLAN_MAX_CANDIDATES:
        raise ValueError(f"{K} candidates per slot: at most {L.PLAN_MAX_CANDIDATES}")
    for name, x in (("noise_std", noise_std), ("temperature", temperature)):
        if not (0.0 <= float(x) < math.inf):
            raise ValueError(f"{name} {x}: a finite value >= 0")
    return K


def check_refine(K, kind="bc", z=None, refine_rounds=0, num_elites=None, refine_momentum=0.0, min_std=0.05) -> int:
    """A planner's CEM keywords, judged on the host before anything is built or launched: the elite count
    (``num_elites=None``: ``max(1, K // 10)``).  ValueError for ``refine_rounds < 0`` (or beyond the 65535 the draw's
    counter word holds), ``num_elites`` outside ``[1, K]``, a momentum outside ``[0, 1)``, a ``min_std`` that is negative
    or not finite, and with ``refine_rounds > 0``: ``K < 3`` (candidate 0 is the policy and candidate 1 the mean plan:
    nothing would be drawn) and BCQ-L with unfixed ``z`` (its decode noise has the seed as a by-value launch argument, so
    every call captures anew: the rounds would replay a graph that each call has to drop)."""
    R, K = int(refine_rounds), int(K)
    if not (0 <= R <= 65535):
        raise ValueError(f"refine_rounds {refine_rounds}: 0 .. 65535")
    ne = max(1, K // 10) if num_elites is None else int(num_elites)
    if not (1 <= ne <= K):
        raise ValueError(f"num_elites {num_elites}: between 1 and the {K} candidates per slot")
    if not (0.0 <= float(refine_momentum) < 1.0):
        raise ValueError(f"refine_momentum {refine_momentum}: in [0, 1)")
    if not (0.0 <= float(min_std) < math.inf):
        raise ValueError(f"min_std {min_std}: a finite value >= 0")
    if R > 0 and K < 3:
        raise ValueError(f"refine_rounds > 0 with {K} candidates per slot: candidate 0 is the policy's proposal and "
                         f"candidate 1 the mean plan, at least one more has to be drawn")
    if R > 0 and kind == "bcql" and z is None:
        raise ValueError("refine_rounds > 0 with BCQ-L needs a fixed z: with drawn decode noise every call captures anew")
    return ne


class Terminal(NamedTuple):
    """What ``check_terminal`` hands the planner: the ``FQE``, the scales its critics were fitted under and the member
    reduction as ``osrl_plan_terminal`` takes it; for a quantile FQE ``risk_alpha`` is the pair ``(alpha_reward,
    alpha_cost)``, otherwise None."""
    fqe: object
    reward_scale: float
    cost_scale: float
    reduce: int
    risk_alpha: Optional[tuple] = None


def check_risk_alpha(risk_alpha, M: int):
    """``risk_alpha`` of a quantile terminal with ``M`` quantiles as ``((alpha_reward, alpha_cost), (k_r, k_c))``: a float
    stands for both, None for ``(1.0, 1.0)`` (the quantile means); ``k`` by ``estimate_risk``'s rule (algorithms/fqe.py
    ``tail_count``: ValueError for an alpha outside (0, 1])."""
    from ..algorithms.fqe import tail_count
    if risk_alpha is None:
        risk_alpha = 1.0
    pair = tuple(risk_alpha) if isinstance(risk_alpha, (tuple, list)) else (risk_alpha, risk_alpha)
    if len(pair) != 2:
        raise ValueError(f"risk_alpha {risk_alpha!r}: a float or a pair (alpha_reward, alpha_cost)")
    pair = (float(pair[0]), float(pair[1]))
    return pair, (tail_count(pair[0], M), tail_count(pair[1], M))


def check_terminal(model, venv, kind: str, terminal, gamma, value_reduce: str = "mean",
                   extra_obs: Optional[float] = None, risk_alpha=None) -> Optional[Terminal]:
    """A planner's ``terminal=`` / ``value_reduce=`` / ``risk_alpha=``, judged on the host before anything is built or launched; None
    without a terminal.  TypeError for anything but an ``FQE`` / ``FQETrainer``, a ``venv`` that is no ``ModelVecEnv``
    and BCQ-L (its action at the horizon needs decode noise, and the planner has no fixed ``z`` for it); ValueError for another ``value_reduce``, an FQE
    fitted for another policy object, on another device or for other state / action widths, a ``gamma`` that is not the
    FQE's (a value discounted at another rate cannot be added to these sums), ``gamma >= 1`` on an environment that can
    halt (the absorbing state's tail ``1 / (1 - gamma)`` does not exist), a trainer with an extra observation column (BC
    multi-task: FQE refuses it too), widths the kernel does not take, a ``risk_alpha`` outside (0, 1] and a ``risk_alpha``
    without quantile critics to take a tail of (a scalar FQE, no terminal)."""
    from ..algorithms.fqe import FQE, FQETrainer, _device_key
    if value_reduce not in L.PLAN_REDUCE:
        raise ValueError(f"value_reduce {value_reduce!r}: one of {sorted(L.PLAN_REDUCE)}")
    if terminal is None:
        if risk_alpha is not None:
            raise ValueError("risk_alpha= without terminal=: the tail is taken over a quantile FQE's outputs")
        return None
    if isinstance(terminal, FQETrainer):
        fqe, rs, cs = terminal.model, float(terminal.reward_scale), float(terminal.cost_scale)
    elif isinstance(terminal, FQE):
        fqe, rs, cs = terminal, 1.0, 1.0
    else:
        raise TypeError(f"terminal= takes an FQE or an FQETrainer, not {type(terminal).__name__}")
    from ..common.model_env import ModelVecEnv
    if not isinstance(venv, ModelVecEnv):  # (check_plan's refusal, for a caller that comes here alone)
        raise TypeError(f"terminal= is judged against a ModelVecEnv, not {type(venv).__name__}")
    alphas, M = None, getattr(fqe, "num_quantiles", None)
    if M is not None:
        alphas, _ = check_risk_alpha(risk_alpha, M)
    elif risk_alpha is not None:
        raise ValueError("risk_alpha= with a scalar FQE: build the terminal with FQE(num_quantiles=M)")
    if kind == "bcql":
        raise TypeError("terminal= with BCQ-L: its action at the horizon needs decode noise, out of scope")
    if extra_obs is not None:
        raise ValueError("terminal= with an extra observation column (BC multi-task): FQE does not take such a policy")
    if fqe.policy is not model:
        raise ValueError("terminal=: the FQE was fitted for another policy object than the trainer's model")
    if _device_key(fqe.device) != _device_key(model.device):
        raise ValueError(f"terminal=: the FQE lives on {fqe.device!r}, the policy on {model.device!r}")
    if (int(fqe.state_dim), int(fqe.action_dim)) != (int(venv.state_dim), int(model.action_dim)):
        raise ValueError(f"terminal=: the FQE takes ({fqe.state_dim}, {fqe.action_dim})-wide states and actions, the planner "
                         f"has ({venv.state_dim}, {model.action_dim})")
    if float(gamma) != float(fqe.gamma):
        raise ValueError(f"terminal=: the planner discounts at gamma = {float(gamma)}, the FQE at {float(fqe.gamma)}")
    if float(gamma) >= 1.0 and venv.can_halt:
        raise ValueError("terminal= on an environment that can halt needs gamma < 1: a halted candidate carries the "
                         "absorbing state's tail 1 / (1 - gamma)")
    if not (rs != 0.0 and cs != 0.0 and math.isfinite(rs) and math.isfinite(cs)):
        raise ValueError(f"terminal=: reward_scale {rs} / cost_scale {cs} must be finite and non-zero")
    if max(fqe.c_hidden_sizes) > L.PLAN_TERMINAL_NARROW and fqe.state_dim + fqe.action_dim > L.PLAN_TERMINAL_WIDE_INPUT:
        raise ValueError(f"terminal=: critics wider than {L.PLAN_TERMINAL_NARROW} take states and actions of at most "
                         f"{L.PLAN_TERMINAL_WIDE_INPUT} columns together")
    return Terminal(fqe, rs, cs, L.PLAN_REDUCE[value_reduce], alphas)


def check_budget(cost_budget, num_envs: int) -> np.ndarray:
    """``act``'s ``cost_budget`` as fp32 ``[num_envs]``: one value for every slot or one per slot (ValueError for another
    length).  In the collector's ``cost_scale`` units, like the discounted cost it is compared with."""
    if torch.is_tensor(cost_budget):
        cost_budget = cost_budget.detach().cpu().numpy()
    b = np.asarray(cost_budget, dtype=np.float32)
    if b.ndim == 0:
        return np.full(int(num_envs), b, np.float32)
    b = b.reshape(-1)
    if b.size != int(num_envs):
        raise ValueError(f"cost_budget holds {b.size} values, the planner {int(num_envs)} slots")
    return b


def check_states(states, num_envs: int, state_dim: int) -> np.ndarray:
    """``act``'s ``states`` as fp32 ``[num_envs, state_dim]`` on the host; ValueError for another shape."""
    if torch.is_tensor(states):
        states = states.detach().cpu().numpy()
    s = np.asarray(states, dtype=np.float32)
    if s.shape != (int(num_envs), int(state_dim)):
        raise ValueError(f"states must be [{int(num_envs)}, {int(state_dim)}], got {s.shape}")
    return s


class ModelPlanner(ModelCollector):
    """``act(states [N, od], cost_budget)`` -> ``[N, ad]`` actions (numpy): upload, fan-out, H recorded model steps (one
    captured graph of ``min(H, _CHUNK)`` steps, replayed in chunks beyond that), select, one host sync.  Nothing is
    compacted and nothing appended to a store: on an environment that can halt, a halted candidate simply stops adding to
    its sums (and counts with ``halt_reward`` / ``halt_cost``).

    The seed word of call number c is ``seed + c`` -- device memory, so the graph is captured once; ``reset_calls()``
    starts the count again.  ``temperature`` is a device word too and may be set between calls.  BCQ-L with unfixed ``z``
    does what ``ModelCollector`` does today: its decode noise has the seed as a by-value launch argument, so every call
    (a new seed) drops the graph and captures again; pass ``z`` for a planner that keeps its graph.

    Of the last call, on the device: ``last_J`` / ``last_C`` ``[N, K]`` (discounted penalised return and discounted cost
    of every candidate, the latter in ``cost_scale`` units), ``last_first_actions`` ``[N, K, ad]``, ``chosen`` ``[N]``
    (int32: the arg-best candidate, under MPPI too) and ``n_feasible`` ``[N]``.  The first three are views of the
    planner's tables: the next call overwrites them.

    ``terminal`` (``check_terminal``: an ``FQE`` / ``FQETrainer`` of this very policy, same ``gamma``) adds the value at the
    horizon in one launch before the select (csrc/plan_value.hip).  ``last_J`` / ``last_C`` then INCLUDE the terminal
    terms: ``J += g Vr``, ``C += g Vc`` with ``g = gamma^H``, ``Vr = reduce_m Q_r,m(s_H, pi(s_H)) / reward_scale`` and ``Vc =
    reduce_m Q_c,m(s_H, pi(s_H)) * cost_scale / FQE cost_scale`` (``value_reduce``: "mean" over the members, or
    "pessimistic" = the lowest return and the highest cost); ``last_V`` ``[N, K, 2]`` holds ``(Vr, Vc)``.  A candidate that
    halted carries the absorbing state's tail instead: ``halt_reward / (1 - gamma)`` and ``halt_cost * cost_scale / (1 -
    gamma)``, times its own ``g`` -- walking into the model's ignorance must not look cheaper than staying out of it.
    Without ``terminal`` the planner issues exactly the launches it issued before, and ``last_V`` is None.

    A quantile ``terminal`` (``FQE(num_quantiles=M)``) with ``risk_alpha = (alpha_reward, alpha_cost)`` (a float: both; None:
    1.0, the quantile means): per member and candidate the ``M`` outputs at ``(s_H, pi(s_H))`` are sorted, ``Q_r,m`` above
    becomes the mean of the ``k_r = ceil(alpha_reward M)`` smallest and ``Q_c,m`` the mean of the ``k_c = ceil(alpha_cost
    M)`` largest (``estimate_risk``'s rule), and everything else reads as above: ``last_V`` holds these CVaR values,
    ``last_V_mean`` ``[N, K, 2]`` the same reduction of the all-``M`` means (diagnostics; None otherwise).  A NaN among a
    member's quantiles makes that member's values NaN, and the select skips such a candidate.  ``risk_alpha`` may be set
    between calls: the terminal launch lies outside the captured graph, nothing is recaptured.  The H imagined steps
    themselves stay risk-neutral; crossing quantiles are not prevented; FQE's extrapolation error applies to each.

    ``refine_rounds = R > 0`` (``check_refine``; DESIGN.md "CEM refinement"): the call looks R + 1 times.  The planner owns
    a noise table ``eps [H, E, ad]`` that the recorded steps read in the drawn noise's place (``osrl_collect_t.eps_in``:
    ``a = clip(pi(s) + noise_std * eps)``), and a sampling distribution ``plan_mean`` / ``plan_std`` ``[N, H, ad]`` in units
    of ``eps``.  A call sets them to 0 and 1 and fills the table with standard normals (csrc/plan_refine.hip
    ``osrl_plan_refit``, round 0); every round is the fan-out, the H recorded steps (the captured graph, replayed) and the
    terminal launch; between two rounds ``osrl_plan_refit`` ranks each slot's candidates by the select's own order, fits
    mean and standard deviation of the ``num_elites`` best ones' table entries, mixes them in with ``refine_momentum``,
    floors the deviation at ``min_std`` and redraws the table: candidate 0 stays the policy, candidate 1 is the refitted
    mean plan, the others ``mean + std * z``.  The select runs once, on the last round's candidates: ``last_J`` /
    ``last_C`` / ``last_V`` / ``last_first_actions`` / ``chosen`` / ``n_feasible`` describe that round, ``last_eps`` ``[H, N,
    K, ad]`` is its table and ``elite_rank`` ``[N, K]`` (int32, 0 = best) the last refit's ranking.  Still one upload and
    one host sync per call; ``num_elites``, ``refine_momentum`` and ``min_std`` are by-value arguments of the refit launch,
    outside the graph, and may be set between calls.  Not done: warm-starting the mean from the previous call's shifted
    plan, time-correlated noise, keeping elites across rounds, CDT, data parallelism.  With ``refine_rounds=0`` the
    planner issues exactly the launches it issued before, builds no table, and the four attributes are None."""

    def __init__(self, model, venv, kind: str, cost_scale: float = 1.0, extra_obs: Optional[float] = None,
                 num_envs: int = 1, horizon: int = 1, noise_std: float = 0.3, gamma: float = 1.0,
                 temperature: float = 0.0, seed: int = 0, z: Optional[torch.Tensor] = None, use_graph: bool = True,
                 terminal=None, value_reduce: str = "mean", risk_alpha=None, refine_rounds: int = 0, num_elites=None,
                 refine_momentum: float = 0.0, min_std: float = 0.05):
        K = check_plan(venv, num_envs, horizon, noise_std, temperature)  # (before any device work)
        term = check_terminal(model, venv, kind, terminal, gamma, value_reduce, extra_obs, risk_alpha)
        n_elite = check_refine(K, kind, z, refine_rounds, num_elites, refine_momentum, min_std)
        if int(refine_rounds) > 0 and int(horizon) > L.PLAN_REFINE_MAX_HORIZON:
            raise ValueError(f"refine_rounds > 0 with horizon {horizon}: at most {L.PLAN_REFINE_MAX_HORIZON}")
        super().__init__(model, venv, kind, cost_scale, extra_obs, seed, z, use_graph)
        N, od, ad, dev = int(num_envs), venv.state_dim, model.action_dim, self.obs.device
        self.num_envs, self.candidates, self.horizon = N, K, int(horizon)
        self.noise_std, self.plan_gamma, self.base_plan_seed, self.calls = float(noise_std), float(gamma), int(seed), 0
        sg = torch.full((N, K), self.noise_std, dtype=torch.float32)
        sg[:, 0] = 0.0  # candidate 0: the policy's own proposal
        self._sigma_plan = sg.reshape(-1).to(dev)
        self._host_in = torch.zeros(N * (od + 1), dtype=torch.float32).pin_memory()  # states, then budgets: one upload
        self._dev_in = torch.zeros(N * (od + 1), dtype=torch.float32, device=dev)
        self._states, self._budget = self._dev_in[:N * od].view(N, od), self._dev_in[N * od:]
        self._temperature = torch.zeros(1, dtype=torch.float32, device=dev)
        self.temperature = temperature
        self.action = torch.zeros(N, ad, dtype=torch.float32, device=dev)
        self.chosen = torch.zeros(N, dtype=torch.int32, device=dev)
        self.n_feasible = torch.zeros(N, dtype=torch.int32, device=dev)
        self.terminal, self._last_V, self._last_V_mean, self._risk_alpha = term, None, None, None
        if term is not None:
            self._build_terminal()
        self.refine_rounds, self.num_elites = int(refine_rounds), n_elite
        self.refine_momentum, self.min_std = float(refine_momentum), float(min_std)
        self.plan_mean = self.plan_std = self._eps_table = self.elite_rank = None
        if self.refine_rounds > 0:  # (fixed addresses for the planner's lifetime: the graph is captured with eps_in set)
            H = self.horizon
            self._eps_table = torch.zeros(H, N * K, ad, dtype=torch.float32, device=dev)
            self.plan_mean = torch.zeros(N, H, ad, dtype=torch.float32, device=dev)
            self.plan_std = torch.ones(N, H, ad, dtype=torch.float32, device=dev)
            self.elite_rank = torch.zeros(N, K, dtype=torch.int32, device=dev)

    @property
    def last_eps(self) -> Optional[torch.Tensor]:
        """``[H, N, K, ad]``: the noise table the last round ran on (candidate 0's rows are unread); None without
        ``refine_rounds``."""
        t = self._eps_table
        return None if t is None else t.view(self.horizon, self.num_envs, self.candidates, t.shape[-1])

    def _alloc(self, steps: int) -> None:
        super()._alloc(steps)
        if self._eps_table is not None:  # (every recorded step of this planner, captured or not, reads the table)
            self.rec.eps_in = self._eps_table.data_ptr()

    def _refit(self, rnd: int) -> None:
        L.check(L.load().osrl_plan_refit(
            self.disc.data_ptr(), self._budget.data_ptr(), self._eps_table.data_ptr(), self.plan_mean.data_ptr(),
            self.plan_std.data_ptr(), self.num_envs, self.candidates, self.horizon, self.model.action_dim, self.num_elites,
            self.refine_momentum, self.min_std, rnd, self.seed_dev.data_ptr(), self.venv.base_seed & 0xFFFFFFFF, None,
            self.elite_rank.data_ptr(), cur_stream()), "osrl_plan_refit")

    def _build_terminal(self) -> None:
        """The descriptors ``osrl_plan_terminal`` / ``osrl_plan_terminal_quantile`` read: the policy's (the act paths' ``osrl_policy_t``) and the 2 num_q
        online critics', reward members first.  They point at the packed copies, which the fused Adam step keeps current;
        ``repack`` here covers parameters edited from outside a trainer."""
        from ..common.net import net_desc_seq
        from .act import _gemv_net, _policy_desc
        fqe, m = self.terminal.fqe, self.model
        fqe.repack()
        m.repack()
        pk, obs_dim, net0, kw = m._policy_spec()  # (max_action: the model's for "cpq", 1 for "dice", unread for "bc")
        self._term_policy = _policy_desc(pk, obs_dim, m.action_dim, net0, kw["max_action"], None, 0, 0.0)
        nets = [net_desc_seq([q], 1.0) for q in list(fqe.critic.q_nets) + list(fqe.cost_critic.q_nets)]
        self._term_critics = (L.GemvNetT * len(nets))()
        for dst, nd in zip(self._term_critics, nets):
            _gemv_net(dst, nd)
        self._term_keep = (net0, nets)  # the descriptors hold the parameter views alive
        self._last_V = torch.zeros(self.venv.E, 2, dtype=torch.float32, device=self.obs.device)
        if fqe.num_quantiles is not None:
            self._last_V_mean = torch.zeros_like(self._last_V)
            self.risk_alpha = self.terminal.risk_alpha

    @property
    def last_V(self) -> Optional[torch.Tensor]:
        """``[N, K, 2]``: ``(Vr, Vc)`` of every candidate at the horizon, scaled as they enter ``last_J`` / ``last_C``
        (a halted candidate's critics' values too, though its sums took the halting tail); None without ``terminal``."""
        return None if self._last_V is None else self._last_V.view(self.num_envs, self.candidates, 2)

    @property
    def last_V_mean(self) -> Optional[torch.Tensor]:
        """``[N, K, 2]``: ``last_V`` with every member's mean over its ``M`` quantiles in the tail mean's place (the
        risk-neutral value; it enters no sum); None unless ``terminal`` is a quantile FQE."""
        return None if self._last_V_mean is None else self._last_V_mean.view(self.num_envs, self.candidates, 2)

    @property
    def risk_alpha(self) -> Optional[tuple]:
        """``(alpha_reward, alpha_cost)`` of a quantile terminal, None otherwise."""
        return self._risk_alpha

    @risk_alpha.setter
    def risk_alpha(self, v) -> None:
        if self._last_V_mean is None:
            raise ValueError("risk_alpha needs a quantile terminal: planner(terminal=<FQE(num_quantiles=M)>)")
        self._risk_alpha, self._tails = check_risk_alpha(v, self.terminal.fqe.num_quantiles)  # (by value at the launch)

    def _terminal(self) -> None:
        t, v, g = self.terminal, self.venv, self.plan_gamma
        halt_r = halt_c = 0.0
        if v.can_halt:
            halt_r, halt_c = v.halt_reward / (1.0 - g), v.halt_cost * self.cost_scale / (1.0 - g)
        tail = (self.obs.data_ptr(), self.obs.stride(0), v.E, 1.0 / t.reward_scale, self.cost_scale / t.cost_scale, halt_r,
                halt_c, v.halt_step.data_ptr() if v.can_halt else None, self.disc.data_ptr(), self._last_V.data_ptr())
        if t.fqe.num_quantiles is None:
            L.check(L.load().osrl_plan_terminal(self._term_policy, self._term_critics, t.fqe.num_q, t.reduce, *tail,
                                                cur_stream()), "osrl_plan_terminal")
        else:
            L.check(L.load().osrl_plan_terminal_quantile(
                self._term_policy, self._term_critics, t.fqe.num_q, t.fqe.num_quantiles, *self._tails, t.reduce, *tail,
                self._last_V_mean.data_ptr(), cur_stream()), "osrl_plan_terminal_quantile")

    @property
    def temperature(self) -> float:
        return self._temp_host

    @temperature.setter
    def temperature(self, v: float) -> None:
        if not (0.0 <= float(v) < math.inf):
            raise ValueError(f"temperature {v}: a finite value >= 0")
        self._temp_host = float(v)
        self._temperature.fill_(float(v))  # (device memory: a captured launch would follow)

    def reset_calls(self) -> None:
        """The next ``act`` is call number 0 again: it draws the first call's noise."""
        self.calls = 0

    @property
    def last_J(self) -> torch.Tensor:
        return self.disc[:, 0].view(self.num_envs, self.candidates)

    @property
    def last_C(self) -> torch.Tensor:
        return self.disc[:, 1].view(self.num_envs, self.candidates)

    @property
    def last_first_actions(self) -> torch.Tensor:
        ad = self.model.action_dim
        return self.tables["actions"].view(self.num_envs, self.candidates, self.horizon, ad)[:, :, 0]

    def run(self, *a, **kw):
        raise TypeError("a ModelPlanner plans (act); record rollouts with the trainer's collect_model")

    def _fanout(self) -> None:
        v = self.venv
        L.check(L.load().osrl_plan_fanout(
            self._states.data_ptr(), self.num_envs, self.candidates, v.state_dim, v.state.data_ptr(), self.obs.data_ptr(),
            self.obs.stride(0), v.acc.data_ptr(), v.unc.data_ptr(), self.disc.data_ptr(),
            v.halt_step.data_ptr() if v.can_halt else None, cur_stream()), "osrl_plan_fanout")

    def _select(self) -> None:
        L.check(L.load().osrl_plan_select(
            self.tables["actions"].data_ptr(), self.horizon, self.disc.data_ptr(), self._budget.data_ptr(),
            self._temperature.data_ptr(), self.num_envs, self.candidates, self.model.action_dim, self.action.data_ptr(),
            self.chosen.data_ptr(), self.n_feasible.data_ptr(), cur_stream()), "osrl_plan_select")

    @torch.no_grad()
    def act(self, states, cost_budget) -> np.ndarray:
        """``states``: ``[N, od]`` (array or tensor); ``cost_budget``: a float or ``[N]``, each slot's remaining budget in
        ``cost_scale`` units.  Every refusal comes before the first launch."""
        N, od, H, R = self.num_envs, self.venv.state_dim, self.horizon, self.refine_rounds
        s, b = check_states(states, N, od), check_budget(cost_budget, N)
        if R > 0:  # (the three may have been set since the last call)
            self.num_elites = check_refine(self.candidates, self.kind, True, R, self.num_elites, self.refine_momentum,
                                           self.min_std)
        host = self._host_in.numpy()
        host[:N * od], host[N * od:] = s.reshape(-1), b
        seed = (self.base_plan_seed + self.calls) & 0xFFFFFFFFFFFFFFFF
        self._begin(H, seed, self._sigma_plan, self.plan_gamma, None)
        self._dev_in.copy_(self._host_in, non_blocking=True)
        if R > 0:
            self._refit(0)
        for r in range(R + 1):  # (the fan-out resets the sums the recorder keeps, disc included)
            self._fanout()
            self._drive_recorded(H, min(H, _CHUNK), None)
            if self.terminal is not None:
                self._terminal()
            if r < R:
                self._refit(r + 1)
        self._select()
        self.calls += 1
        return self.action.cpu().numpy()
