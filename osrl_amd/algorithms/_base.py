"""What the six model classes and the five MLP trainers share.  The constructors stay in the algorithm files: their
argument lists and creation order mirror the reference line by line."""
from __future__ import annotations

from importlib import import_module
from typing import Optional

import numpy as np
import torch
import torch.nn as nn


class FlatModel(nn.Module):
    """A model whose parameters are views into flat HBM optimizer groups (``self.groups``)."""

    ENGINE = ""  # "<module under osrl_amd.engine>.<class>" of the training engine

    def repack(self) -> None:
        """Refresh the fragment-ordered weight copies the kernels read; call after modifying parameters
        in place from outside the trainer (load_state_dict does it automatically)."""
        for g in self.groups.values():
            if g.device.type == "cuda":
                g.repack()

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        if assign:
            raise RuntimeError("assign=True would detach parameters from their flat HBM groups")
        res = super().load_state_dict(state_dict, strict=strict)
        self.repack()
        return res

    def _apply(self, fn, *a, **k):  # parameters are views into flat HBM buffers: moving them breaks the engine
        raise RuntimeError("osrl_amd models are bound to their HIP device at construction; .to()/.cuda()/.cpu() "
                           "are unsupported (pass device= to the constructor)")

    def _engine_class(self):
        mod, cls = self.ENGINE.split(".")
        return getattr(import_module("..engine." + mod, __package__), cls)

    def engine(self, batch_size: int, **kw):
        from ..common.checkpoint import engine_handoff
        if self._engine is None or self._engine.B != batch_size or kw:
            if self._lrs is None:
                raise RuntimeError(f"call setup_optimizers() (or build a {type(self).__name__}Trainer) before training")
            old, self._engine = self._engine, self._engine_class()(self, batch_size, **kw)
            engine_handoff(self, self._engine, old)
        return self._engine

    def _policy_spec(self):
        """``(kind, obs_dim, net0, kwargs)`` of the model's ``FastPolicy`` / ``VecFastPolicy``."""
        raise NotImplementedError

    @torch.no_grad()
    def fast_policy(self, num_envs: Optional[int] = None):
        """The B = 1 latency path (engine/act.py): one kernel launch per ``act()``, pinned-memory I/O.
        With ``num_envs`` an integer: the lockstep form for that many host environments (``VecFastPolicy``), built once
        per model and ``num_envs``."""
        if num_envs is not None:
            from ..engine.act import VecFastPolicy, cached_vec_policy

            def make(n):
                kind, obs_dim, net0, kw = self._policy_spec()
                return VecFastPolicy(kind, self.device, obs_dim, self.action_dim, net0, num_envs=n, **kw)
            return cached_vec_policy(self, num_envs, make)
        if getattr(self, "_fast", None) is None:
            from ..engine.act import FastPolicy
            kind, obs_dim, net0, kw = self._policy_spec()
            self._fast = FastPolicy(kind, self.device, obs_dim, self.action_dim, net0, **kw)
        return self._fast


class RolloutMixin:
    """``evaluate`` / ``rollout_many`` / ``rollout`` of the MLP trainers (``self.model``, ``self.env``,
    ``self.reward_scale``, ``self.cost_scale``).  Where a trainer differs from the rest it overrides one of the hooks."""

    EVAL_KIND = ""  # the policy kind of engine/rollout.py ``evaluate_batched``

    def _before_evaluate(self) -> None:
        pass

    def _eval_extra(self) -> Optional[float]:
        """A value appended to every observation the policy sees (None: nothing)."""
        return None

    def _act_for_rollout(self, obs):
        return self.model.act(obs, True, True)[0]

    def _cost_scale(self) -> Optional[float]:
        """Factor on ``info["cost"]`` in the episode sums (None: summed as it is)."""
        return self.cost_scale

    def _scale_results(self, r, c, n):
        return r / self.reward_scale, c / self.cost_scale, n

    def evaluate(self, eval_episodes, schedule: str = "waves"):
        """The reference's ``evaluate``: (mean return, mean cost, mean length).  With a ``VecSyntheticSafeEnv`` as
        ``self.env`` the episodes run as one batch on device (engine/rollout.py); a list or tuple of N host (gym-style)
        environments runs episode ``q`` on environment ``q % N``, N at a time in lockstep (``rollout_many``); any other
        (gym-style) env takes the reference's episode-by-episode loop.  ``schedule`` matters for a list of environments
        only: "waves" (default) starts N episodes and waits for the longest; "refill" gives a slot whose episode ended
        the next episode at once (``rollout_jobs``)."""
        from ..common.synthetic_env import DeviceVecEnv
        from ..engine.act import check_schedule
        check_schedule(schedule)
        self._before_evaluate()
        if isinstance(self.env, DeviceVecEnv):  # (VecSyntheticSafeEnv, or a ModelVecEnv: common/model_env.py)
            from ..engine.rollout import evaluate_batched
            cs = self._cost_scale()
            return self._scale_results(*evaluate_batched(self, self.EVAL_KIND, eval_episodes,
                                                         1.0 if cs is None else cs, self._eval_extra()))
        if isinstance(self.env, (list, tuple)):
            from ..engine.act import evaluate_lockstep, evaluate_refill
            if schedule == "refill":
                return self._scale_results(*evaluate_refill(self, eval_episodes))
            return self._scale_results(*evaluate_lockstep(self, eval_episodes))
        self.model.eval()
        rets, costs, lens = [], [], []
        for _ in range(eval_episodes):
            r, l, c = self.rollout()
            rets.append(r)
            lens.append(l)
            costs.append(c)
        self.model.train()
        return self._scale_results(np.mean(rets), np.mean(costs), np.mean(lens))

    def collect(self, noise_std=0.0, gamma: Optional[float] = None, seed: int = 0, noise=None, into=None):
        """The ``evaluate`` rollout on a ``VecSyntheticSafeEnv``, recorded: every episode of ``self.env`` runs to its end
        with ``a = clip(pi(s) + sigma_e * eps)`` and comes back as a DSRL-layout dataset on device plus the per-episode
        (discounted) returns -- a ``Collected`` (engine/collect.py).  ``noise_std``: one sigma or one per episode;
        ``gamma`` (None: 1) weighs the discounted sums; ``seed`` keys the noise drawn on device; ``noise``
        ``[episode_len, E, action_dim]`` injects it instead.  The policy, the appended cost limit of BC multi-task and
        the cost scale are ``evaluate``'s.  Any other kind of environment: TypeError.  ``into``: a ``ReplayStore`` built
        with ``capacity`` that takes the rows directly (``store.append``: engines attached to it draw from them at their
        next step, nothing is recaptured); the result's ``dataset`` is then None, and a store of other widths (BC
        multi-task) is a ValueError before the run."""
        from ..common.synthetic_env import VecSyntheticSafeEnv
        if not isinstance(self.env, VecSyntheticSafeEnv):
            raise TypeError(f"collect() records the batched on-device rollout: self.env must be a VecSyntheticSafeEnv, "
                            f"not {type(self.env).__name__}")
        self._before_evaluate()
        from ..engine.collect import collect_batched
        cs = self._cost_scale()
        return collect_batched(self, self.EVAL_KIND, 1.0 if cs is None else cs, self._eval_extra(),
                               noise_std=noise_std, gamma=gamma, seed=seed, noise=noise, into=into)

    def collect_model(self, menv, horizon: Optional[int] = None, start=None, noise_std=0.0,
                      gamma: Optional[float] = None, seed: int = 0, noise=None, into=None, sample_prob=None):
        """Rollouts of the current policy on a learned model, recorded (engine/collect.py ``ModelCollector``): every
        episode of the ``ModelVecEnv`` ``menv`` (an argument, not ``self.env``; anything else: TypeError) runs
        ``horizon`` steps (None: ``menv.episode_len``) with ``a = clip(pi(s) + sigma_e * eps)`` and comes back as a
        ``Collected`` of ``E * horizon`` rows, episode-major, under the seven DSRL keys: ``rewards`` after ``menv``'s
        ``reward_penalty``, ``terminals`` 0, ``timeouts`` 1 on each episode's last row.  It is a model's opinion.
        ``start=None``: from ``menv``'s own initial states (a full model episode).  ``start=store`` (a ``ReplayStore``):
        k-step branched rollouts as MOPO / MBPO make them -- every episode starts at a row drawn on device, uniformly,
        from the store's pinned prefix (``pinned_rows > 0``: the real data) or else its live rows, keyed by ``(seed,
        episode id)`` alone; weighted starts are out of scope.  ``noise_std``, ``gamma``, ``seed``, ``noise``
        (``[horizon, E, action_dim]``) as ``collect`` takes them.  The policy, the appended cost limit of BC multi-task
        and the cost scale are ``evaluate``'s.
        ``into``: a ``ReplayStore`` built with ``capacity`` under ``collect``'s width rules; a weighted store is taken
        with ``sample_prob`` (a scalar or ``[E * horizon]``: the new rows' weights, handed to ``append``), a
        ``state_init`` store is refused with ``start=store`` (a branch start is not an initial state).  ValueError
        before anything runs.  ``self.model_collector(menv)`` is the cached collector: its ``start_rows`` and
        ``row_disagreement`` are device tensors of the last run.
        On a ``menv`` with a ``halt_threshold`` an episode ends where the model's uncertainty exceeds it: the result
        holds ``sum(lengths)`` rows, dense and episode-major, a halting row has ``terminals`` 1 and ``timeouts`` 0,
        ``sample_prob`` is a scalar, and the collector's ``row_offsets`` (``[E + 1]``) says where each episode starts."""
        co = self.model_collector(menv)
        self._before_evaluate()
        return co.run(horizon=horizon, start=start, noise_std=noise_std, gamma=gamma, seed=seed, noise=noise, into=into,
                      sample_prob=sample_prob)

    def model_collector(self, menv):
        """The ``ModelCollector`` of ``collect_model`` on ``menv`` (buffers, tables, captured graph), cached on the
        trainer like ``evaluate``'s rollout."""
        from ..engine.collect import ModelCollector
        from ..engine.rollout import cached
        cs = self._cost_scale()
        key = (id(menv), self.EVAL_KIND, 1.0 if cs is None else float(cs), self._eval_extra())
        return cached(self, "_model_collector", key,
                      lambda: ModelCollector(self.model, menv, *key[1:], use_graph=getattr(self, "use_graph", True)))

    def planner(self, menv, num_envs, horizon, noise_std=0.3, gamma=1.0, temperature=0.0, seed=0):
        """A ``ModelPlanner`` (engine/mpc.py) of the current policy on the ``ModelVecEnv`` ``menv``: policy-guided
        shooting at act time.  ``menv.E == num_envs * K``: each of the ``num_envs`` real states handed to
        ``planner.act(states, cost_budget)`` fans out into K imagined episodes of ``horizon`` steps, candidate 0 following
        the policy exactly, the others with ``a = clip(pi(s) + noise_std * eps)``; the action returned is the first
        action of the candidate with the best ``gamma``-discounted penalised return among those whose discounted cost
        (in ``cost_scale`` units) stays within the budget, of the cheapest when none does, or with ``temperature > 0``
        the softmax-weighted mean of the feasible first actions.  The policy, the appended cost limit of BC multi-task
        and the cost scale are ``evaluate``'s.  Anything but a ``ModelVecEnv``: TypeError; a shape that does not fit:
        ValueError, before anything is launched.  The planner is the caller's to keep: it is not cached."""
        from ..engine.mpc import ModelPlanner, check_plan
        check_plan(menv, num_envs, horizon, noise_std, temperature)
        self._before_evaluate()
        cs = self._cost_scale()
        return ModelPlanner(self.model, menv, self.EVAL_KIND, 1.0 if cs is None else float(cs), self._eval_extra(),
                            num_envs=num_envs, horizon=horizon, noise_std=noise_std, gamma=gamma,
                            temperature=temperature, seed=seed, use_graph=getattr(self, "use_graph", True))

    @torch.no_grad()
    def evaluate_planned(self, planner, envs, eval_episodes, cost_limit):
        """``evaluate`` with every action planned: ``eval_episodes`` episodes over the host (gym-style) environments
        ``envs`` (``planner.num_envs`` of them) on the refill schedule, each policy call one ``planner.act`` in which a
        slot's budget is what its episode has left of ``cost_limit`` (``max(cost_limit * cost_scale - cost so far, 0)``;
        engine/act.py ``PlanRefillAdapter``).  Returns ``evaluate``'s (mean return, mean cost, mean length)."""
        from ..engine.act import evaluate_planned
        self._before_evaluate()
        means, _ = evaluate_planned(planner, envs, eval_episodes, cost_limit, self.model.episode_len, self._cost_scale())
        return self._scale_results(*means)

    @torch.no_grad()
    def rollout_many(self, envs, num_slots: Optional[int] = None, episode_ids=None):
        """``rollout`` on each of the host environments ``envs`` at once, in lockstep through
        ``model.fast_policy(num_envs)`` (engine/act.py ``rollout_lockstep``): three arrays (return, length, cost sum), one
        entry per environment.  ``num_slots`` (default ``len(envs)``): the width of the policy to use, the slots past
        ``len(envs)`` idle.  The policy acts deterministically; noise it still draws on the device (BCQ-L's decode
        noise z) is keyed by the episode id (``episode_ids``, default 0 .. len(envs) - 1) and the step.  BC in
        ``multi-task`` mode appends the cost limit to every observation (``_eval_extra``)."""
        from ..engine.act import rollout_lockstep
        return rollout_lockstep(self.model, envs, num_slots, episode_ids, cost_scale=self._cost_scale(),
                                append=self._eval_extra())

    @torch.no_grad()
    def rollout_jobs(self, envs, num_jobs, episode_ids=None):
        """``num_jobs`` episodes over the host environments ``envs`` on the refill schedule (engine/act.py
        ``rollout_refill``): job ``q`` starts in slot ``q`` while slots are free, and a slot whose episode has ended takes
        the next job in the policy call in which the others step.  Returns a ``RefillResult``: per job (return, length,
        cost sum) and the slot it ran in, and the number of policy calls.  Job ``q`` has episode id ``episode_ids[q]``
        (default ``q``) and equals that episode run alone through ``rollout_many`` on the same environment."""
        from ..engine.act import rollout_jobs_mlp
        return rollout_jobs_mlp(self.model, envs, num_jobs, episode_ids, cost_scale=self._cost_scale(),
                                append=self._eval_extra())

    @torch.no_grad()
    def collect_jobs(self, envs, num_jobs, noise_std=0.0, gamma: Optional[float] = None, seed: int = 0, noise=None,
                     episode_ids=None, into=None):
        """``rollout_jobs`` recorded, with exploration noise: ``num_jobs`` episodes over the host (gym-style) environments
        ``envs`` on the refill schedule, every action ``a = clip(pi(s) + sigma_q * eps, +-max_action)`` computed by the
        policy call itself (``VecFastPolicy.step(explore_std=...)``), every transition kept -- what ``collect`` does on a
        ``VecSyntheticSafeEnv``, for real simulators.  Returns a ``Collected`` (engine/collect.py) whose rows are
        job-major, each job with its true length (``terminals`` 1 where the environment terminated, ``timeouts`` 1 where
        it truncated or reached ``episode_len``; ``observations`` are the environment's own, without BC multi-task's
        appended cost limit) and whose dataset is on the device (one upload at the end).
        ``noise_std``: one sigma or one per job; ``gamma`` (None: 1) weighs the discounted sums; job ``q``'s noise is
        keyed by ``(seed, episode_ids[q], step, column)`` -- the device collectors' key, ``episode_ids`` defaulting to
        ``q`` -- or injected as ``noise [num_jobs, episode_len, action_dim]``.  With ``noise_std=0`` job ``q`` is
        ``rollout_jobs``'s, bit for bit.  ``into``: a ``ReplayStore`` built with ``capacity`` (``collect``'s rules), or a
        ``SequenceStore`` built with capacities, refused BEFORE the run unless ``num_jobs`` trajectories of
        ``episode_len`` rows fit; the rows go to its ``append`` and the result's ``dataset`` is None."""
        from ..engine.act import collect_jobs_mlp
        self._before_evaluate()
        return collect_jobs_mlp(self.model, envs, num_jobs, noise_std, gamma, seed, noise, episode_ids, into,
                                cost_scale=self._cost_scale(), append=self._eval_extra())

    @torch.no_grad()
    def rollout(self):
        """The reference's episode loop on ``self.env``: (return, length, cost sum)."""
        cs, extra = self._cost_scale(), self._eval_extra()
        put = (lambda o: o) if extra is None else (lambda o: np.append(o, extra))  # noqa: E731
        obs, info = self.env.reset()
        obs = put(obs)
        ep_ret, ep_cost, ep_len = 0.0, 0.0, 0
        for _ in range(self.model.episode_len):
            act = self._act_for_rollout(obs)
            obs_next, reward, terminated, truncated, info = self.env.step(act)
            obs = put(obs_next)
            ep_ret += reward
            ep_len += 1
            ep_cost += info["cost"] if cs is None else info["cost"] * cs
            if terminated or truncated:
                break
        return ep_ret, ep_len, ep_cost
