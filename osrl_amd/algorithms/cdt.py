"""Constrained Decision Transformer on MI355X behind the reference's API (osrl/algorithms/cdt.py).

``CDT`` keeps the constructor and ``state_dict`` layout of cdt.py:45-164 (the same torch container modules
are created in the same order, so a seeded construction reproduces the reference's initial weights);
``CDTTrainer.train_one_step`` keeps the signature of cdt.py:343.  Supported configuration = the reference's
every constructor variant of cdt.py:45-141: any subset of the return / cost tokens, with or without the timestep
embedding, the cost-prefix token, the add / mul / cat cost features on the state feature, deeper action heads,
stochastic or deterministic, dropout.  Limits: <= 1024 tokens per sequence (seq_repeat * seq_len + cost_prefix),
embedding_dim <= 1024 with head_dim = embedding_dim / num_heads <= 128; past them the constructor raises
NotImplementedError naming the limit.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from ..common.logger import store_stats
from ..common.net import DiagGaussianActor, TransformerBlock, bind_group, mlp, plan_group
from ..engine.core import FlatGroup, require_cuda
from ._base import FlatModel


class _Params(nn.Module):
    """Holds the reference-named submodules so that plan_group/bind_group see keys without a prefix."""


class CDT(FlatModel):
    def __init__(self, state_dim: int, action_dim: int, max_action: float, seq_len: int = 10,
                 episode_len: int = 1000, embedding_dim: int = 128, num_layers: int = 4, num_heads: int = 8,
                 attention_dropout: float = 0.0, residual_dropout: float = 0.0, embedding_dropout: float = 0.0,
                 time_emb: bool = True, use_rew: bool = False, use_cost: bool = False, cost_transform: bool = False,
                 add_cost_feat: bool = False, mul_cost_feat: bool = False, cat_cost_feat: bool = False,
                 action_head_layers: int = 1, cost_prefix: bool = False, stochastic: bool = False,
                 init_temperature=0.1, target_entropy=None, device: str = "cuda", differentiable: bool = False):
        super().__init__()
        unsupported = []
        if not all(0.0 <= p < 1.0 for p in (attention_dropout, residual_dropout, embedding_dropout)):
            raise ValueError("dropout probabilities must be in [0, 1)")
        if action_head_layers < 1:
            raise ValueError("action_head_layers must be >= 1")
        seq_repeat = 2 + int(bool(use_cost)) + int(bool(use_rew))  # cdt.py:96-105
        S = seq_repeat * seq_len + int(bool(cost_prefix))           # cdt.py:107-112
        if embedding_dim % num_heads:
            unsupported.append(f"embedding_dim {embedding_dim} not divisible by num_heads {num_heads}")
        elif embedding_dim > 1024:  # (row kernels: 16 features per lane; the MLP's K = 4E <= 4096 of osrl_linear)
            unsupported.append(f"embedding_dim {embedding_dim} > 1024")
        elif embedding_dim // num_heads > 128:  # the tiled attention kernels' widest head
            unsupported.append(f"head_dim {embedding_dim // num_heads} > 128")
        if S > 1024:
            unsupported.append(f"{S} tokens per sequence > 1024 (seq_repeat * seq_len + cost_prefix)")
        if unsupported:
            raise NotImplementedError("osrl_amd CDT does not support: " + "; ".join(unsupported))
        self.seq_len, self.embedding_dim = seq_len, embedding_dim
        self.state_dim, self.action_dim = state_dim, action_dim
        self.episode_len, self.max_action = episode_len, max_action
        self.num_layers, self.num_heads = num_layers, num_heads
        self.cost_transform_on = bool(cost_transform)
        self.cost_transform = (lambda x: 50 - x) if cost_transform else None
        # cdt.py:243-250: every cost-feature op also requires use_cost
        self.add_cost_feat = bool(add_cost_feat and use_cost)
        self.mul_cost_feat = bool(mul_cost_feat and use_cost)
        self.cat_cost_feat = bool(cat_cost_feat and use_cost)
        self.stochastic = stochastic
        self.attention_dropout, self.residual_dropout = float(attention_dropout), float(residual_dropout)
        self.embedding_dropout = float(embedding_dropout)
        self.time_emb, self.use_rew, self.use_cost = bool(time_emb), bool(use_rew), bool(use_cost)
        self.cost_prefix = bool(cost_prefix)
        self.seq_repeat = seq_repeat
        self.action_head_layers = int(action_head_layers)
        self.device = str(device)
        dev = require_cuda(device)

        # container modules, created in the reference's order (cdt.py:87-141)
        self.emb_drop = nn.Dropout(embedding_dropout)
        self.emb_norm = nn.LayerNorm(embedding_dim)
        self.out_norm = nn.LayerNorm(embedding_dim)
        if self.time_emb:
            self.timestep_emb = nn.Embedding(episode_len + seq_len, embedding_dim)
        self.state_emb = nn.Linear(state_dim, embedding_dim)
        self.action_emb = nn.Linear(action_dim, embedding_dim)
        if self.use_cost:
            self.cost_emb = nn.Linear(1, embedding_dim)
        if self.use_rew:
            self.return_emb = nn.Linear(1, embedding_dim)
        if self.cost_prefix:
            self.prefix_emb = nn.Linear(1, embedding_dim)
        self.blocks = nn.ModuleList([TransformerBlock(S, embedding_dim, num_heads, attention_dropout,
                                                      residual_dropout) for _ in range(num_layers)])
        # cdt.py:125 tests the RAW constructor flag: the head is 2E wide whenever cat_cost_feat was asked for
        Eh = self.head_in_dim = 2 * embedding_dim if cat_cost_feat else embedding_dim
        if cat_cost_feat and not use_cost:
            raise NotImplementedError("cat_cost_feat without use_cost builds a 2E-wide head the reference's forward "
                                      "feeds E-wide features (cdt.py:125,247-250): it cannot run there either")
        if stochastic:  # cdt.py:127-133
            if action_head_layers >= 2:
                self.action_head = nn.Sequential(nn.Linear(Eh, Eh), nn.GELU(), DiagGaussianActor(Eh, action_dim))
                self.head_hidden_keys, self.head_out_key = ["cdt.action_head.0.weight"], "cdt.action_head.2.head.weight"
            else:
                self.action_head = DiagGaussianActor(Eh, action_dim)
                self.head_hidden_keys, self.head_out_key = [], "cdt.action_head.head.weight"
        else:  # cdt.py:134-137
            self.action_head = mlp([Eh] * action_head_layers + [action_dim], activation=nn.GELU,
                                   output_activation=nn.Identity)
            self.head_hidden_keys = [f"cdt.action_head.{2 * i}.weight" for i in range(action_head_layers - 1)]
            self.head_out_key = f"cdt.action_head.{2 * (action_head_layers - 1)}.weight"
        self.state_pred_head = nn.Linear(embedding_dim, state_dim)
        self.cost_pred_head = nn.Linear(embedding_dim, 2)
        self.apply(self._init_weights)

        g = FlatGroup("cdt", dev)
        plan_group(g, "cdt", self)
        g.finalize()
        bind_group(g, "cdt", self)
        self.groups: Dict[str, FlatGroup] = {"cdt": g}
        if stochastic:  # cdt.py:143-146: a plain tensor outside the state_dict
            self.log_temperature = torch.full((1,), float(np.log(init_temperature)), dtype=torch.float32, device=dev)
            self.target_entropy = target_entropy
        self._engine = None
        self._fast = None
        # forward() under grad mode records an autograd graph through the HIP kernels (ops.cdt_apply); off: inference only
        self.differentiable = bool(differentiable)

    def fast_policy(self, num_envs: Optional[int] = None):
        """The act latency path for the episode loop on a host environment (engine/cdt_act.py ``CDTFastPolicy``), built
        once per model.  With ``num_envs`` an integer: the lockstep form for that many host environments
        (``CDTVecFastPolicy``), built once per model and ``num_envs``.  Raises NotImplementedError naming the limit
        outside the path's domain."""
        if num_envs is not None:
            from ..engine.act import cached_vec_policy
            from ..engine.cdt_act import CDTVecFastPolicy
            return cached_vec_policy(self, num_envs, lambda n: CDTVecFastPolicy(self, n), CDTVecFastPolicy.LIMIT)
        if getattr(self, "_fast", None) is None:
            from ..engine.cdt_act import CDTFastPolicy
            self._fast = CDTFastPolicy(self)
        return self._fast

    def fast_eligible(self) -> bool:
        """The fast path computes the eval-mode forward: a model left in train() mode with dropout draws masks."""
        from ..engine.cdt_act import unsupported
        no_drop = max(self.attention_dropout, self.residual_dropout, self.embedding_dropout) == 0
        return (not self.training or no_drop) and unsupported(self) is None

    @staticmethod
    def _init_weights(module: nn.Module):
        """cdt.py:156-164."""
        if isinstance(module, (nn.Linear, nn.Embedding)):
            torch.nn.init.normal_(module.weight, mean=0.0, std=0.02)
            if isinstance(module, nn.Linear) and module.bias is not None:
                torch.nn.init.zeros_(module.bias)
        elif isinstance(module, nn.LayerNorm):
            torch.nn.init.zeros_(module.bias)
            torch.nn.init.ones_(module.weight)

    def temperature(self):
        return self.log_temperature.exp() if self.stochastic else None

    def engine(self, batch_size: int, cfg: Optional[dict] = None, dist=None):
        from ..common.checkpoint import engine_handoff
        from ..engine.cdt import CDTEngine
        if self._engine is None or self._engine.B != batch_size or dist is not None or \
                (cfg is not None and cfg != self._engine.cfg):
            if cfg is None:
                raise RuntimeError("build a CDTTrainer before training")
            old, self._engine = self._engine, CDTEngine(self, batch_size, cfg, dist=dist)
            engine_handoff(self, self._engine, old)
        return self._engine

    def _default_cfg(self) -> dict:
        return self._engine.cfg if self._engine is not None else dict(
            learning_rate=1e-4, weight_decay=1e-4, betas=(0.9, 0.999), clip_grad=0.25, lr_warmup_steps=1,
            loss_cost_weight=0.0, loss_state_weight=0.0, no_entropy=False)

    def load_window(self, e, states, actions, returns_to_go, costs_to_go, time_steps, padding_mask=None,
                    episode_cost=None) -> int:
        """Copy one forward's inputs into engine ``e``; returns the window length Tin.  Shorter windows (early rollout
        steps, cdt.py:485-489) are left-aligned and zero-padded to seq_len: with the causal mask the first Tin positions
        are exactly the short-sequence result."""
        B, Tin, T = states.shape[0], states.shape[1], self.seq_len
        if Tin > T:
            raise ValueError(f"window of {Tin} steps > seq_len {T}")
        mask = torch.ones(B, Tin, device=states.device) if padding_mask is None else \
            (~padding_mask.to(torch.bool)).float()
        if Tin < T:
            def pad(x, val=0):
                out = torch.full((B, T) + tuple(x.shape[2:]), val, dtype=x.dtype, device=x.device)
                out[:, :Tin] = x
                return out
            states, actions, returns_to_go, costs_to_go = pad(states), pad(actions), pad(returns_to_go), pad(costs_to_go)
            time_steps, mask = pad(time_steps), pad(mask)
        if self.cost_prefix and episode_cost is None:
            raise ValueError("cost_prefix=True: pass episode_cost [B] (cdt.py:207-213)")
        e.load_batch(states, actions, returns_to_go, costs_to_go, time_steps, mask, torch.zeros_like(mask),
                     torch.as_tensor(episode_cost, dtype=torch.float32, device=states.device).reshape(B)
                     if self.cost_prefix else None)
        return Tin

    def forward(self, states, actions, returns_to_go, costs_to_go, time_steps, padding_mask=None,
                episode_cost=None):
        """cdt.py:166-265: returns (action_preds, cost_preds, state_preds) where action_preds is
        ``torch.distributions.Normal(mu, std)`` for a stochastic head.  With ``differentiable`` set and grad mode on, the
        outputs are attached to the autograd graph (ops.cdt_apply: forward and backward on the HIP kernels); otherwise
        this is the inference forward and nothing is recorded."""
        if self.differentiable and torch.is_grad_enabled():
            return self._forward_grad(states, actions, returns_to_go, costs_to_go, time_steps, padding_mask,
                                      episode_cost)
        return self._forward_infer(states, actions, returns_to_go, costs_to_go, time_steps, padding_mask, episode_cost)

    def grad_engine(self, batch_size: int):
        """The engine of the differentiable forward for this batch size and the current mode (train() with dropout > 0
        draws masks, every other case runs without): one per mode, rebuilt when the batch size changes.  Separate from
        the trainer's ``_engine`` (own gradient slabs; no optimizer state is touched)."""
        from ..engine.cdt import CDTEngine
        drop = self.training and max(self.attention_dropout, self.residual_dropout, self.embedding_dropout) > 0
        cache = self.__dict__.setdefault("_grad_engines", {})
        e = cache.get(drop)
        if e is None or e.B != batch_size:
            cache[drop] = None  # (the old engine's buffers go before the new ones are allocated)
            e = cache[drop] = CDTEngine(self, batch_size, self._default_cfg(), grad=True, dropout=drop)
        return e

    def _forward_grad(self, states, actions, returns_to_go, costs_to_go, time_steps, padding_mask, episode_cost):
        from ..ops import cdt_apply
        e = self.grad_engine(states.shape[0])
        head, logits, sp = cdt_apply(self, e, states, actions, returns_to_go, costs_to_go, time_steps, padding_mask,
                                     episode_cost)
        if self.stochastic:
            ad = self.action_dim
            ap = torch.distributions.Normal(head[..., :ad], head[..., ad:].exp())
        else:
            ap = head
        return ap, torch.log_softmax(logits, -1), sp

    @torch.no_grad()
    def _forward_infer(self, states, actions, returns_to_go, costs_to_go, time_steps, padding_mask=None,
                       episode_cost=None):
        B, T = states.shape[0], self.seq_len
        from ..engine.cdt import CDTEngine
        if getattr(self, "_infer", None) is None or self._infer.B != B:
            self._infer = CDTEngine(self, B, self._default_cfg(), inference=True)
        e = self._infer
        Tin = self.load_window(e, states, actions, returns_to_go, costs_to_go, time_steps, padding_mask, episode_cost)
        self.repack()
        if self.training and max(self.attention_dropout, self.residual_dropout, self.embedding_dropout) > 0:
            e.st.tick()  # a model left in train() mode draws a fresh dropout mask per call, like nn.Dropout
        e.forward(train=self.training)
        ad, od = self.action_dim, self.state_dim
        if self.stochastic:
            mu = e.head[:, :ad].reshape(B, T, ad)[:, :Tin].clone()
            ls = e.head[:, ad:].reshape(B, T, ad)[:, :Tin].clone()
            ap = torch.distributions.Normal(mu, ls.exp())
        else:
            ap = e.head.reshape(B, T, ad)[:, :Tin].clone()
        return (ap, torch.log_softmax(e.logits.reshape(B, T, 2)[:, :Tin], -1),
                e.sp.reshape(B, T, od)[:, :Tin].clone())


class CDTTrainer:
    """cdt.py:268-418."""

    def __init__(self, model: CDT, env=None, logger=None, learning_rate: float = 1e-4,
                 weight_decay: float = 1e-4, betas: Tuple[float, ...] = (0.9, 0.999), clip_grad: float = 0.25,
                 lr_warmup_steps: int = 10000, reward_scale: float = 1.0, cost_scale: float = 1.0,
                 loss_cost_weight: float = 0.0, loss_state_weight: float = 0.0, cost_reverse: bool = False,
                 no_entropy: bool = False, device="cuda", stats_mode: str = "lazy", use_graph: bool = True,
                 seed: int = 0, fast_rollout: bool = True, matmul: str = "f32") -> None:
        """``matmul``: "f32" (default) runs the projection GEMMs of the train step and their input gradients on the
        f32-MFMA kernels; "bf16x3" runs them as exact bf16 triples on the bf16 matrix cores (osrl_linear_split) wherever
        that kernel takes the layer's shape -- same model, checkpoints and parity bound, fp32-class but not bit-equal to
        "f32".  Weight gradients, attention, LayerNorm, GELU, the loss and AdamW are the same in both; the inference
        forward, ``differentiable=True`` and the act path (``fast_policy``) always run "f32"."""
        from ..engine.plan import check_matmul
        check_matmul(matmul)  # (before any device work)
        self.model, self.logger, self.env = model, logger, env
        self.clip_grad, self.reward_scale, self.cost_scale, self.device = clip_grad, reward_scale, cost_scale, device
        self.cost_weight, self.state_weight = loss_cost_weight, loss_state_weight
        self.cost_reverse, self.no_entropy = cost_reverse, no_entropy
        self.stochastic = model.stochastic
        self.max_action = model.max_action
        self.stats_mode, self.use_graph = stats_mode, use_graph
        self.fast_rollout = bool(fast_rollout)  # rollout() on host envs through CDT.fast_policy() when eligible
        self.cfg = dict(learning_rate=learning_rate, weight_decay=weight_decay, betas=tuple(betas),
                        clip_grad=clip_grad, lr_warmup_steps=lr_warmup_steps, loss_cost_weight=loss_cost_weight,
                        loss_state_weight=loss_state_weight, no_entropy=no_entropy, seed=int(seed), matmul=matmul)

    def train_one_step(self, states, actions, returns, costs_return, time_steps, mask, episode_cost, costs):
        """cdt.py:343-418 (``episode_cost`` only feeds the cost-prefix variant)."""
        eng = self.model.engine(states.shape[0], self.cfg)
        if self.model.__dict__.get("_grad_engines"):  # a user optimizer may have edited the parameters in place since
            self.model.repack()                        # the last differentiable forward: refresh the packed copies
        eng.step(states, actions, returns, costs_return, time_steps, mask, costs, use_graph=self.use_graph,
                 episode_cost=episode_cost if self.model.cost_prefix else None)
        keys = None if self.stochastic else ["all_loss", "act_loss", "cost_loss", "cost_acc", "state_loss", "train_lr"]
        store_stats(self.logger, eng.st, self.stats_mode, tab="train", keys=keys)

    def evaluate(self, num_rollouts, target_return, target_cost, schedule: str = "waves"):
        """cdt.py:420-434.  With a ``VecSyntheticSafeEnv`` as ``self.env`` the ``num_rollouts`` episodes run as one
        batch on device (engine/rollout.py ``CDTBatchedRollout``).  With a list or tuple of N host environments rollout
        ``j`` runs on environment ``j % N``, N rollouts at a time in lockstep (``rollout_many``), or with
        ``schedule="refill"`` as one job queue (``evaluate_targets``)."""
        from ..common.synthetic_env import DeviceVecEnv
        from ..engine.act import check_schedule
        check_schedule(schedule)
        if isinstance(self.env, (list, tuple)):
            return self.evaluate_targets(num_rollouts, [(target_return, target_cost)], schedule=schedule)[0]
        if isinstance(self.env, DeviceVecEnv):
            if self.env.E != num_rollouts:
                raise ValueError(f"the vector environment holds {self.env.E} episodes, evaluate() was asked for "
                                 f"{num_rollouts}")
            r, c, n = self._batched_rollout().run(target_return, target_cost)
            return float(r.mean()) / self.reward_scale, float(c.mean()) / self.cost_scale, float(n.mean())
        self.model.eval()
        rets, costs, lens = [], [], []
        for _ in range(num_rollouts):
            r, l, c = self.rollout(self.model, self.env, target_return, target_cost)
            rets.append(r)
            lens.append(l)
            costs.append(c)
        self.model.train()
        return np.mean(rets) / self.reward_scale, np.mean(costs) / self.cost_scale, np.mean(lens)

    def _batched_rollout(self):
        """The ``CDTBatchedRollout`` on ``self.env`` (buffers + captured graph), cached on the trainer."""
        from ..engine.rollout import CDTBatchedRollout, cached
        return cached(self, "_rollout", id(self.env), lambda: CDTBatchedRollout(self.model, self.env, self.cost_scale,
                                                                                 self.cost_reverse, self.use_graph))

    def collect_targets(self, target_return, target_cost, noise_std=0.0, sample: bool = False,
                        gamma: Optional[float] = None, seed: int = 0, noise=None, into=None):
        """The ``evaluate`` rollout on a ``VecSyntheticSafeEnv``, recorded (the other trainers' ``collect``; here the
        method carries the targets a CDT rollout cannot do without, and sits beside ``evaluate_targets``).  Every episode
        of ``self.env`` runs to its end by the windowed autoregression, conditioned on ``(target_return, target_cost)`` --
        one pair for all episodes or one value per episode -- and comes back as a ``Collected`` (engine/collect.py): the
        DSRL-layout dataset on device plus the per-episode (discounted) sums.
        The action is ``clip(mu + s * eps)``: ``s = noise_std`` (one sigma or one per episode), or with ``sample=True``
        the Gaussian head's own ``exp(log_std)`` (ValueError on a ``stochastic=False`` model, and together with a non-zero
        ``noise_std``); the window records the action taken.  ``gamma``, ``seed``, ``noise`` as ``collect`` takes them.
        ``into``: a ``SequenceStore`` built with capacities (``store.append``: an attached CDT engine draws from the new
        trajectories at its next ``step_store``) or a capacity ``ReplayStore``; the result's ``dataset`` is then None, and
        a store that cannot take the run is a ValueError before the run.  Any other kind of environment: TypeError."""
        from ..common.synthetic_env import VecSyntheticSafeEnv
        from ..engine.collect import check_sampling, collect_cdt_batched
        check_sampling(self.model, sample, noise_std)
        if not isinstance(self.env, VecSyntheticSafeEnv):
            raise TypeError(f"collect_targets() records the batched on-device rollout: self.env must be a "
                            f"VecSyntheticSafeEnv, not {type(self.env).__name__}")
        return collect_cdt_batched(self, target_return=target_return, target_cost=target_cost, noise_std=noise_std,
                                   sample=sample, gamma=gamma, seed=seed, noise=noise, into=into)

    def planner(self, *args, **kwargs):
        """The MLP trainers' ``planner`` (engine/mpc.py) is not built for CDT: every candidate would need a window of its
        own.  Always a TypeError."""
        raise TypeError("CDTTrainer has no planner: policy-guided shooting needs one transformer window per candidate, "
                        "which is out of scope; the five MLP trainers have planner() / evaluate_planned()")

    @torch.no_grad()
    def rollout(self, model: CDT, env, target_return: float, target_cost: float):
        """cdt.py:436-518: autoregressive rollout on a sliding window of the last seq_len steps.  With
        ``fast_rollout`` and an eligible model (eval mode or no dropout, inside the act path's domain) the window lives
        on the device and each env step is one C call (``CDT.fast_policy()``); otherwise the loop below."""
        if self.fast_rollout and model.fast_eligible():
            return self._rollout_fast(model, env, target_return, target_cost)
        dev = torch.device(model.device)
        EL, T = model.episode_len, model.seq_len
        states = torch.zeros(1, EL + 1, model.state_dim, device=dev)
        actions = torch.zeros(1, EL, model.action_dim, device=dev)
        returns = torch.zeros(1, EL + 1, device=dev)
        costs = torch.zeros(1, EL + 1, device=dev)
        time_steps = torch.arange(EL, dtype=torch.long, device=dev).view(1, -1)
        obs, info = env.reset()
        states[:, 0] = torch.as_tensor(obs, device=dev)
        returns[:, 0] = float(target_return)
        costs[:, 0] = float(target_cost)
        epi_cost = torch.tensor([target_cost], dtype=torch.float, device=dev)
        ep_ret, ep_cost, ep_len = 0.0, 0.0, 0
        for step in range(EL):
            lo = max(0, step + 1 - T)
            acts, _, _ = model(states[:, lo:step + 1], actions[:, lo:step + 1], returns[:, lo:step + 1],
                               costs[:, lo:step + 1], time_steps[:, lo:step + 1], None, epi_cost)
            if self.stochastic:
                acts = acts.mean
            act = acts.clamp(-self.max_action, self.max_action)[0, -1].cpu().numpy()
            obs_next, reward, terminated, truncated, info = env.step(act)
            cost = ((1.0 - info["cost"]) if self.cost_reverse else info["cost"]) * self.cost_scale
            actions[:, step] = torch.as_tensor(act, device=dev)
            states[:, step + 1] = torch.as_tensor(obs_next, device=dev)
            returns[:, step + 1] = returns[:, step] - float(reward)
            costs[:, step + 1] = costs[:, step] - float(cost)
            ep_ret += reward
            ep_len += 1
            ep_cost += info["cost"]
            if terminated or truncated:
                break
        return ep_ret, ep_len, ep_cost

    def evaluate_targets(self, num_rollouts, targets, schedule: str = "waves"):
        """``evaluate`` for each ``(target_return, target_cost)`` pair of ``targets``: a list of ``(return, cost,
        length)`` triples.  With a list or tuple of N host environments as ``self.env`` the ``len(targets) *
        num_rollouts`` rollouts are laid out target-major and job ``q`` runs in wave ``q // N`` on environment
        ``q % N``, so rollouts for different targets share a wave.  With a ``VecSyntheticSafeEnv`` of
        ``len(targets) * num_rollouts`` episodes (and more than one pair) the whole grid is ONE batched rollout, target-major:
        episode ``j`` carries ``targets[j // num_rollouts]`` and starts at the environment's initial state ``base_seed +
        j``, each triple is the mean over its own ``num_rollouts`` episodes; with ``num_rollouts`` episodes it is one
        ``evaluate`` per pair, any other size is a ValueError.  With any other environment this is one ``evaluate`` per
        pair.  ``schedule="refill"`` (list of environments): the same jobs as one queue, where a slot
        whose episode has ended takes the next job at once (``rollout_jobs``; the run is kept as ``last_refill``)."""
        from ..common.synthetic_env import DeviceVecEnv
        from ..engine.act import check_schedule
        check_schedule(schedule)
        targets = [(float(tr), float(tc)) for tr, tc in targets]
        if isinstance(self.env, DeviceVecEnv):
            k, G = int(num_rollouts), len(targets)
            if G > 1 and self.env.E == G * k:  # the whole grid as one batched rollout, target-major
                ro = self._batched_rollout()
                r, c, n = ro.run(np.repeat([t[0] for t in targets], k), np.repeat([t[1] for t in targets], k))
                return [(float(r[i * k:(i + 1) * k].mean()) / self.reward_scale,
                         float(c[i * k:(i + 1) * k].mean()) / self.cost_scale, float(n[i * k:(i + 1) * k].mean()))
                        for i in range(G)]
            if self.env.E != k:
                raise ValueError(f"the vector environment holds {self.env.E} episodes: evaluate_targets() takes "
                                 f"num_rollouts ({k}, one rollout per target pair) or len(targets) * num_rollouts "
                                 f"({G * k}, the whole grid as one rollout)")
        if not isinstance(self.env, (list, tuple)):
            return [self.evaluate(num_rollouts, tr, tc) for tr, tc in targets]
        envs = list(self.env)
        N = len(envs)
        if N == 0:
            raise ValueError("evaluate over an empty list of environments")
        jobs = [t for t in targets for _ in range(int(num_rollouts))]
        self.model.eval()
        rets, lens, costs = [], [], []
        if schedule == "refill":
            res = self.last_refill = self.rollout_jobs(self.model, envs, [t[0] for t in jobs], [t[1] for t in jobs])
            rets, lens, costs = list(res.returns), list(res.lengths), list(res.costs)
        else:
            for q0 in range(0, len(jobs), N):
                wave = jobs[q0:q0 + N]
                r, l, c = self.rollout_many(self.model, envs[:len(wave)], [t[0] for t in wave], [t[1] for t in wave],
                                            num_slots=N)
                rets += list(r)
                lens += list(l)
                costs += list(c)
        self.model.train()
        out, k = [], int(num_rollouts)
        for i in range(len(targets)):
            sl = slice(i * k, (i + 1) * k)
            out.append((np.mean(rets[sl]) / self.reward_scale, np.mean(costs[sl]) / self.cost_scale,
                        np.mean(lens[sl])))
        return out

    @torch.no_grad()
    def rollout_many(self, model: CDT, envs, target_returns, target_costs, num_slots: Optional[int] = None):
        """``rollout`` on each of the host environments ``envs`` at once: three arrays (return, length, raw cost sum),
        one entry per environment, equal to what ``rollout`` returns for each environment alone.  The targets are
        scalars or one per environment.  With ``fast_rollout`` and an eligible model the episodes run in lockstep
        through ``CDT.fast_policy(num_envs)``, one C call per env step for all of them, and a slot leaves the loop when
        its environment terminates, truncates or reaches ``episode_len``; otherwise one ``rollout`` per environment.
        ``num_slots`` (default ``len(envs)``): the width of the policy to use, the slots past ``len(envs)`` idle."""
        envs = list(envs)
        n = len(envs)
        trs = np.broadcast_to(np.asarray(target_returns, dtype=np.float64), (n,))
        tcs = np.broadcast_to(np.asarray(target_costs, dtype=np.float64), (n,))
        N = n if num_slots is None else int(num_slots)
        if N < n:
            raise ValueError(f"{n} environments do not fit {N} slots")
        ep_ret, ep_len, ep_cost = [0.0] * n, np.zeros(n, np.int64), [0.0] * n
        if n == 0:
            return np.asarray(ep_ret), ep_len, np.asarray(ep_cost)
        if not (self.fast_rollout and model.fast_eligible()):
            for e, env in enumerate(envs):
                ep_ret[e], ep_len[e], ep_cost[e] = self.rollout(model, env, float(trs[e]), float(tcs[e]))
            return np.asarray(ep_ret), ep_len, np.asarray(ep_cost)
        pol = model.fast_policy(num_envs=N)
        obs = np.zeros((N, model.state_dim), np.float32)
        reward, cost = np.zeros(N, np.float64), np.zeros(N, np.float64)
        tr_n, tc_n = np.zeros(N, np.float64), np.zeros(N, np.float64)
        tr_n[:n], tc_n[:n] = trs, tcs
        active = np.zeros(N, bool)
        active[:n] = True
        for e, env in enumerate(envs):
            obs[e], _ = env.reset()
        act = pol.reset(obs, tr_n, tc_n)
        EL = model.episode_len
        for step in range(EL):
            for e in np.flatnonzero(active):
                obs_next, r, terminated, truncated, info = envs[e].step(act[e])
                ep_ret[e] += r
                ep_len[e] += 1
                ep_cost[e] += info["cost"]
                if terminated or truncated or step + 1 == EL:
                    active[e] = False
                    continue
                obs[e], reward[e] = obs_next, r
                cost[e] = ((1.0 - info["cost"]) if self.cost_reverse else info["cost"]) * self.cost_scale
            if not active.any():
                break
            act = pol.step(obs, reward, cost, active=active)
        return np.asarray(ep_ret), ep_len, np.asarray(ep_cost)

    @torch.no_grad()
    def rollout_jobs(self, model: CDT, envs, target_returns, target_costs):
        """One rollout per ``(target_returns[q], target_costs[q])`` over the host environments ``envs`` on the refill
        schedule (engine/act.py ``rollout_refill``): job ``q`` starts in slot ``q`` while slots are free, and a slot
        whose episode has ended takes the next job in the policy call in which the others step
        (``CDTVecFastPolicy.step(restart=...)``).  Returns a ``RefillResult``: per job (return, length, raw cost sum),
        each equal to ``rollout`` alone on the job's environment in that environment's job order, the slot (environment)
        each job ran in, and the number of policy calls.  Without ``fast_rollout`` or an eligible model job ``q`` runs
        through ``rollout`` on environment ``q % len(envs)`` (no policy calls are counted)."""
        from ..engine.act import RefillResult, rollout_refill
        envs = list(envs)
        trs, tcs = np.asarray(target_returns, dtype=np.float64), np.asarray(target_costs, dtype=np.float64)
        if trs.ndim != 1 or trs.shape != tcs.shape:
            raise ValueError(f"expected target_returns and target_costs as two lists of one length, got shapes "
                             f"{trs.shape} and {tcs.shape}")
        J, N = len(trs), len(envs)
        if J and N == 0:
            raise ValueError("jobs over an empty list of environments")
        if J and not (self.fast_rollout and model.fast_eligible()):
            out = [self.rollout(model, envs[q % N], float(trs[q]), float(tcs[q])) for q in range(J)]
            return RefillResult(np.asarray([o[0] for o in out]), np.asarray([o[1] for o in out], np.int64),
                                np.asarray([o[2] for o in out]), np.arange(J) % N, 0)
        adapter = _CDTRefillAdapter(self, model, N) if J else None
        return rollout_refill(adapter, envs, list(zip(trs.tolist(), tcs.tolist())), model.episode_len)

    @torch.no_grad()
    def collect_jobs(self, model: CDT, envs, target_returns, target_costs, noise_std=0.0, sample: bool = False,
                     gamma: Optional[float] = None, seed: int = 0, noise=None, episode_ids=None, into=None):
        """``rollout_jobs`` recorded, with exploration noise (the other trainers' ``collect_jobs``; ``collect_targets``
        for host environments): one episode per ``(target_returns[q], target_costs[q])`` on the refill schedule, every
        action ``clip(mu + s * eps)`` computed by the act path's head launch -- ``s = noise_std`` (one sigma or one per
        job) or, with ``sample=True``, the Gaussian head's own ``exp(log_std)`` (``check_sampling``'s rules) -- and the
        window records the action taken.  Job ``q``'s noise is keyed by ``(seed, episode_ids[q], the episode's step,
        column)``, ``collect_targets``' key, or injected as ``noise [jobs, episode_len, action_dim]``.  Returns a
        ``Collected``: rows job-major with each job's true length, the dataset on device, the cost sums times
        ``cost_scale``.  With ``sample=True`` the head rows ``(mu | log_std)`` of every step, job-major like the dataset,
        are kept as ``self.last_head_rows`` (numpy ``[rows, 2 * action_dim]``) for behaviour log-probabilities.
        ``into``: a ``SequenceStore`` with capacities (refused before the run unless every job could run to
        ``episode_len``) or a capacity ``ReplayStore``.  A model outside the act path's domain: NotImplementedError."""
        from ..engine.act import check_job_noise, check_jobs_store, collect_refill, finish_jobs
        from ..engine.cdt_act import unsupported
        from ..engine.collect import check_sampling
        check_sampling(model, sample, noise_std)
        envs = list(envs)
        trs, tcs = np.asarray(target_returns, dtype=np.float64), np.asarray(target_costs, dtype=np.float64)
        if trs.ndim != 1 or trs.shape != tcs.shape:
            raise ValueError(f"expected target_returns and target_costs as two lists of one length, got shapes "
                             f"{trs.shape} and {tcs.shape}")
        J, N = len(trs), len(envs)
        sg, noise, ids = check_job_noise(J, model.episode_len, model.action_dim, noise_std, noise, episode_ids)
        check_jobs_store(into, J, model.episode_len, model.state_dim, model.action_dim)
        why = unsupported(model)
        if why is not None:
            raise NotImplementedError("the CDT act latency path does not support: " + why)
        if not model.fast_eligible():
            raise NotImplementedError("collect_jobs runs the eval-mode forward of the act path: call model.eval() on a "
                                      "model with dropout")
        if J and N == 0:
            raise ValueError("jobs over an empty list of environments")
        adapter = _CDTCollectAdapter(self, model, N, bool(sample), int(seed), noise) if J else None
        jobs = [(q, float(trs[q]), float(tcs[q]), int(ids[q]), float(sg[q])) for q in range(J)]
        got = collect_refill(adapter, envs, jobs, model.episode_len, gamma, self.cost_scale)
        if J == 0:
            got.dataset["observations"] = got.dataset["next_observations"] = np.zeros((0, model.state_dim), np.float32)
            got.dataset["actions"] = np.zeros((0, model.action_dim), np.float32)
        self.last_head_rows = adapter.head_rows() if sample and J else None
        return finish_jobs(got, model.device, into)

    def _rollout_fast(self, model: CDT, env, target_return: float, target_cost: float):
        pol = model.fast_policy()
        obs, info = env.reset()
        act = pol.reset(obs, target_return, target_cost)
        ep_ret, ep_cost, ep_len = 0.0, 0.0, 0
        EL = model.episode_len
        for step in range(EL):
            obs_next, reward, terminated, truncated, info = env.step(act)
            cost = ((1.0 - info["cost"]) if self.cost_reverse else info["cost"]) * self.cost_scale
            ep_ret += reward
            ep_len += 1
            ep_cost += info["cost"]
            if terminated or truncated or step + 1 == EL:
                break
            act = pol.step(obs_next, reward, cost)
        return ep_ret, ep_len, ep_cost


class _CDTRefillAdapter:
    """engine/act.py ``rollout_refill`` over ``CDT.fast_policy(num_envs)``: a job is a ``(target_return, target_cost)``
    pair."""

    def __init__(self, trainer: CDTTrainer, model: CDT, num_envs: int):
        self.pol = model.fast_policy(num_envs=num_envs)
        self.obs_dim, self.N = model.state_dim, num_envs
        self.reverse, self.scale = trainer.cost_reverse, trainer.cost_scale

    def observe(self, o):
        return o

    def costs(self, info):
        return ((1.0 - info["cost"]) if self.reverse else info["cost"]) * self.scale, info["cost"]

    def act(self, obs, reward, cost, step, restart, jobs):
        tr, tc = np.zeros(self.N, np.float64), np.zeros(self.N, np.float64)
        for e, j in enumerate(jobs):
            if j is not None:
                tr[e], tc[e] = j
        return self.pol.step(obs, reward, cost, active=step, restart=restart, target_return=tr, target_cost=tc)


class _CDTCollectAdapter(_CDTRefillAdapter):
    """``_CDTRefillAdapter`` with the exploration tail: a job is ``(q, target_return, target_cost, episode id, sigma)``;
    ``noise`` (None, or ``[J, episode_len, action_dim]``) is injected instead of the keyed draw."""

    def __init__(self, trainer: CDTTrainer, model: CDT, num_envs: int, sample: bool, seed: int, noise):
        super().__init__(trainer, model, num_envs)
        N, ad = num_envs, model.action_dim
        self.sample, self.seed, self.noise = sample, seed, noise
        self.tr, self.tc = np.zeros(N, np.float64), np.zeros(N, np.float64)
        self.ids, self.sigma = np.zeros(N, np.int64), np.zeros(N, np.float32)
        self.job, self.t = np.zeros(N, np.int64), np.zeros(N, np.int64)
        self.eps = None if noise is None else np.zeros((N, ad), np.float32)
        self.heads = {}  # job -> list of head rows, in step order

    def act(self, obs, reward, cost, step, restart, jobs):
        for e, j in enumerate(jobs):
            if j is not None:
                self.job[e], self.tr[e], self.tc[e], self.ids[e], self.sigma[e] = j
                self.t[e] = -1
        run = step | restart
        self.t[run] += 1
        if self.eps is not None:
            self.eps[run] = self.noise[self.job[run], self.t[run]]
        act = self.pol.step(obs, reward, cost, active=step, restart=restart, target_return=self.tr, target_cost=self.tc,
                            explore_std=self.sigma, sample=self.sample, explore_seed=self.seed, explore_noise=self.eps,
                            episode_ids=self.ids)
        if self.sample:
            head = self.pol.last_head
            for e in np.flatnonzero(run):
                self.heads.setdefault(int(self.job[e]), []).append(head[e])
        return act

    def head_rows(self) -> np.ndarray:
        return np.stack([h for q in sorted(self.heads) for h in self.heads[q]])
