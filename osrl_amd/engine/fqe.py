"""Fitted Q evaluation (FQE) of a frozen policy as a static launch plan on MI355X.

There is no reference file to follow: the reference evaluates a policy by rolling it out.  FQE fits, on the logged
transitions alone, a reward critic and a cost critic for the policy pi with the backup

    x + gamma (1 - done) Q_targ(s', pi(s')),        x = reward | cost

and reads ``Q(s0, pi(s0))`` at the dataset's initial states (``ValueReadout``).  The pieces are the ones the Q-learning
engines use: ensembles sharing an input tile, the backward launch that computes its own dY (``OSRL_SEED_FQE``,
include/osrl_amd.h), the fused Adam + Polyak step, the minibatch draw inside the captured step.

One chain on one stream:  prologue -> pi(s') (the launches of ``BatchedRollout.body`` for the policy's kind) -> the
2 num_q target nets on [s', pi(s')] -> the 2 num_q online nets on [s, a] -> the seeded backward -> dW + Adam + Polyak.
The policy's packed weights are read in place and never written.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib as L
from ..common.net import actor_head_desc, net_desc_seq, vae_dec_desc
from . import glue as G
from ._step import StepEngine
from .core import DwPlan, MlpRun, StepState, concat_nets, cur_stream, randn_fill

STAT_KEYS = ["loss/fqe_reward_loss", "loss/fqe_cost_loss"]
_Z_STREAM = 12  # Philox stream id of the BCQ-Lag decode noise drawn by ValueReadout (the step's own uses stream 0)


def policy_kind(policy) -> str:
    """The ``kind`` of engine/rollout.py the policy acts by; TypeError for a policy FQE cannot evaluate."""
    name = type(policy).__name__
    kinds = {"BC": "bc", "CPQ": "cpq", "BEARL": "cpq", "COptiDICE": "dice", "BCQL": "bcql"}
    if name == "CDT":
        raise TypeError("FQE needs a policy whose action is a function of the state alone; CDT's depends on a history")
    if name not in kinds:
        raise TypeError(f"FQE evaluates BC, CPQ, BEARL, COptiDICE and BCQL policies, not {name}")
    return kinds[name]


class PolicyForward:
    """pi(obs) on ``rows`` rows: the action ``model.act`` takes deterministically, by the launches of
    ``BatchedRollout.body`` for the policy's kind.  ``forward`` returns the [rows, action_dim] buffer it fills."""

    def __init__(self, policy, kind: str, rows: int, device, tile_rows: int = 0):
        m = self.policy = policy
        self.kind, self.rows, self.ad = kind, int(rows), int(m.action_dim)
        policy.repack()  # (the packed copies follow the parameters, as BatchedRollout makes sure of)
        run = lambda d: MlpRun(d, self.rows, False, device, tile_rows=tile_rows)  # noqa: E731
        if kind == "bc":
            self.r_pi = run(net_desc_seq([m.actor.pi], float(m.max_action)))
            self.a = self.r_pi.y[0]
        else:
            self.a = torch.zeros(self.rows, self.ad, dtype=torch.float32, device=device)
            if kind in ("cpq", "dice"):
                self.r_pi = run(actor_head_desc(m.actor))
            else:
                self.r_dec = run(vae_dec_desc(m.vae))
                self.r_pi = run(net_desc_seq([m.actor.pi], 1.0))

    def forward(self, obs: torch.Tensor, z: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``z`` (bcql): the decode noise [rows, latent_dim], already clamped (net.py:334-335)."""
        m, n, ad = self.policy, self.rows, self.ad
        if self.kind == "bc":
            self.r_pi.forward(obs)
        elif self.kind in ("cpq", "dice"):  # COptiDICE.act does not scale by max_action (coptidice.py:252)
            head = self.r_pi.forward(obs)[0]
            G.gauss_head(head, None, n, ad, float(m.max_action) if self.kind == "cpq" else 1.0, a=self.a)
        else:
            dec = self.r_dec.forward(obs, z)[0]
            t = self.r_pi.forward(obs, dec)[0]
            G.bcq_perturb(dec, t, n, ad, float(m.actor.phi), float(m.max_action), self.a)
        return self.a


def _critic_descs(model):
    seq = lambda mod: net_desc_seq(list(mod.q_nets), 1.0)  # noqa: E731
    return (concat_nets(seq(model.critic), seq(model.cost_critic)),
            concat_nets(seq(model.critic_old), seq(model.cost_critic_old)))


class FQEEngine(StepEngine):
    SIDE_STREAMS = 0

    def __init__(self, model, batch_size: int, seed: int = 0, dist=None):
        if dist is not None:
            raise ValueError("FQE has no data-parallel step (dist must be None)")
        m = self.model = model
        B = self.B = int(batch_size)
        self.dist, self.seed, self.rows_global = None, int(seed), 0
        dev = torch.device(m.device)
        od, ad, E = m.state_dim, m.action_dim, m.num_q
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)  # noqa: E731
        self.st = StepState(dev, STAT_KEYS)
        self.obs, self.nobs, self.act = z(B, od), z(B, od), z(B, ad)
        self.rew, self.cost, self.done = z(B), z(B), z(B)
        self.noise_flat = self.noise = None
        if m.kind == "bcql":  # the decode noise of pi(s'), one draw per row and step
            self.noise_flat, self.noise = self.noise_layout({"z": (B, m.policy.latent_dim)}, dev)
        self.pi = PolicyForward(m.policy, m.kind, B, dev)
        d_on, d_tg = _critic_descs(m)
        m.repack()
        self.r_t = MlpRun(d_tg, B, False, dev)
        self.r_q = MlpRun(d_on, B, True, dev)
        self.dq = z(2 * E, B, 1)
        self.r_q.setup_backward(self.dq)
        # reward and cost ensembles live in ONE group: one dW plan, one Adam + Polyak launch
        self.p_critic = DwPlan(m.groups["critic"], self.r_q.dw_entries(), B, dev)
        self.seed_fqe = G.seed_fqe(self.r_t.y, E, E, self.rew, self.cost, self.done, B, m.gamma,
                                   G.SeedStat(dev, 2 * E, B), self.st.stat_ptr(STAT_KEYS[0]),
                                   self.st.stat_ptr(STAT_KEYS[1]))
        self._plans_built()

    def attach_replay(self, store) -> None:
        if store is not None:
            self.model.check_store(store)
        super().attach_replay(store)

    def body(self, device_noise: bool) -> None:
        m, st = self.model, self.st
        batch = (self.obs, self.nobs, self.act, self.rew, self.cost, self.done)
        # (a store built with state_init carries a 7th table, is_init, that the step does not read)
        fields = range(len(batch)) if self.replay is not None and self.replay.n_fields != len(batch) else None
        st.prologue(self.replay, batch, self.noise_flat, self.seed, device_noise, fields)
        zn = None
        if self.noise is not None:
            zn = self.noise["z"]
            G.clamp_(zn, -0.5, 0.5)  # net.py:334-335
        a_next = self.pi.forward(self.nobs, zn)
        self.r_t.forward(self.nobs, a_next)
        self.r_q.forward(self.obs, self.act)
        self.r_q.backward_dz(seed=self.seed_fqe)
        self._optim("critic", self.p_critic, tau=m.tau)


class ValueReadout:
    """``Q(s0, pi(s0))`` of both online ensembles on chunks of ``rows`` initial states, accumulated per member in fp64
    (osrl_fqe_value_sums).  Row results do not depend on the chunk size: every launch runs on 16-row tiles, whose rows
    are computed independently of each other."""

    def __init__(self, model, rows: int, device):
        m = self.model = model
        self.rows = int(rows)
        self.s0 = torch.zeros(self.rows, m.state_dim, dtype=torch.float32, device=device)
        self.pi = PolicyForward(m.policy, m.kind, self.rows, device, tile_rows=16)
        self.r_q = MlpRun(_critic_descs(m)[0], self.rows, False, device, tile_rows=16)

    def accumulate(self, table: torch.Tensor, idx: torch.Tensor, z: Optional[torch.Tensor], acc: torch.Tensor) -> None:
        """``table``: the store's observations [n, od]; ``idx``: int64 [rows] row indices; ``acc``: fp64 [2 num_q]."""
        lib, m, n = L.load(), self.model, self.rows
        assert idx.dtype == torch.int64 and idx.numel() == n and idx.is_contiguous()
        assert acc.dtype == torch.float64 and acc.numel() == 2 * m.num_q
        L.check(lib.osrl_gather_rows(table.data_ptr(), m.state_dim, idx.data_ptr(), n, self.s0.data_ptr(), m.state_dim,
                                     None, cur_stream()), "osrl_gather_rows")
        q = self.r_q.forward(self.s0, self.pi.forward(self.s0, z))
        L.check(lib.osrl_fqe_value_sums(q.data_ptr(), 2 * m.num_q, n, acc.data_ptr(), cur_stream()),
                "osrl_fqe_value_sums")


def draw_decode_noise(n: int, latent_dim: int, seed: int, device) -> torch.Tensor:
    """The clamped decode noise of ``n`` BCQ-Lag actions, a function of ``seed`` alone."""
    z = torch.zeros(n, latent_dim, dtype=torch.float32, device=device)
    randn_fill(z, int(seed), _Z_STREAM, None)
    G.clamp_(z, -0.5, 0.5)
    return z
