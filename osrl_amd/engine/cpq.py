"""The CPQ train step as a static launch plan on MI355X.

Follows ``CPQTrainer.train_one_step`` (osrl/algorithms/cpq.py:294-313) phase by phase:
``vae_loss`` :125-135 -> ``critic_loss`` :137-153 -> ``cost_critic_loss`` :155-201 ->
``actor_loss`` :203-222 -> ``sync_weight`` :224-230 (fused into each group's Adam kernel).

Every buffer is allocated once; one step is a fixed sequence of ~40 kernel launches with no host
synchronisation, so it is captured in a hipGraph (``torch.cuda.CUDAGraph``) and replayed.
Common sub-expressions the reference recomputes are evaluated once (exact, not approximate):
  * the actor trunk on ``next_observations`` (cpq.py:141 and :159 differ only by the noise draw);
  * the actor trunk on ``observations`` (cpq.py:164 and :209: the actor is not updated in between).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from .. import _lib as L
from ..common.net import actor_head_desc, net_desc_seq, vae_dec_desc, vae_enc_desc
from . import glue as G
from . import plan as P
from ._step import PipelinedReplay, StepEngine, VaePhase
from .core import Branches, DwPlan, MlpRun, StepState, concat_nets

# Plan choices that depend on the shape live in engine/plan.py (cpq_plan: head tails, dW tiles, the all-CU VAE launches, where
# a pipelined graph's next prologue sits and whether its steps are joined; the measurements behind each rule are in
# DESIGN_LOG.md, and so are the placements that were measured, lost and left the code).  Left here: the two lab switches the
# ordering test (tests/test_gpu_pipeline.py) takes its control from -- a no-join graph built WITHOUT one of the two edges that
# order step k's side branch against step k+1's main chain:
#   * plan.vae_adam_side (C2): the VAE's optimizer step runs on step k's side branch, and step k+1's VAE phase, on the main
#     chain, reads what it wrote;
#   * the VAE's optimizer step on the main chain (C4): step k's N*B-row encoder launch, late on its side branch, reads the
#     weights step k+1's optimizer step rewrites ~280 us later, and the main chain's first edge from that branch is the wait
#     for the action draws BEHIND that optimizer step.
# Either way an event behind the launch on the side branch, waited for in front of the actor group's Adam, the last launch of
# step k's main chain.  Read per capture, not per process (_edge): the test builds graphs with and without them.
P.knob("OSRL_VAE_ADAM_EDGE", "actor", "no-join graphs, VAE Adam on the side branch: its edge to the main chain in front of "
       "the actor group's Adam (actor) / none: ordered by timing slack (0, lab)")
P.knob("OSRL_VAE_WAR_EDGE", "actor", "no-join graphs, VAE Adam on the main chain: ordered behind the previous step's N*B-row "
       "encoder launch by an edge to that step's actor Adam (actor) / by timing slack (0, lab)")


def _edge(name: str) -> bool:
    v = P.knob(name, "actor")
    if v not in ("actor", "0"):
        raise ValueError(f"{name}={v!r}: actor or 0")
    return v == "actor"


@dataclass
class Carry:
    """What step k of a pipelined graph leaves for step k+1 (``prev.carry``).  Step k+1 consumes it at the head of its two
    streams: the prologue event in ``_main_vae``, the pending launches in ``_side_first``."""
    dual: bool = False               # step k's dual step is still to be issued (``dual_step()`` clears it)
    polyak: bool = False             # ... and, in front of it, the cost critics' target update (plan.ood_rows)
    ev_prologue: Optional[torch.cuda.Event] = None  # behind step k+1's prologue on step k's side branch, where nothing else ...
    prologue_covered: bool = False   # ... orders it: here the main chain's wait for the critic's Adam is behind it already


@dataclass
class _Step:
    """One issue of the body: what is decided once at its top (``_decide``) and what one phase hands to a later one."""
    par: Branches
    device_noise: bool
    nxt: Optional["CPQEngine"]       # pipelined graphs: the twin engine the NEXT step runs on
    carried: Optional["CPQEngine"]   # ... and the previous step's, where that step left its ``carry`` to this one
    no_join: bool                    # the steps of this graph are not joined (plan.pipe_no_join)
    vae_adam_side: bool              # the VAE's optimizer step at the head of the side branch's second half
    vae_dw_side: bool                # ... and the VAE group's dW launch in front of it
    adam_edge: bool                  # OSRL_VAE_ADAM_EDGE / OSRL_VAE_WAR_EDGE (above)
    war_edge: bool
    ev_vae: Optional[torch.cuda.Event] = None       # main: behind the VAE phase (plan.ood_rows_late: behind the cost critics' dW)
    ev_next2: Optional[torch.cuda.Event] = None     # side: behind the action draws
    ev_critic: Optional[torch.cuda.Event] = None    # side: behind the critic's Adam, its last reader of cost_critic_old
    ev_kl: Optional[torch.cuda.Event] = None        # side, data parallel: behind the KL rows
    ev_vae_adam: Optional[torch.cuda.Event] = None  # side, the edges above: behind the VAE's Adam / the N*B-row encoder launch,
    ev_enc_ood: Optional[torch.cuda.Event] = None   # ... for THIS step's actor phase (nothing of them is left to the next step)
    head_obs: Optional[torch.Tensor] = None         # the actor's head on ``obs`` (the unseeded actor phase's backward reads it)
    qc_s: Optional[torch.Tensor] = None             # the target cost critics on the N*B rows (None with plan.ood_rows)


STAT_KEYS = ["loss/loss_vae", "loss/critic_loss", "loss/cost_critic_loss", "loss/alpha_value", "loss/actor_loss"]
NOISE_KEYS = ["eps_vae", "eps_next_c", "eps_next_cc", "eps_ood", "eps_actor"]


class CPQEngine(PipelinedReplay, VaePhase, StepEngine):
    # (one side branch.  Data parallel: it holds no collective -- every rank issues its RCCL calls from the capture stream,
    # in one order)
    SIDE_STREAMS, PICK_FASTEST, DP_CAPTURE = 1, True, True

    def __init__(self, model, batch_size: int, rows_global: int = 0, seed: int = 0, dist=None):
        m = self.model = model
        B = self.B = int(batch_size)
        self.rows_global = int(rows_global)
        # data parallel: the ranks' rows are different samples of one global batch -> independent noise streams
        self.seed = seed if dist is None else dist.rank_seed(seed)
        self.dist = dist
        dev = torch.device(m.device)
        self.dev = dev
        od, ad, Lz, N = m.state_dim, m.action_dim, m.latent_dim, m.sample_action_num
        f = dict(dtype=torch.float32, device=dev)
        z = lambda *s: torch.zeros(*s, **f)  # noqa: E731
        self.st = StepState(dev, STAT_KEYS)
        self.carry = Carry()  # (pipelined graphs: what this engine's last step left to the next step of its graph)
        # (tests/test_gpu_pipeline.py test_unjoined_graphs_are_ordered_by_edges_not_by_timing: a spin kernel of this many
        # cycles on the side branch in front of its second half -- VAE Adam / N*B-row encoder launch -- of every step)
        self._stress_spin = int(P.knob("OSRL_STRESS_SPIN_CYCLES", "0", "tests: spin kernel (cycles) in front of the side branch's second half"))
        self._stress_at = P.knob("OSRL_STRESS_SPIN_AT", "second", "tests: ... (second) / at the head of the side branch (head) / at the "
                                 "head of the main chain (main)")
        nq, nqc = m.num_q, m.num_qc
        c_hidden = [int(l.out_features) for l in m.cost_critic_old.q_nets[0] if isinstance(l, torch.nn.Linear)][:-1]
        pl = self.plan = P.cpq_plan(od, ad, B, int(m.vae_hidden_sizes), N, seeds=G.SEEDS and G.VAE_TAILS and max(nq, nqc) <= 4
                                    and G.VAE_NS_AUTO, c_hidden=c_hidden)
        # the OOD rows as a set (plan.ood_rows) is a single-GPU plan: the data-parallel step keeps the masked mean over all rows
        self.ood_rows = bool(pl.ood_rows) and dist is None

        # static inputs (a replayed graph reads these addresses)
        self.obs, self.nobs, self.act = z(B, od), z(B, od), z(B, ad)
        self.rew, self.cost, self.done = z(B), z(B), z(B)
        # one flat noise buffer -> one Philox launch per step
        shapes = {"eps_vae": (B, Lz), "eps_next_c": (B, ad), "eps_next_cc": (B, ad), "eps_ood": (N, B, ad),
                  "eps_actor": (B, ad)}
        assert list(shapes) == NOISE_KEYS
        self.noise_flat, self.noise = self.noise_layout(shapes, dev)

        # network descriptors (pointers into the flat groups)
        self.d_actor = actor_head_desc(m.actor)
        self.d_critic = net_desc_seq(list(m.critic.q_nets), 1.0)
        self.d_cost = net_desc_seq(list(m.cost_critic.q_nets), 1.0)
        self.d_critic_old = net_desc_seq(list(m.critic_old.q_nets), 1.0)
        self.d_cost_old = net_desc_seq(list(m.cost_critic_old.q_nets), 1.0)
        self.d_enc = vae_enc_desc(m.vae)
        self.d_dec = vae_dec_desc(m.vae)
        g = m.groups
        m.repack()

        # ---- vae phase
        self._vae_runs(dev)
        # 1024 rows per split-K slab (the default policy gives 256): 140 tiles x 2 splits = 280 workgroups fit the 512
        # resident slots in one round (x 4 splits = 560: a second, almost empty round), and the Adam kernel sums two
        # slabs instead of four.  In the step: 2175 steps/s vs 2135 (4 splits), 2140 (3), 2015 (1); the other groups
        # measure best at the default 256 rows (2175 vs 2110 at 512, 2010 at 1024)
        # round 3: 400-wide layers are 25 = 5 x 5 column blocks -- on 80 x 80 tiles with a flat (tile, split) work list
        # the VAE's dW is 250 even workgroups in one round (core.DwPlan tile_blocks; OSRL_VAE_DW_T5=0: the 64 x 64 form)
        if pl.vae_dw_tile:
            self.p_vae = DwPlan(g["vae"], self.r_enc.dw_entries() + self.r_dec.dw_entries(), B, dev,
                                n_splits=pl.vae_dw_splits, tile_blocks=pl.vae_dw_tile)  # 70 tiles x 3 splits = 210 workgroups: one round (tools/dw_bench.py)
        else:
            self.p_vae = DwPlan(g["vae"], self.r_enc.dw_entries() + self.r_dec.dw_entries(), B, dev,
                                n_splits=pl.vae_dw_splits)

        # ---- critic phase
        self.r_actor_next = MlpRun(self.d_actor, B, False, dev)
        self.a_next = z(B, ad)
        self.r_old_next = MlpRun(concat_nets(self.d_critic_old, self.d_cost_old), B, False, dev)
        self.r_critic = MlpRun(self.d_critic, B, True, dev)
        self.dq = z(nq, B, 1)
        self.r_critic.setup_backward(self.dq)
        # round 4: the two critic groups' dW on 32 x 32 tiles x 2 row splits (17 KB of LDS, 154 registers per lane): such
        # workgroups fit on a CU beside the 8-wave N*B-row encoder launch (130 KB, 2 x 152 registers per SIMD), which a
        # 64 x 64 tile's 68 KB / 304 registers do not -- the cost critics' dW runs beside that launch on the main branch
        # (84 -> 65 us there; C2 2245 -> 2260-2267 steps/s with both groups, gpurun_out/r4c)
        t_def, s_def = ("2", 2) if pl.small_dw else ("0", None)
        self.p_critic = DwPlan(g["critic"], self.r_critic.dw_entries(), B, dev,
                               tile_blocks=int(P.knob("OSRL_DW_T_CRITIC", t_def, "dW tile of the critic group (16-blocks)")),
                               n_splits=(int(P.knob("OSRL_DW_S_CRITIC", "0")) if P.knob_set("OSRL_DW_S_CRITIC") else s_def))

        # ---- cost-critic phase
        self.a_next2 = z(B, ad)
        self.r_costold_next = MlpRun(self.d_cost_old, B, False, dev)
        self.r_actor_obs = MlpRun(self.d_actor, B, True, dev)  # also the actor forward of the actor phase
        self.sampled = z(N * B, ad)
        # Both N*B-row forwards (target cost critics beside the VAE phase, VAE encoder beside the cost-critic phase)
        # take the 80-row one-workgroup-per-CU kernel (csrc/mlp.hip mlp_fwd_nb_kernel): 73 / 71 us alone vs 98 / 88 us
        # for 32-row tiles.  Its 84 KB (256-wide) / 134 KB (400-wide) of LDS per workgroup leave the chain's launches
        # room on every CU.  (Until the kernel's epilogue / bias / stage-in rework of round 2 the capped 32-row tile
        # loop was the better neighbour for the VAE phase: 1968 vs 1876 steps/s; now 80-row tiles give 2095 vs 2020.
        # OSRL_OOD_TILE=0 OSRL_OOD_WG_CAP=512 restores the old form.)
        ood_tile = pl.ood_tile
        self.r_costold_ood = MlpRun(self.d_cost_old, N * B, False, dev,
                                    wg_cap=int(P.knob("OSRL_OOD_WG_CAP", "0", "workgroup cap of the N*B cost-critic launch")),
                                    tile_rows=ood_tile)
        self.r_enc_ood = MlpRun(self.d_enc, N * B, False, dev,
                                wg_cap=int(P.knob("OSRL_ENC_WG_CAP", "0", "workgroup cap of the N*B encoder launch")),
                                tile_rows=int(P.knob("OSRL_ENC_TILE", str(ood_tile or 80), "row tile of the N*B encoder launch")))
        # shared-observation tiles of the two N*B-row launches (plan.ood_share): their rows are the B observations N times over
        # (cpq.py:164-176), so the observation part of layer 0 runs once per observation of a tile (osrl_rows_t.share0)
        self.pre_cost = self.pre_enc = 0
        if pl.ood_share and ood_tile == 80:
            if not self.ood_rows:  # (a row SET has no tiles of shared observations)
                self.pre_cost = self.r_costold_ood.share_k16(od, B, N)
            if not self.ood_rows or P.knob("OSRL_OOD_ROWS_ENC_SHARE", "1", "plan.ood_rows: the N*B-row encoder launch keeps its shared-observation tiles: 1 / 0") == "1":
                self.pre_enc = self.r_enc_ood.share_k16(od, B, N)
        self.kl = z(N * B)
        self.quant = z(4)
        self.ood_mean = z(4)
        self.ood_list = torch.zeros(N * B, dtype=torch.int32, device=dev)  # plan.ood_rows: the rows with KL >= quantile, ascending
        self.ood_count = torch.zeros(4, dtype=torch.int32, device=dev)
        self.r_cost = MlpRun(self.d_cost, B, True, dev)
        self.dqc = z(nqc, B, 1)
        self.r_cost.setup_backward(self.dqc)
        self.p_cost = DwPlan(g["cost_critic"], self.r_cost.dw_entries(), B, dev,
                             tile_blocks=int(P.knob("OSRL_DW_T_COST", t_def, "dW tile of the cost-critic group (16-blocks)")),
                             n_splits=(int(P.knob("OSRL_DW_S_COST", "0")) if P.knob_set("OSRL_DW_S_COST") else s_def))

        # ---- actor phase
        self.a_pi, self.tanh_u = z(B, ad), z(B, ad)
        self.r_pi_q = MlpRun(concat_nets(self.d_critic, self.d_cost), B, True, dev, save_nets=list(range(nq)))
        self.dq_pi = z(nq, B, 1)
        self.r_pi_q.setup_backward(self.dq_pi, need_dz=False, dx_cols=(od, ad))
        self.dhead_actor = z(1, B, 2 * ad)
        self.r_actor_obs.setup_backward(self.dhead_actor)
        self.p_actor = DwPlan(g["actor"], self.r_actor_obs.dw_entries(), B, dev)

        # ---- loss seeds (round 4): each backward launch computes the gradient it starts from (glue.seed_*,
        # osrl_mlp_backward_dz_seed) -- the five loss launches between a forward and a backward leave the chains
        rg = self.rows_global
        st = self.st
        self.seeds = None
        if G.SEEDS and G.VAE_TAILS and max(nq, nqc) <= 4:
            y_old, y_pi = self.r_old_next.y, self.r_pi_q.y
            self.seeds = {
                "vae": self._vae_seed(dev),
                "critic": G.seed_cpq_critic(y_old[:nq], nq, y_old[nq:], nqc, self.rew, self.done, B, m.gamma, m.q_thres,
                                            rg, G.SeedStat(dev, nq, B), st.stat_ptr("loss/critic_loss")),
                "cost": G.seed_cpq_cost(self.r_costold_next.y, nqc, self.cost, B, m.gamma, rg, G.SeedStat(dev, nqc, B),
                                        st.stat_ptr("loss/cost_critic_loss")),
                "actor": G.seed_cpq_actor(y_pi[:nq], nq, y_pi[nq:], nqc, B, m.q_thres, rg, G.SeedStat(dev, nq, B),
                                          st.stat_ptr("loss/actor_loss")),
                "head": G.seed_gauss_head(self.noise["eps_actor"], self.tanh_u, self.r_pi_q.dx, nq, B, m.max_action),
            }

        self._vae_all_cu()  # (round 5)
        self._plans_built()
        self.parallel_branches = True
        self._probe = None

    # ------------------------------------------------------------------ #
    def _optim(self, name: str, plan: DwPlan, tau: float = 0.0, extra=None) -> None:
        """(the base's, plus bench.py's ``vae_dw`` probe and the fused dW + Adam launch)"""
        if name == "vae":
            self._pr("vae_dw", 0)
        if self.dist is None and plan.can_fuse_adam():  # dW and the optimizer step in one launch (same bits)
            plan.launch_adam(self.model._lrs[name], self.st.ptr, tau=tau)
            if name == "vae":
                self._pr("vae_dw", 1)
            return
        plan.launch()
        if name == "vae":
            self._pr("vae_dw", 1)
        self._update(name, tau, extra)

    def _pr(self, site: str, i: int) -> None:
        """bench.py's in-step probe: HIP events (on the launching stream) around a named launch of the step body."""
        if self._probe is not None and site in self._probe:
            p = self._probe[site]
            if isinstance(p, int):  # device address of three uint64: stamps INSIDE the captured graph (osrl_stamp_realtime)
                cs = torch.cuda.current_stream().cuda_stream
                L.check(L.load().osrl_stamp_realtime(p + 8 * i, cs), "osrl_stamp_realtime")
                if i == 1:  # a second stamp right behind the closing one: the cost of a stamp itself (bench.py subtracts it)
                    L.check(L.load().osrl_stamp_realtime(p + 16, cs), "osrl_stamp_realtime")
            else:
                p[i].record()

    def prologue(self, device_noise: bool) -> None:
        """tick + minibatch gather + Philox noise of ONE step into this engine's buffers (one launch)."""
        self.st.prologue(self.replay, (self.obs, self.nobs, self.act, self.rew, self.cost, self.done), self.noise_flat,
                         self.seed, device_noise)

    def body(self, device_noise: bool, par: Optional[Branches] = None, nxt: Optional["CPQEngine"] = None,
             prologue_done: bool = False, prev: Optional["CPQEngine"] = None) -> None:
        """One step, single GPU or data parallel (``self.dist``): the launch plan below.

        What the plan exploits (cpq.py:155-201): everything the OOD penalty is made of -- the N*B sampled actions, the
        target cost critics on them, the VAE encoder on them, the KL rows, their 0.75-quantile, ``qc_ood`` -- sits
        under ``torch.no_grad()`` and enters the cost-critic loss as ``- exp(log_alpha) * (qc_ood.mean() - thres)``,
        a term with NO gradient to any network.  It moves ``log_alpha`` and the logged loss, nothing else.  So the
        69 % of the step's FLOPs that live in the two N*B-row launches are not on the path of any parameter update,
        and the plan keeps them off the latency chain:

          main  : vae phase -> cost-critic phase (MSE part only) -> [critic updated] -> actor phase
          side  : actor forwards + heads -> target cost critics on the N*B rows -> critic phase ->
                  (vae updated) encoder on the N*B rows -> KL -> quantile -> qc_ood mean -> dual step + logged loss

        The side branch joins at the END of the step.  Ordering constraints kept by events: the cost-critic Adam also
        Polyak-updates ``cost_critic_old``, so it waits for the side branch's last reader of the targets; the encoder on
        the N*B rows waits for the VAE's Adam; the actor phase waits for the critic's Adam.

        ``nxt`` / ``prologue_done`` / ``prev`` (engine/pipeline.py, several steps per graph): the NEXT step's prologue --
        into the twin engine ``nxt``'s buffers and step state -- is issued on THIS step's side branch (``_next_prologue``)
        and the next step is run with ``prologue_done=True``; what else this step leaves to the next one is ``self.carry``,
        which the next step reads through ``prev``."""
        par = par or Branches(False)
        assert nxt is None or self.dist is None, "pipelined steps are a single-GPU plan"
        if not prologue_done:
            self.prologue(device_noise)
        s = self._decide(device_noise, par, nxt, prev)
        self._main_vae(s)
        self._side_first(s)
        self._main_cost(s)
        self._side_second(s)
        self._main_actor(s)
        self._tail(s)

    def _decide(self, device_noise: bool, par: Branches, nxt, prev) -> _Step:
        """Every plan flag of one issue, once."""
        pl, single = self.plan, self.dist is None
        # plan.pipe_no_join (pipelined graphs): the steps of a graph are not joined.  The main chain of step k+1 waits for
        # its prologue only (issued on step k's side branch: ``carry.ev_prologue``), and step k's dual step runs at the head
        # of step k+1's side branch, right behind the fork -- the one place of the side branch that already has an edge from
        # the END of step k's main chain (so both halves of the logged cost loss are there) without a new mid-chain edge.
        no_join = pl.pipe_no_join and par.enabled and single
        # (single GPU, plan.vae_adam_side: the VAE's optimizer step at the head of the side branch's second half, in
        # front of its only reader, instead of on the main chain -- +0.7 % at C2, DESIGN_LOG round 5)
        vae_adam_side = single and par.enabled and pl.vae_adam_side and not self.p_vae.can_fuse_adam()
        adam_edge, war_edge = _edge("OSRL_VAE_ADAM_EDGE"), _edge("OSRL_VAE_WAR_EDGE")
        # (plan.vae_dw_side: the VAE group's dW too -- its only reader is that optimizer step.  Not where the lab switch
        # OSRL_VAE_ADAM_EDGE=0 takes away the edge that orders it in a no-join graph)
        vae_dw_side = bool(vae_adam_side and self.ood_rows and pl.vae_dw_side and not (no_join and not adam_edge))
        carried = prev if (no_join and prev is not None and prev.carry.dual) else None
        self.carry = Carry()
        return _Step(par, device_noise, nxt, carried, no_join, vae_adam_side, vae_dw_side, adam_edge, war_edge)

    def _next_prologue(self, s: _Step, site: str) -> None:
        """Pipelined graphs: the next step's prologue (its minibatch + noise + tick, 14 us) at ``site`` of this step's side
        branch, if that is where the plan puts it (plan.pipe_prologue; engine/plan.py has the measurements: where it sits
        decides how the N*B-row launch behind it lines up with the main chain's all-CU VAE launches).  Called at every
        candidate site, in issue order: "head" = first on the branch (the N*B-row launch behind it starts ~14 us later against
        the main chain's VAE launches), "critic" = in front of the critic phase, "early" = in front of the OOD statistic (C2:
        +1.2 .. +2.6 % against +0.5 % behind it, DESIGN_LOG round 6)."""
        if s.nxt is None or self.plan.pipe_prologue != site:
            return
        s.nxt.prologue(s.device_noise)
        if site in ("head", "critic"):
            # the main chain waits for this branch's critic Adam (ev_critic), which is behind this launch: the next step's
            # first launch needs no edge of its own from this branch
            self.carry.prologue_covered = True
        elif self.ood_rows:
            # "early" with plan.ood_rows: issued, but NO event for the next step -- the step then has nothing to carry on
            # (_tail) and stays JOINED, whatever plan.pipe_no_join says.  (A no-join graph with this placement would be a
            # graph form of its own; the pinned plans put the prologue at "head" / "critic" wherever rows are selected.)
            pass
        else:
            self.carry.ev_prologue = s.par.mark(0)

    def _main_vae(self, s: _Step) -> None:
        """Main: what the previous step left for this chain, the fork, vae_loss (cpq.py:125-135), and where the VAE group's
        dW and Adam go."""
        par = s.par
        if s.carried is not None:
            par.wait(s.carried.carry.ev_prologue)
        par.fork(0)
        if self._stress_spin and par.enabled and self._stress_at == "main":
            torch.cuda._sleep(self._stress_spin)  # (tests: the main chain arrives late)
        self._vae_phase(self.seeds)
        if not s.vae_adam_side:
            self._optim("vae", self.p_vae, 0.0)
        elif not s.vae_dw_side:  # (the optimizer step alone goes to the side branch's second half)
            self._pr("vae_dw", 0)
            self.p_vae.launch()
            self._pr("vae_dw", 1)
        if par.enabled:
            s.ev_vae = torch.cuda.Event()
            s.ev_vae.record()

    def _side_first(self, s: _Step) -> None:
        """Side, first half: what the previous step carried over, the actor forwards + heads, the target cost critics on the
        N*B rows (beside the VAE phase, where the capped tile loop disturbs the chain least), then the critic phase."""
        m, st, nz, B, par, sd = self.model, self.st, self.noise, self.B, s.par, self.seeds
        ad, N, nq, nqc = m.action_dim, m.sample_action_num, m.num_q, m.num_qc
        with par.on(0):
            if self._stress_spin and par.enabled and self._stress_at == "head":
                torch.cuda._sleep(self._stress_spin)  # (tests: the side branch arrives late)
            if s.carried is not None:
                if s.carried.carry.polyak:
                    # (plan.ood_rows in a no-join graph: the cost critics' target update of the previous step -- behind its last
                    # reader, the forward on the selected rows at that step's side-branch tail, and behind its main chain's
                    # optimizer step, which this branch's fork waited for; in front of this step's readers of the targets: the
                    # critic phase on this branch, the cost phase on the main chain through its wait for the action draws)
                    m.groups["cost_critic"].polyak_step(m.tau)
                    s.carried.carry.polyak = False
                # (created HERE, behind the main chain's VAE launches: the graph executor keeps the FIRST-created successor
                # of a node on that node's queue -- issued right at the fork, the dual step was the first successor of the
                # previous step's last Adam and the two chains swapped queues at every boundary: 2155 vs 2320 steps/s)
                s.carried.dual_step()
            self._next_prologue(s, "head")
            if self.plan.head_tails:
                # every action draw of the step (cpq.py:141 a_next, :159 a_next2, :164-176 the N OOD draws, :209 the
                # actor-phase sample) by the actor trunks' own forward launch, from its LDS-resident head tiles: four
                # single-purpose launches (30 us on this branch inside the step, profiles/r3_timeline_*.txt) fewer
                hn, ho = self.r_actor_next.forward_with(
                    (self.nobs,), self.r_actor_obs, (self.obs,),
                    tail=G.gauss_tail(ad, m.max_action, eps=nz["eps_next_cc"], a=self.a_next2, eps2=nz["eps_next_c"],
                                      a2=self.a_next),
                    other_tail=G.gauss_tail(ad, m.max_action, eps2=nz["eps_actor"], a2=self.a_pi, tanh2=self.tanh_u,
                                            eps_ood=nz["eps_ood"], n_samples=N, sampled=self.sampled))
                s.head_obs = ho[0]
                s.ev_next2 = par.mark(0)
            else:
                hn, ho = self.r_actor_next.forward_with((self.nobs,), self.r_actor_obs, (self.obs,))
                head_next, s.head_obs = hn[0], ho[0]
                G.gauss_head(head_next, nz["eps_next_cc"], B, ad, m.max_action, a=self.a_next2)
                s.ev_next2 = par.mark(0)
                G.gauss_head(head_next, nz["eps_next_c"], B, ad, m.max_action, a=self.a_next)
                G.gauss_ood_sample(s.head_obs, nz["eps_ood"], N, B, ad, self.sampled)
                # the actor-phase sample (cpq.py:209) needs only this forward and its own noise
                G.gauss_head(s.head_obs, nz["eps_actor"], B, ad, m.max_action, a=self.a_pi, tanh_u=self.tanh_u)
            if not self.ood_rows:  # (plan.ood_rows: this forward runs BEHIND the KL quantile, on the rows that pass it)
                self._pr("costold_ood", 0)
                s.qc_s = self.r_costold_ood.forward(self.obs, self.sampled, map0=L.MAP_MOD, div0=B, share_k16=self.pre_cost)
                self._pr("costold_ood", 1)
            self._next_prologue(s, "critic")
            # critic_loss (cpq.py:137-153)
            self._pr("critic_fwd", 0)
            y_old, q = self.r_old_next.forward_with((self.nobs, self.a_next), self.r_critic, (self.obs, self.act))
            self._pr("critic_fwd", 1)
            if sd is not None:
                self.r_critic.backward_dz(seed=sd["critic"])
            else:
                G.cpq_critic_loss(y_old[:nq], nq, y_old[nq:], nqc, q, nq, self.rew, self.done, B, m.gamma, m.q_thres,
                                  self.rows_global, self.dq, st.stat_ptr("loss/critic_loss"))
                self.r_critic.backward_dz()
            if self.dist is None:
                self._optim("critic", self.p_critic, m.tau)
            else:  # collectives stay on the capture stream (same order on every rank): reduced + stepped over there
                self.p_critic.launch()
                if P.knob("OSRL_DP_SIDE_REDUCE", "1", "DP: the critic group's slab sum on the side branch") == "1":
                    self.dist.reduce_local(m.groups["critic"])  # the per-rank slab sum is no collective: off the main chain
            s.ev_critic = par.mark(0)  # also: the side branch's last reader of cost_critic_old is enqueued

    def _main_cost(self, s: _Step) -> None:
        """Main: cost_critic_loss (cpq.py:155-201), the part with a gradient: Bellman MSE of the online cost critics."""
        m, st, B, par, sd, dp = self.model, self.st, self.B, s.par, self.seeds, self.dist
        nqc = m.num_qc
        par.wait(s.ev_next2)
        qc_old_next, qc = self.r_costold_next.forward_with((self.nobs, self.a_next2), self.r_cost, (self.obs, self.act))
        if sd is not None:
            self.r_cost.backward_dz(seed=sd["cost"])
        else:
            G.cpq_cost_loss(qc_old_next, nqc, qc, nqc, None, self.cost, B, m.gamma, m.qc_thres, m.alpha_lr, self.rows_global,
                            1.0, None, self.dqc, st.stat_ptr("loss/cost_critic_loss"))
            self.r_cost.backward_dz()
        fuse_cost = dp is None and self.p_cost.can_fuse_adam() and not self.ood_rows
        if not fuse_cost:
            self.p_cost.launch()
        if self.ood_rows and s.ev_vae is not None and self.plan.ood_rows_late:
            # (plan.ood_rows_late: without the N*B-row cost-critic launch in its first half the side branch reaches the VAE's
            # Adam + the N*B-row encoder launch ~70 us earlier -- beside THIS dW launch, whose 384 small workgroups then take
            # 70 instead of 25 us, gpurun_out/r6oodrows3; the side branch waits for this point instead of the VAE's dW)
            s.ev_vae = torch.cuda.Event()
            s.ev_vae.record()
        par.wait(s.ev_critic)  # Adam + Polyak of this group rewrites cost_critic_old: after its readers on the side branch
        if fuse_cost:
            self.p_cost.launch_adam(m._lrs["cost_critic"], st.ptr, tau=m.tau)
        elif self.ood_rows:
            # the targets' LAST reader of this step -- the forward on the selected OOD rows -- runs at the end of the side
            # branch: the optimizer step here without its Polyak half, the target update behind that reader (polyak_step)
            m.groups["cost_critic"].adam_step(m._lrs["cost_critic"], st.ptr, tau=m.tau, polyak=False)
        elif dp is None:
            self._update("cost_critic", m.tau)
        else:
            self._update_critics_dp()

    def _side_second(self, s: _Step) -> None:
        """Side, second half: the OOD statistic with the UPDATED vae -- the VAE's dW and Adam where the plan puts them here,
        the encoder on the N*B rows, the statistic in its three forms.
        (Round 4, measured and dropped: letting this half wait for the cost critics' optimizer step instead -- so that it
        does not stretch the cost phase it runs beside -- is SLOWER, 2161-2165 vs 2242-2244 steps/s at C2, 2257 vs 2285 at
        C4: the step is throughput-bound, the N*B-row work has to start as early as its inputs allow.)"""
        m, B, par = self.model, self.B, s.par
        N, nqc, rg = m.sample_action_num, m.num_qc, self.rows_global
        carries_on = s.no_join and s.nxt is not None
        with par.on(0):
            par.wait(s.ev_vae)
            if self._stress_spin and par.enabled and self._stress_at == "second":
                torch.cuda._sleep(self._stress_spin)  # (tests: this branch's second half arrives LATE; results must not move)
            if s.vae_adam_side:
                if s.vae_dw_side:
                    # (engine/plan.py vae_dw_side.  Reads the activation and dZ buffers the main chain's VAE phase wrote: this
                    # branch waited for ev_vae above, recorded behind that phase -- or, with plan.ood_rows_late, further down
                    # the same chain)
                    self._pr("vae_dw", 0)
                    self.p_vae.launch()
                    self._pr("vae_dw", 1)
                self._update("vae", 0.0)  # (engine/plan.py vae_adam_side: off the main chain, in front of its only reader)
                if carries_on and s.adam_edge:
                    # ... of THIS step: the next step's VAE phase, on the main chain, reads it too, and steps that are not
                    # joined need an edge of their own for that.  With plan.vae_dw_side the same edge carries a second
                    # dependency: the next step's VAE phase REWRITES the activation and dZ buffers this step's dW launch
                    # reads.  The optimizer step follows the dW launch on this stream and the event is recorded behind it, so
                    # whoever waits for it is behind both (a joined step, or the last step of a graph, has the join for that).
                    s.ev_vae_adam = par.mark(0)
            self._pr("enc_ood", 0)  # bench.py: HIP events around the dominant launch as it runs inside the step
            # (the KL rows of cpq.py:178-182 by the encoder launch itself: OSRL_TAIL_VAE_KL)
            self.r_enc_ood.forward(self.obs, self.sampled, map0=L.MAP_MOD, div0=B, tail=G.vae_kl_tail(m.latent_dim, self.kl),
                                   share_k16=self.pre_enc)
            self._pr("enc_ood", 1)
            if carries_on and s.war_edge and not s.vae_adam_side:
                s.ev_enc_ood = par.mark(0)  # (the next step's VAE Adam, on the main chain, rewrites what this launch read)
            self._next_prologue(s, "early")
            if self.dist is not None:  # (the batch-GLOBAL quantile: gathered from the main branch, _main_actor)
                s.ev_kl = par.mark(0)
            elif self.ood_rows:
                # cpq.py:183-184 as a row SET: quantile + ascending list of the rows with KL >= quantile in one
                # single-workgroup launch, the target cost critics on those rows (a quarter of N*B; the grid is sized for
                # all of them, workgroups past the count leave at once), their sum.  The cost critics' target update follows
                # on the MAIN branch behind the join (a main -> side edge this late makes the graph executor serialise the
                # actor phase behind this branch: 500 vs 428 us per step, profiles/r6_ood_rows_timeline_side_polyak.txt).
                G.cpq_ood_select(self.kl, N * B, 0.75, self.quant, self.ood_list, self.ood_count)
                self._pr("costold_ood", 0)
                qc_sel = self.r_costold_ood.forward(self.obs, self.sampled, map0=L.MAP_MOD, div0=B, row_list=self.ood_list,
                                                    n_rows_dev=self.ood_count)
                self._pr("costold_ood", 1)
                G.cpq_ood_sum(qc_sel, nqc, N * B, self.ood_count, 1.0 / (float(N) * float(rg if rg > 0 else B)), self.ood_mean)
            elif N * B <= 32768:  # quantile + masked mean in one single-workgroup launch (keys in registers)
                G.cpq_ood_stat(s.qc_s, nqc, self.kl, 0.75, N, B, rg, self.quant, self.ood_mean)
            else:
                G.quantile(self.kl, N * B, 0.75, self.quant)
                G.cpq_ood_mean(s.qc_s, nqc, self.kl, self.quant, N, B, rg, self.ood_mean)

    def _main_actor(self, s: _Step) -> None:
        """Main: actor_loss (cpq.py:203-222): needs the updated critic (side branch: this stream waited for ev_critic in the
        cost phase -- a second wait on it is one more graph edge, ~6 us on the chain) and cost critic (this chain)."""
        m, st, nz, B, par, sd, dp = self.model, self.st, self.noise, self.B, s.par, self.seeds, self.dist
        ad, N, nq, nqc, rg = m.action_dim, m.sample_action_num, m.num_q, m.num_qc, self.rows_global
        self._pr("actor_phase_fwd", 0)
        y = self.r_pi_q.forward(self.obs, self.a_pi)
        self._pr("actor_phase_fwd", 1)
        if dp is not None:
            # the batch-GLOBAL quantile (cpq.py:183 over all world * N * B values): the gather is a collective, so it
            # is issued from the capture stream -- here, behind the actor phase's forward launch, which is about when
            # the side branch has its KL rows (profiles/r2_timeline.txt: 397 us vs 405 us); the selection and the
            # masked mean go back to the side branch and run beside the actor phase's backward
            par.wait(s.ev_kl)
            kl_all = dp.all_gather_concat(self.kl)
            ev_g = torch.cuda.Event() if par.enabled else None
            if ev_g is not None:
                ev_g.record()
            with par.on(0):
                par.wait(ev_g)
                dp.quantile_select(kl_all, 0.75, self.quant)
                G.cpq_ood_mean(s.qc_s, nqc, self.kl, self.quant, N, B, rg, self.ood_mean)
        if sd is not None:
            self.r_pi_q.backward_dz(seed=sd["actor"])
            self.r_actor_obs.backward_dz(seed=sd["head"])
        else:
            G.cpq_actor_loss(y[:nq], nq, y[nq:], nqc, B, m.q_thres, rg, self.dq_pi, st.stat_ptr("loss/actor_loss"))
            self.r_pi_q.backward_dz()
            G.gauss_head_bwd(s.head_obs, nz["eps_actor"], self.tanh_u, self.r_pi_q.dx, nq, B, ad, m.max_action,
                             self.dhead_actor)
            self.r_actor_obs.backward_dz()
        if dp is None:
            # (no-join graphs: the two edges from this step's side branch, in front of the last launch of this chain)
            par.wait(s.ev_vae_adam)
            par.wait(s.ev_enc_ood)
            self._optim("actor", self.p_actor, m.tau)
        else:  # (its gradient is reduced behind the join: _tail)
            self.p_actor.launch()

    def _tail(self, s: _Step) -> None:
        """Carry on into the next step of a no-join graph, or join the side branch and run the dual step."""
        m, st, c = self.model, self.st, self.carry
        if s.no_join and s.nxt is not None and (c.ev_prologue is not None or c.prologue_covered):
            c.dual = True  # (the next step of this graph runs it: dual_step())
            c.polyak = bool(self.ood_rows)
            return
        s.par.join(0)
        if self.dist is not None:  # actor gradient, the per-rank partial statistics and the partial qc_ood mean in one collective
            self._update("actor", m.tau, extra=[st.stats, self.ood_mean])
        # dual step + the OOD term of the logged loss (cpq.py:186-195): after the join, so that the side branch has no
        # incoming edge from the main branch after the VAE's Adam (the graph executor keeps two linear chains); under
        # data parallelism the statistics are already the global ones here, so the global term is added once
        if self.ood_rows:  # the cost critics' target update: behind its last reader (side branch, joined above)
            m.groups["cost_critic"].polyak_step(m.tau)
        self.dual_step()

    def dual_step(self) -> None:
        """log_alpha's ascent + the OOD term of this step's logged cost loss (cpq.py:186-195), on the current stream."""
        m = self.model
        G.cpq_alpha_step(self.ood_mean, m.qc_thres, m.alpha_lr, 1.0, m.log_alpha, self.st.stat_ptr("loss/cost_critic_loss"))
        self.carry.dual = False

    def _branches(self) -> Branches:
        # (data parallel: a second stream that no launch uses since OSRL_DP_SIDE_COLL left -- kept, because the streams that
        # exist at capture decide the branch -> hardware-queue mapping (core.pick_fastest): without it C2 under forced data
        # parallelism 2149-2152 against 2154-2159 steps/s, with it 2165-2174 against 2160-2168, profiles/cpq_body_ab.json)
        return Branches(self.parallel_branches, 2 if self.dist is not None else 1)
