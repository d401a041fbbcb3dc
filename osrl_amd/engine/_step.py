"""What the six train-step engines share (engine/bc.py, cpq.py, bcql.py, bearl.py, coptidice.py, cdt.py).

An engine's ``__init__`` allocates its buffers and plans and ends with ``_plans_built()``; its ``body()`` issues one step.
Everything around the body is here, once: the flat noise buffer, the snapshot of the training state, the hipGraph
capture (always undone in ``finally``), replay-or-eager, ``step`` / ``step_replay`` over the engine's batch fields, and
the optimizer-step helpers.  ``PipelinedReplay`` (CPQ, BCQ-Lag) adds several steps per graph, ``VaePhase`` (CPQ, BCQ-Lag,
BEAR-Lag) the VAE phase the three share.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import torch

from . import core as _core
from . import glue as G
from .core import (Branches, DwPlan, MlpRun, capture_restoring, check_plans_current, load_into, pick_fastest,
                   scalar_state, slab_epochs)


class StepEngine:
    BATCH: Tuple[str, ...] = ("obs", "nobs", "act", "rew", "cost", "done")  # the batch buffers, in ``step()``'s order
    SIDE_STREAMS = 0      # side branches of the captured step (``body(device_noise, par)``); 0: ``body`` takes no ``par``
    PICK_FASTEST = False  # with OSRL_CAPTURE_TRIES > 1: capture a branched step that often, keep the fastest graph
    # the step is captured under data parallelism too, collectives included (CPQ, CDT); the others run it eagerly there
    DP_CAPTURE = False
    parallel_branches = True
    graph: Optional[torch.cuda.CUDAGraph] = None
    replay = None
    _replay_epoch = 0
    _graph_failed = False

    @staticmethod
    def noise_layout(shapes: Dict[str, tuple], device) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
        """One flat noise buffer (-> one Philox launch per step) and a view per key, back to back in the mapping's
        order; the total padded to a multiple of 4 floats."""
        sizes = [int(torch.Size(s).numel()) for s in shapes.values()]
        flat = torch.zeros((sum(sizes) + 3) // 4 * 4, dtype=torch.float32, device=device)
        views, o = {}, 0
        for (k, s), n in zip(shapes.items(), sizes):
            views[k] = flat[o:o + n].view(s)
            o += n
        return flat, views

    def _plans_built(self) -> None:
        # every dW plan of this engine is built: the slab epochs they were built against are recorded NOW (not at the
        # first step), so an engine that is constructed directly, never stepped and then superseded is flagged stale
        self._slab_epochs = slab_epochs(self.model)

    # ---- the training state a step advances ---------------------------------------------------------------------------
    def _snap_groups(self):
        return self.model.groups.values()

    def _state_tensors(self):
        st = self.st
        out = [b for g in self._snap_groups() for b in (g.p, g.m, g.v, g.tgt) if b is not None]
        return out + [st.state, st.stats, st.ring] + scalar_state(self.model, self)

    def _snapshot(self):
        return [t.clone() for t in self._state_tensors()], self.st.host_step

    def _restore(self, snap) -> None:
        for t, c in zip(self._state_tensors(), snap[0]):
            t.copy_(c)
        self.st.host_step = snap[1]
        self.model.repack()

    # ---- capture and replay -------------------------------------------------------------------------------------------
    def _branches(self) -> Optional[Branches]:
        return Branches(self.parallel_branches, self.SIDE_STREAMS) if self.SIDE_STREAMS else None

    def _issue(self, par: Optional[Branches] = None) -> None:
        """One step on device-drawn inputs: what the warm-up pass, the capture and the eager path run."""
        if par is None:
            self.body(True)
        else:
            self.body(True, par)

    def _capture_once(self):
        par = self._branches()
        g, arena = capture_restoring(self.st.state.device, lambda: self._issue(par), self._snapshot, self._restore)
        return g, par, arena  # (the side streams and the argument blocks the kernels read stay alive with the graph)

    def capture(self) -> None:
        """Capture one step (device-drawn noise) into a hipGraph; the training state the warm-up and capture passes
        advance is put back.  ``PICK_FASTEST``: on one GPU a few times over, keeping the graph whose replays are
        fastest (core.pick_fastest: the branch -> hardware-queue mapping depends on the streams created before)."""
        tries = _core.CAPTURE_TRIES if (self.PICK_FASTEST and self.dist is None and self.parallel_branches) else 1
        (self.graph, self._par, self._arena), self.capture_ms = pick_fastest(
            self._capture_once, lambda c: c[0].replay(), self._snapshot, self._restore, tries)

    def _run(self, use_graph: bool) -> None:
        """Replay the captured step (capturing it first), or issue it eagerly.  ``DP_CAPTURE``: with a DataParallel hook
        the collectives are captured into the same hipGraph; if the runtime refuses (older RCCL), every rank falls
        back to eager launches."""
        dp = self.dist
        if dp is not None and (not self.DP_CAPTURE or os.environ.get("OSRL_DP_EAGER") == "1"):
            use_graph = False  # (the operator override: a data-parallel step without its collectives captured)
        if use_graph and not self._graph_failed:
            if self.graph is None:
                ok = True
                try:
                    self.capture()
                except Exception as e:  # pragma: no cover - depends on the RCCL build
                    if dp is None:
                        raise
                    import warnings
                    warnings.warn(f"hipGraph capture of the data-parallel step failed ({e!r}); running eagerly")
                    ok = False
                if dp is not None and not dp.all_agree(ok, self.st.state.device):
                    self._graph_failed, self.graph = True, None  # every rank runs eagerly, or none does
            if self.graph is not None:
                self.graph.replay()
                self.st.host_step += 1
                return
        self._issue()

    # ---- the public step ----------------------------------------------------------------------------------------------
    def load_batch(self, *batch) -> None:
        """Caller tensors into the static batch buffers, in ``BATCH`` order (observations, next_observations, actions,
        rewards, costs, done for the Q-learning engines)."""
        if len(batch) != len(self.BATCH):
            raise TypeError(f"{type(self).__name__} takes {len(self.BATCH)} batch tensors ({', '.join(self.BATCH)}), "
                            f"got {len(batch)}")
        load_into(tuple((getattr(self, k), v) for k, v in zip(self.BATCH, batch)))

    def load_noise(self, noise: Dict[str, torch.Tensor]) -> None:
        if getattr(self, "noise", None) is None:
            raise TypeError(f"{type(self).__name__} draws no noise: step() takes no noise= for it")
        for k, buf in self.noise.items():
            buf.copy_(torch.as_tensor(noise[k]).reshape(buf.shape), non_blocking=True)

    def attach_replay(self, store) -> None:
        """Sample minibatches on device from ``store`` (common/replay.py) inside the step itself."""
        self.replay = store
        self.graph = None
        self._replay_epoch = getattr(store, "sample_epoch", 0)

    def _replay_mode_changed(self) -> None:
        """The store switched between uniform and weighted sampling (``ReplayStore.set_sample_prob``): what was captured
        holds the old mode's arguments, so it is dropped and captured again by the step that is about to run."""
        self.graph = None

    def _sync_replay(self) -> None:
        epoch = getattr(self.replay, "sample_epoch", 0)
        if epoch != self._replay_epoch:
            self._replay_mode_changed()
            self._replay_epoch = epoch

    def step_replay(self, use_graph: bool = True) -> None:
        """One train step on a minibatch drawn on device from the attached replay store."""
        check_plans_current(self)
        assert self.replay is not None
        self._sync_replay()
        self._run(use_graph)

    def step(self, *batch, noise=None, use_graph: bool = True) -> None:
        """One train step on the caller's minibatch (``load_batch``).  ``noise``: the step's draws, injected (the step
        then runs eagerly); otherwise they are drawn on device."""
        check_plans_current(self)
        if self.replay is not None:
            raise RuntimeError("a replay store is attached: call step_replay() (or attach_replay(None))")
        self.load_batch(*batch)
        if noise is not None:
            self.load_noise(noise)
            self.body(False)
            return
        self._run(use_graph)

    # ---- optimizer steps ----------------------------------------------------------------------------------------------
    def _update(self, name: str, tau: float = 0.0, extra=None) -> None:
        """(data parallel: all-reduce of the flat gradient -- with ``extra``: that and the tensors of ``extra`` in ONE
        collective -- then) the fused Adam + Polyak + repack of one group."""
        grp = self.model.groups[name]
        if self.dist is not None:
            if extra is None:
                self.dist.allreduce_group(grp)
            else:
                self.dist.all_reduce_many_([self.dist.reduce_local(grp), *extra])
        grp.adam_step(self.model._lrs[name], self.st.ptr, tau=tau)

    def _optim(self, name: str, plan: DwPlan, tau: float = 0.0, extra=None) -> None:
        plan.launch()
        self._update(name, tau, extra)

    def _update_critics_dp(self) -> None:
        """Data parallel: both critic groups' gradients in ONE collective (neither update reads the other's result)."""
        m, dp, st = self.model, self.dist, self.st
        gc, gcc = m.groups["critic"], m.groups["cost_critic"]
        dp.all_reduce_many_([dp.reduce_local(gc), dp.reduce_local(gcc)])
        gc.adam_step(m._lrs["critic"], st.ptr, tau=m.tau)
        gcc.adam_step(m._lrs["cost_critic"], st.ptr, tau=m.tau)


class PipelinedReplay:
    """``steps_replay`` of CPQ and BCQ-Lag: several steps per hipGraph (engine/pipeline.py)."""
    _pipe = None

    def attach_replay(self, store) -> None:
        super().attach_replay(store)
        # Another store: the pipelined graphs go, the twin engine and the two linked step states stay.  (A new twin would
        # be linked from this engine's state alone: when the last pipelined step ran on the old twin, its step count and
        # its uncommitted statistics were lost and the next step repeated a step number.)
        if self._pipe is not None and store is not None:
            self._pipe.reattach(store)
        else:
            self._pipe = None

    def steps_replay(self, n: int, steps_per_graph: Optional[int] = None) -> None:
        """EXACTLY ``n`` train steps on minibatches drawn on device from the attached replay store.  Where the plan says so
        (``plan.steps_per_graph`` > 1, single GPU) whole multiples go through graphs of that many steps, software-pipelined
        across steps (engine/pipeline.py: bit-equal to ``n`` calls of ``step_replay()``); the remainder through the
        one-step graph.  The loop of examples/train/train_cpq.py:138-144 / train_bcql.py:142-148 with the DataLoader
        folded into the step."""
        spg = int(self.plan.steps_per_graph if steps_per_graph is None else steps_per_graph)
        if spg <= 1 or self.dist is not None:
            for _ in range(int(n)):
                self.step_replay(True)
            return
        pipe = self._pipe
        if pipe is None or pipe.n != spg:
            from .pipeline import PipelinedSteps
            pipe = self._pipe = PipelinedSteps(self, spg)
        pipe.run(n)


class VaePhase:
    """``vae_loss`` (cpq.py:125-135, bcql.py:122-132, bearl.py:142-153) of CPQ, BCQ-Lag and BEAR-Lag: its buffers and its
    launches up to the VAE group's optimizer step, which each engine's ``body`` places itself.

    Reads from the engine: ``model``, ``B``, ``rows_global``, ``st``, ``obs``, ``act``, ``noise["eps_vae"]``, ``d_enc``,
    ``d_dec``; ``_vae_all_cu`` also ``seeds`` and ``plan.vae_ns``.  Order in ``__init__``: the batch / noise buffers and
    the descriptors, then ``_vae_runs`` (the dW plan and the seeds read ``r_enc`` / ``r_dec``), then the engine's
    ``seeds``, then ``_vae_all_cu``."""
    vae_ns = None  # glue.VaeNs: the phase as all-CU layer launches, where the plan says so (_vae_all_cu)

    def _vae_runs(self, dev) -> None:
        m, B = self.model, self.B
        od, ad, Lz = m.state_dim, m.action_dim, m.latent_dim
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)  # noqa: E731
        self.r_enc, self.r_dec = MlpRun(self.d_enc, B, True, dev), MlpRun(self.d_dec, B, True, dev)
        self.z, self.du, self.dhead_enc = z(B, Lz), z(1, B, ad), z(1, B, 2 * Lz)
        self.r_dec.setup_backward(self.du, dx_cols=(od, Lz))
        self.r_enc.setup_backward(self.dhead_enc)

    def _vae_seed(self, dev):
        """The loss seed of the decoder's backward launch (glue.seed_vae): that launch computes the gradient it starts
        from and the logged loss."""
        m, B = self.model, self.B
        return G.seed_vae(self.act, self.r_enc.y[0], B, m.action_dim, m.latent_dim, m.beta, self.rows_global,
                          G.SeedStat(dev, 1, B), self.st.stat_ptr("loss/loss_vae"))

    def _vae_all_cu(self) -> None:
        """The phase's forward / backward as all-CU layer launches (csrc/vae_ns.hip, glue.VaeNs) where the plan says so
        (engine/plan.py vae_ns_auto: by measurement) and the library takes the shape; never without the loss seeds."""
        m = self.model
        if self.seeds is not None and self.plan.vae_ns:
            self.vae_ns = G.VaeNs.build(self.r_enc, self.r_dec, self.obs, self.act, self.noise["eps_vae"], self.z,
                                        m.latent_dim, m.beta, self.rows_global, self.st.stat_ptr("loss/loss_vae"))

    def _vae_phase(self, sd, ws=None) -> torch.Tensor:
        """Encode, decode, loss, backward of both nets.  ``sd``: the engine's loss seeds or None; ``ws``: the grid form of
        the unseeded loss launch (glue.loss_ws).  Returns the encoder head [B, 2 Lz]."""
        m, B, eps = self.model, self.B, self.noise["eps_vae"]
        Lz, rg = m.latent_dim, self.rows_global
        if self.vae_ns is not None:  # five all-CU layer launches instead of the four fused ones (same buffers)
            self.vae_ns.forward()
            self.vae_ns.backward()
            return self.r_enc.y[0]
        head = G.vae_encode(self.r_enc, self.obs, self.act, eps, Lz, self.z)
        u = self.r_dec.forward(self.obs, self.z)[0]
        if sd is not None:  # reconstruction gradient + the logged loss by the decoder's backward launch itself
            self.r_dec.backward_dz(tail=G.vae_latent_bwd_tail(head, eps, Lz, m.beta, rg, self.dhead_enc), seed=sd["vae"])
        else:
            G.vae_loss(u, self.act, head, B, m.action_dim, Lz, m.beta, rg, self.du, self.st.stat_ptr("loss/loss_vae"),
                       ws=ws)
            G.vae_decoder_backward(self.r_dec, head, eps, Lz, m.beta, rg, self.dhead_enc)
        self.r_enc.backward_dz()
        return head
