"""Dataset ingestion on device: the reference's pre-training host passes over a DSRL dataset --
``process_sequence_dataset`` (osrl/common/dataset.py:137-183), ``compute_cost_sample_prob`` (:439-459),
``compute_sample_prob`` (:399-436), ``process_bc_dataset`` (:30-134) -- run as HIP kernels (csrc/ingest.hip,
csrc/augment.hip) on arrays uploaded once, and hand their results straight to the on-device samplers
(``SequenceStore`` / ``ReplayStore``) without a trip back to the host.

Same function names and argument meaning as the reference; inputs are the DSRL dict of numpy arrays (or device
tensors), outputs are device tensors.  There is no CPU path: a missing HIP library raises.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple, Union

import numpy as np
import torch

from .. import _lib as L
from ..engine.core import cur_stream, require_cuda

BC_MODES = {"all": 0, "multi-task": 0, "safe": 1, "risky": 2, "boundary": 3}  # include/osrl_amd.h OSRL_BC_*
COST_AFFINE, COST_RECIPROCAL = 0, 1


def _dev(x, device, dtype=torch.float32) -> torch.Tensor:
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=device, dtype=dtype).contiguous()


class Episodes:
    """Episode boundaries of a flat dataset, in HBM: ``start`` int64[n_ep], ``length`` int32[n_ep]."""

    def __init__(self, dataset: Dict[str, "np.ndarray | torch.Tensor"], device):
        self.device = require_cuda(device)
        lib = L.load()
        self.terminals, self.timeouts = _dev(dataset["terminals"], self.device), _dev(dataset["timeouts"], self.device)
        n = self.n = int(self.terminals.shape[0])
        self.ws = torch.zeros(int(lib.osrl_ingest_ws_elems(n)), dtype=torch.int32, device=self.device)
        end = torch.zeros(n, dtype=torch.int64, device=self.device)
        start = torch.zeros(n, dtype=torch.int64, device=self.device)
        length = torch.zeros(n, dtype=torch.int32, device=self.device)
        cnt = torch.zeros(1, dtype=torch.int32, device=self.device)
        L.check(lib.osrl_episode_segments(self.terminals.data_ptr(), self.timeouts.data_ptr(), n, end.data_ptr(),
                                          start.data_ptr(), length.data_ptr(), cnt.data_ptr(), self.ws.data_ptr(),
                                          cur_stream()), "osrl_episode_segments")
        self.n_episodes = int(cnt.item())  # the one host sync of ingestion: sizes the per-episode tables
        self.start, self.length = start[:self.n_episodes].clone(), length[:self.n_episodes].clone()
        # transitions covered by complete episodes (the tail after the last done flag is dropped / left at zero)
        self.n_covered = int((self.start[-1] + self.length[-1]).item()) if self.n_episodes else 0

    def returns(self, x: torch.Tensor, gamma: float, reverse: bool = False, broadcast_first: bool = False,
                x_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``discounted_cumsum`` (dataset.py:19-27) of ``x`` inside every episode (zeros outside)."""
        out = torch.zeros_like(x)
        L.check(L.load().osrl_episode_returns(x.data_ptr(), self.start.data_ptr(), self.length.data_ptr(),
                                              self.n_episodes, float(gamma), int(reverse), int(broadcast_first),
                                              out.data_ptr(), None if x_out is None else x_out.data_ptr(),
                                              cur_stream()), "osrl_episode_returns")
        return out


def process_sequence_dataset(dataset: Dict[str, "np.ndarray | torch.Tensor"], cost_reverse: bool = False,
                             device="cuda") -> Dict[str, torch.Tensor]:
    """dataset.py:137-183 on device.  Instead of a python list of per-episode dicts the result is the flat form the
    window sampler reads: ``observations [n,od]``, ``actions [n,ad]``, ``rewards``, ``costs`` (1 - c under
    ``cost_reverse``), ``returns`` / ``cost_returns`` (to-go sums, gamma = 1) over the n transitions covered by
    complete episodes, plus ``traj_start`` int64[n_traj] and ``traj_len`` int32[n_traj]."""
    ep = Episodes(dataset, device)
    n = ep.n_covered
    f = lambda k: _dev(dataset[k], ep.device)  # noqa: E731
    rew, cost_in = f("rewards"), f("costs")
    costs = torch.zeros_like(cost_in)
    cret = ep.returns(cost_in, 1.0, reverse=cost_reverse, x_out=costs)
    ret = ep.returns(rew, 1.0)
    obs, act = f("observations"), f("actions")
    return dict(observations=obs[:n], actions=act[:n], rewards=rew[:n], costs=costs[:n], returns=ret[:n],
                cost_returns=cret[:n], traj_start=ep.start, traj_len=ep.length)


CostTransform = Union[Tuple[str, float, float], Tuple[str, float], Callable]


def sample_prob_from_weights(weights, with_cdf: bool = False, device=None):
    """Any per-trajectory weights (numpy or tensor, host or device) -> fp32 ``prob = max(w, 0) / sum`` (and the
    inclusive cdf the window sampler reads), normalised on device in fp64 in a fixed order of additions."""
    dev = weights.device if torch.is_tensor(weights) and weights.is_cuda else require_cuda(device or "cuda")
    w = _dev(weights, dev, torch.float64).reshape(-1)
    n = int(w.shape[0])
    if not 1 <= n <= 1 << 20:
        raise ValueError(f"1 .. 2^20 trajectory weights, got {n}")
    prob = torch.zeros(n, dtype=torch.float32, device=dev)
    cdf = torch.zeros(n, dtype=torch.float32, device=dev)
    L.check(L.load().osrl_weights_sample_prob(w.data_ptr(), n, prob.data_ptr(), cdf.data_ptr(), cur_stream()),
            "osrl_weights_sample_prob")
    return (prob, cdf) if with_cdf else prob


def compute_cost_sample_prob(tables: Dict[str, torch.Tensor], cost_transform: CostTransform = ("affine", -1.0, 50.0),
                             with_cdf: bool = False):
    """dataset.py:439-459 on device.  ``cost_transform`` names the two forms the reference's scripts use:
    ``("affine", a, b)`` = ``a*x + b`` (the default ``50 - x``; train_cdt.py:139 ``70 - x``) or
    ``("reciprocal", b)`` = ``1 / (x + b)`` (train_cdt.py:139); those stay on device end to end.  A python callable
    (the reference's own argument) is applied on the host to the ``n_traj`` first cost returns, one fp32 scalar at a
    time as the reference applies it, negatives set to 0, and the weights are normalised on device.  Returns prob
    (and the cdf the sampler reads)."""
    n_traj = int(tables["traj_start"].shape[0])
    dev = tables["cost_returns"].device
    if callable(cost_transform):
        c0 = tables["cost_returns"][tables["traj_start"]].cpu().numpy()  # one small copy: [n_traj] fp32
        w = np.array([cost_transform(x) for x in c0])
        return sample_prob_from_weights(np.where(w < 0, 0, w), with_cdf, dev)
    kind, a, b = (COST_AFFINE, float(cost_transform[1]), float(cost_transform[2])) if cost_transform[0] == "affine" \
        else (COST_RECIPROCAL, 0.0, float(cost_transform[1]))
    if cost_transform[0] not in ("affine", "reciprocal"):
        raise ValueError(cost_transform)
    prob = torch.zeros(n_traj, dtype=torch.float32, device=dev)
    cdf = torch.zeros(n_traj, dtype=torch.float32, device=dev)
    L.check(L.load().osrl_cost_sample_prob(tables["cost_returns"].data_ptr(), tables["traj_start"].data_ptr(), n_traj,
                                           kind, a, b, prob.data_ptr(), cdf.data_ptr(), cur_stream()),
            "osrl_cost_sample_prob")
    return (prob, cdf) if with_cdf else prob


def compute_start_index_sample_prob(tables: Dict[str, torch.Tensor], prob: float = 0.4, with_cdf: bool = False):
    """dataset.py:472-494 on device: the per-trajectory start-index distribution of
    ``SequenceDataset(start_sampling=True)`` as ONE flat fp32 table [total rows] laid out like the trajectory tables
    (the reference returns a python list of per-trajectory fp64 arrays); ``with_cdf`` also returns the inclusive
    running sums inside each trajectory, which is what the window sampler reads."""
    costs = tables["costs"].contiguous()
    n_traj = int(tables["traj_start"].shape[0])
    p = torch.zeros_like(costs)
    cdf = torch.zeros_like(costs)
    L.check(L.load().osrl_start_index_prob(costs.data_ptr(), tables["traj_start"].data_ptr(),
                                           tables["traj_len"].data_ptr(), n_traj, float(prob), p.data_ptr(),
                                           cdf.data_ptr(), cur_stream()), "osrl_start_index_prob")
    return (p, cdf) if with_cdf else p


def process_bc_dataset(dataset: Dict[str, "np.ndarray | torch.Tensor"], cost_limit: float, gamma: float, bc_mode: str,
                       device="cuda") -> Dict[str, torch.Tensor]:
    """dataset.py:30-134 on device: per-episode discounted returns broadcast to every transition, the mode's
    selection as a stable compaction, every array filtered, the cost return appended to the observation for
    "multi-task".  "frontier" fits the Pareto frontier of the episode returns (csrc/augment.hip) and keeps the
    transitions within (rmax - rmin) / 5 of it; it needs every transition inside a complete episode and raises
    NotImplementedError for a trailing partial episode.  Returns NEW device tensors keyed like the input (plus
    ``cost_returns`` / ``rew_returns``); the reference edits its dict in place."""
    if bc_mode not in BC_MODES and bc_mode != "frontier":
        raise NotImplementedError(bc_mode)
    ep = Episodes(dataset, device)
    dev, n = ep.device, ep.n
    d = {k: _dev(v, dev) for k, v in dataset.items()}
    d["terminals"], d["timeouts"] = ep.terminals, ep.timeouts
    d["cost_returns"] = ep.returns(d["costs"], gamma, broadcast_first=True)
    d["rew_returns"] = ep.returns(d["rewards"], gamma, broadcast_first=True)
    f32 = lambda x: float(np.float32(x))  # noqa: E731  numpy compares the fp32 returns with fp32-rounded thresholds
    t0, t1 = {"safe": (f32(cost_limit), 0.0), "risky": (f32(2 * cost_limit), 0.0),
              "boundary": (f32(0.5 * cost_limit), f32(1.5 * cost_limit))}.get(bc_mode, (0.0, 0.0))
    idx = torch.zeros(n, dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = L.load()
    if bc_mode == "frontier":
        _bc_frontier_select(ep, d["cost_returns"], d["rew_returns"], idx, cnt)
    else:
        L.check(lib.osrl_bc_select(d["cost_returns"].data_ptr(), n, BC_MODES[bc_mode], t0, t1, idx.data_ptr(),
                                   cnt.data_ptr(), ep.ws.data_ptr(), cur_stream()), "osrl_bc_select")
    keep = int(cnt.item())
    out: Dict[str, torch.Tensor] = {}
    for k, v in d.items():
        w = int(v[0].numel()) if v.dim() > 1 else 1
        extra = d["cost_returns"] if (bc_mode == "multi-task" and k == "observations") else None
        cols = w + (1 if extra is not None else 0)
        dst = torch.zeros((keep, cols) if (v.dim() > 1 or extra is not None) else (keep,), dtype=torch.float32, device=dev)
        L.check(lib.osrl_gather_rows(v.data_ptr(), w, idx.data_ptr(), keep, dst.data_ptr(), cols,
                                     None if extra is None else extra.data_ptr(), cur_stream()), "osrl_gather_rows")
        out[k] = dst
    out["index"] = idx[:keep].clone()
    return out


# --------------------------------------------------------------------------------------------------------------- #
# Pareto-frontier augmentation (dataset.py:186-396, :557-630; csrc/augment.hip)
# --------------------------------------------------------------------------------------------------------------- #
FILTER_BINS = (10, 50)      # augmentation()'s grid_filter: cost x reward bins (dataset.py:320)
FILTER_PER_BIN = (10, 2)    # at most 10 per bin, bins with 2 or fewer dropped (dataset.py:321)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _injected(draws: Optional[dict], name: str, dev, dtype=torch.float64) -> Optional[torch.Tensor]:
    """One array of injected draws (``draws[name]``, numpy or device) as a device tensor, or None (Philox)."""
    if not draws or draws.get(name) is None:
        return None
    return _dev(draws[name], dev, dtype).reshape(-1)


class Frontier:
    """A Pareto frontier fitted on device: ``coef`` float64[deg+1] (highest power first, as np.polyfit),
    ``pareto_idx`` int32 indices of the Pareto set, ``stats`` = (r2 deg 0..2, max y, min y).  ``poly`` reads the
    coefficients back (one small copy) as the ``np.poly1d`` the reference keeps."""

    def __init__(self, coef, deg, pareto_idx, pcount, stats):
        self.coef_dev, self.deg_dev, self._pidx, self._pcount, self.stats = coef, deg, pareto_idx, pcount, stats

    @property
    def deg(self) -> int:
        return int(self.deg_dev.item())

    @property
    def pareto_idx(self) -> torch.Tensor:
        return self._pidx[:int(self._pcount.item())]

    @property
    def poly(self) -> np.poly1d:
        return np.poly1d(self.coef_dev[:self.deg + 1].cpu().numpy())


def _fit_frontier(c: torch.Tensor, r: torch.Tensor, deg: int, pick: bool = False) -> Frontier:
    """Pareto set of (-c, r) then np.polyfit on it, all on device (fp64 inputs of length n)."""
    lib, dev, n = L.load(), c.device, int(c.shape[0])
    flag = torch.zeros(n, dtype=torch.int32, device=dev)
    L.check(lib.osrl_pareto_mask(c.data_ptr(), r.data_ptr(), n, flag.data_ptr(), cur_stream()), "osrl_pareto_mask")
    coef = torch.zeros(8, dtype=torch.float64, device=dev)
    dego = torch.zeros(1, dtype=torch.int32, device=dev)
    pidx = torch.zeros(n, dtype=torch.int32, device=dev)
    pcnt = torch.zeros(1, dtype=torch.int32, device=dev)
    stats = torch.zeros(5, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.osrl_polyfit_ws_elems(n, 2 if pick else int(deg))), dtype=torch.float64, device=dev)
    L.check(lib.osrl_polyfit(c.data_ptr(), r.data_ptr(), flag.data_ptr(), n, int(deg), int(pick), coef.data_ptr(),
                             dego.data_ptr(), pidx.data_ptr(), pcnt.data_ptr(), stats.data_ptr(), ws.data_ptr(),
                             cur_stream()), "osrl_polyfit")
    return Frontier(coef, dego, pidx, pcnt, stats)


def pareto_frontier(cost, rew, deg: int = 3, device="cuda") -> Frontier:
    """``np.poly1d(np.polyfit(cost[P], rew[P], deg))`` over the Pareto set P of (-cost, rew) (oapackage's
    ParetoDoubleLong in the reference, dataset.py:329-340), on device in fp64."""
    if not 0 <= int(deg) <= 7:
        raise ValueError(f"deg must be in 0..7, got {deg}")
    dev = cost.device if torch.is_tensor(cost) else require_cuda(device)
    c, r = _dev(cost, dev, torch.float64).reshape(-1), _dev(rew, dev, torch.float64).reshape(-1)
    if c.shape != r.shape or c.numel() < 1:
        raise ValueError("cost and rew must be non-empty and of one length")
    return _fit_frontier(c, r, int(deg))


def compute_sample_prob(tables: Dict[str, torch.Tensor], frontier: Frontier, beta: float = 1.0, with_cdf: bool = False,
                        with_dist: bool = False):
    """``compute_sample_prob`` (dataset.py:399-436, what ``SequenceDataset(pf_sample=True)`` samples trajectories
    by) on device: ``prob_i ~ 1 / (dist_i + beta)``, ``dist_i`` the distance of trajectory i's (cost return, return) to
    ``frontier`` (an ``ingest.Frontier``).  The reference gets the distance from one scipy BFGS solve per trajectory
    started at the cost return; that solve does not find the nearest point of the curve but the stationary point
    downhill from its start, and that is the definition here (csrc/pf_dist.h): the first root, with a sign change,
    of ``(x - c) + (p(x) - r) p'(x)`` on the downhill side of ``c``, clamped at 0.  Where the reference's line
    search jumps into another basin or stops early its result depends on the solver's path and differs.
    Returns prob fp32 [n_traj]; ``with_cdf`` adds the inclusive cdf the window sampler reads, ``with_dist`` the fp64
    distances (in that order)."""
    if not float(beta) > 0.0:
        raise ValueError(f"beta must be > 0, got {beta}")
    n_traj = int(tables["traj_start"].shape[0])
    if not 1 <= n_traj <= 1 << 20:
        raise ValueError(f"1 .. 2^20 trajectories, got {n_traj}")
    dev = tables["cost_returns"].device
    prob = torch.zeros(n_traj, dtype=torch.float32, device=dev)
    cdf = torch.zeros(n_traj, dtype=torch.float32, device=dev)
    dist = torch.zeros(n_traj, dtype=torch.float64, device=dev)
    ws = torch.empty(n_traj, dtype=torch.float64, device=dev)
    L.check(L.load().osrl_pf_sample_prob(tables["returns"].data_ptr(), tables["cost_returns"].data_ptr(),
                                         tables["traj_start"].data_ptr(), n_traj, frontier.coef_dev.data_ptr(),
                                         frontier.deg_dev.data_ptr(), float(beta), prob.data_ptr(), cdf.data_ptr(),
                                         dist.data_ptr(), ws.data_ptr(), cur_stream()), "osrl_pf_sample_prob")
    out = (prob,) + ((cdf,) if with_cdf else ()) + ((dist,) if with_dist else ())
    return out if len(out) > 1 else prob


def _bc_frontier_select(ep: "Episodes", cost_returns: torch.Tensor, rew_returns: torch.Tensor, idx, cnt) -> None:
    """process_bc_dataset "frontier" (dataset.py:73-93): Pareto set of the episode returns, polyfit deg 0, 1, 2 until
    r^2 >= 0.9, keep the transitions within (rmax - rmin) / 5 of the frontier."""
    if ep.n_episodes < 1:
        raise ValueError('bc_mode="frontier" needs at least one complete episode')
    if ep.n_covered != ep.n:
        # the reference leaves zero returns on these transitions and keeps or drops them by comparing 0 with the
        # frontier at cost 0 -- an artefact of its loop, not a selection; cut the dataset at its last done flag
        raise NotImplementedError(f'bc_mode="frontier" on a dataset whose last {ep.n - ep.n_covered} transitions '
                                  "belong to no complete episode (no done flag after them)")
    lib, dev = L.load(), ep.device
    c0 = torch.empty(ep.n_episodes, dtype=torch.float64, device=dev)
    r0 = torch.empty_like(c0)
    L.check(lib.osrl_traj_returns(rew_returns.data_ptr(), cost_returns.data_ptr(), ep.start.data_ptr(), ep.n_episodes,
                                  r0.data_ptr(), c0.data_ptr(), cur_stream()), "osrl_traj_returns")
    fr = _fit_frontier(c0, r0, 2, pick=True)
    mask = torch.empty(ep.n, dtype=torch.float32, device=dev)
    L.check(lib.osrl_bc_frontier_select(cost_returns.data_ptr(), rew_returns.data_ptr(), ep.n, fr.coef_dev.data_ptr(),
                                        fr.deg_dev.data_ptr(), fr.stats.data_ptr(), mask.data_ptr(), idx.data_ptr(),
                                        cnt.data_ptr(), ep.ws.data_ptr(), cur_stream()), "osrl_bc_frontier_select")


SEQ_KEYS = ("observations", "actions", "rewards", "costs", "returns", "cost_returns")


def _traj_returns(tables):
    lib, dev = L.load(), tables["returns"].device
    n = int(tables["traj_start"].shape[0])
    r0 = torch.empty(n, dtype=torch.float64, device=dev)
    c0 = torch.empty_like(r0)
    L.check(lib.osrl_traj_returns(tables["returns"].data_ptr(), tables["cost_returns"].data_ptr(),
                                  tables["traj_start"].data_ptr(), n, r0.data_ptr(), c0.data_ptr(), cur_stream()),
            "osrl_traj_returns")
    return r0, c0


def _combine(tables, nearest, map_, S: int, tc, tr, noise: bool = False, cstd: float = 0.0, rstd: float = 0.0,
             draws: Optional[dict] = None, seed: int = 0):
    """The original trajectories followed by one relabelled copy per sample (osrl_augment_layout / _gather)."""
    lib, dev = L.load(), tables["returns"].device
    n_traj = int(tables["traj_start"].shape[0])
    n_rows = int(tables["returns"].shape[0])
    new_start = torch.empty(n_traj + S, dtype=torch.int64, device=dev)
    new_len = torch.empty(n_traj + S, dtype=torch.int32, device=dev)
    src = torch.empty(max(S, 1), dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    L.check(lib.osrl_augment_layout(_ptr(nearest), _ptr(map_), S, tables["traj_start"].data_ptr(),
                                    tables["traj_len"].data_ptr(), n_traj, n_rows, new_start.data_ptr(),
                                    new_len.data_ptr(), src.data_ptr(), total.data_ptr(), cur_stream()),
            "osrl_augment_layout")
    rows = int(total.item())  # host read: sizes the combined tables
    out = {}
    for k in SEQ_KEYS:
        v = tables[k]
        t = torch.empty((rows,) + tuple(v.shape[1:]), dtype=torch.float32, device=dev)
        t[:n_rows].copy_(v)
        out[k] = t
    nc = _injected(draws, "noise_c", dev) if noise else None
    nr = _injected(draws, "noise_r", dev) if noise else None
    if (nc is None) != (nr is None):
        raise ValueError("inject both noise_c and noise_r, or neither")
    if nc is not None and (nc.numel() < rows - n_rows or nr.numel() < rows - n_rows):
        raise ValueError(f"injected noise rows: {rows - n_rows} needed")
    obs, act = tables["observations"], tables["actions"]
    od, ad = int(obs[0].numel()), int(act[0].numel())
    L.check(lib.osrl_augment_gather(obs.data_ptr(), act.data_ptr(), tables["rewards"].data_ptr(),
                                    tables["costs"].data_ptr(), tables["returns"].data_ptr(),
                                    tables["cost_returns"].data_ptr(), od, ad, tables["traj_start"].data_ptr(),
                                    src.data_ptr(), S, new_start.data_ptr(), new_len.data_ptr(), n_traj, _ptr(tc),
                                    _ptr(tr), int(noise), float(cstd), float(rstd), _ptr(nc), _ptr(nr),
                                    int(seed) & 0xFFFFFFFFFFFFFFFF, out["observations"].data_ptr(),
                                    out["actions"].data_ptr(), out["rewards"].data_ptr(), out["costs"].data_ptr(),
                                    out["returns"].data_ptr(), out["cost_returns"].data_ptr(), cur_stream()),
            "osrl_augment_gather")
    out["traj_start"], out["traj_len"] = new_start, new_len
    return out


def augmentation(tables: Dict[str, torch.Tensor], deg: int = 3, max_rew_decrease: float = 1.0, beta: float = 1.0,
                 augment_percent: float = 0.3, max_reward: float = 1000.0, min_reward: float = 0.0, seed: int = 0,
                 draws: Optional[dict] = None):
    """``augmentation()`` (dataset.py:282-396) on the flat tables of ``process_sequence_dataset``: grid filter of the
    trajectory returns, Pareto frontier polyfit, ``int(augment_percent * filtered)`` targets above the frontier, each
    relabelling a copy of its nearest trajectory (or a drawn partner).  Returns ``(combined tables, info)``: the
    tables hold the originals followed by the copies; ``info`` holds ``idx`` (the reference's nearest_idx, indices
    into the filtered set), ``indices`` (filtered -> original trajectory), ``frontier`` (a ``Frontier``),
    ``targets`` (cost, reward fp64) and the trajectory counts.  ``draws`` injects the random stream (see
    include/osrl_amd.h): ``pick``, ``u_rew``, ``u_part``; otherwise Philox keyed by ``seed``."""
    if not 0 <= int(deg) <= 7:
        raise ValueError(f"deg must be in 0..7, got {deg}")
    lib, dev = L.load(), tables["returns"].device
    n_traj = int(tables["traj_start"].shape[0])
    if n_traj < 1:
        raise ValueError("augmentation needs at least one trajectory")
    r0, c0 = _traj_returns(tables)
    filt = torch.empty(n_traj, dtype=torch.int32, device=dev)
    fx = torch.empty(n_traj, dtype=torch.float64, device=dev)
    fy = torch.empty_like(fx)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.osrl_grid_filter_ws_elems(n_traj)), dtype=torch.float64, device=dev)
    pick = _injected(draws, "pick", dev, torch.int32)
    L.check(lib.osrl_grid_filter(c0.data_ptr(), r0.data_ptr(), n_traj, FILTER_BINS[0], FILTER_BINS[1],
                                 FILTER_PER_BIN[0], FILTER_PER_BIN[1], _ptr(pick), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                 filt.data_ptr(), fx.data_ptr(), fy.data_ptr(), cnt.data_ptr(), ws.data_ptr(),
                                 cur_stream()), "osrl_grid_filter")
    F = int(cnt.item())  # host read: the filtered count sizes everything after it
    if F < 0:
        raise ValueError("augmentation: every trajectory has the same cost return or the same return "
                         "(the grid filter's bin width is 0)")
    if F == 0:
        raise ValueError("augmentation: the grid filter kept no trajectory (every bin holds 2 or fewer)")
    fx, fy, filt = fx[:F], fy[:F], filt[:F]
    fr = _fit_frontier(fx, fy, int(deg))
    S = int(augment_percent * F)
    tc = torch.empty(max(S, 1), dtype=torch.float64, device=dev)
    tr = torch.empty_like(tc)
    nearest = torch.empty(max(S, 1), dtype=torch.int32, device=dev)
    if S > 0:
        u_rew, u_part = _injected(draws, "u_rew", dev), _injected(draws, "u_part", dev)
        if u_rew is not None and u_rew.numel() < S:
            raise ValueError(f"injected u_rew: {S} draws needed")
        ws2 = torch.empty(int(lib.osrl_augment_targets_ws_elems(F, S)), dtype=torch.float64, device=dev)
        L.check(lib.osrl_augment_targets(fr.coef_dev.data_ptr(), fr.deg_dev.data_ptr(), fx.data_ptr(), fy.data_ptr(), F,
                                         S, float(min_reward), float(max_reward), float(max_rew_decrease), float(beta),
                                         _ptr(u_rew), _ptr(u_part), int(seed) & 0xFFFFFFFFFFFFFFFF, tc.data_ptr(),
                                         tr.data_ptr(), nearest.data_ptr(), ws2.data_ptr(), cur_stream()),
                "osrl_augment_targets")
    out = _combine(tables, nearest if S else None, filt, S, tc, tr, seed=seed)
    info = dict(idx=nearest[:S], indices=filt, frontier=fr, targets=(tc[:S], tr[:S]), n_original=n_traj,
                n_augmented=S)
    return out, info


def random_augmentation(tables: Dict[str, torch.Tensor], augment_percent: float = 0.3, aug_rmin: float = 0,
                        aug_rmax: float = 600, aug_cmin: float = 5, aug_cmax: float = 50, cgap: float = 5,
                        rstd: float = 1, cstd: float = 0.25, seed: int = 0, draws: Optional[dict] = None):
    """``random_augmentation()`` (dataset.py:557-630): ``int(augment_percent * n_traj)`` uniform (cost, reward)
    targets, each relabelling a copy of the nearest trajectory below ``max(c - cgap, min c + 1)``, plus per-row
    Gaussian noise.  Returns ``(combined tables, info)`` like ``augmentation``; ``draws``: ``u_cr``
    ([samples, 2] uniforms), ``noise_c`` / ``noise_r`` (the normal rows, [augmented rows])."""
    lib, dev = L.load(), tables["returns"].device
    n_traj = int(tables["traj_start"].shape[0])
    if n_traj < 1:
        raise ValueError("random_augmentation needs at least one trajectory")
    r0, c0 = _traj_returns(tables)
    S = int(augment_percent * n_traj)
    tc = torch.empty(max(S, 1), dtype=torch.float64, device=dev)
    tr = torch.empty_like(tc)
    nearest = torch.empty(max(S, 1), dtype=torch.int32, device=dev)
    if S > 0:
        u_cr = _injected(draws, "u_cr", dev)
        if u_cr is not None and u_cr.numel() < 2 * S:
            raise ValueError(f"injected u_cr: {2 * S} draws needed")
        L.check(lib.osrl_random_aug_targets(c0.data_ptr(), r0.data_ptr(), n_traj, S, float(aug_cmin), float(aug_cmax),
                                            float(aug_rmin), float(aug_rmax), float(cgap), _ptr(u_cr),
                                            int(seed) & 0xFFFFFFFFFFFFFFFF, tc.data_ptr(), tr.data_ptr(),
                                            nearest.data_ptr(), cur_stream()), "osrl_random_aug_targets")
    out = _combine(tables, nearest if S else None, None, S, tc, tr, noise=True, cstd=cstd, rstd=rstd, draws=draws,
                   seed=seed)
    info = dict(idx=nearest[:S], indices=None, frontier=None, targets=(tc[:S], tr[:S]), n_original=n_traj,
                n_augmented=S)
    return out, info
