"""Data-parallel correctness at world_size 2 on ONE GPU: two replicas run the sharded step in two host threads (own
streams, eager launches) and exchange through an in-process stand-in for the process group that implements the two
primitives the engines use (all-reduce SUM, all-gather) with exactly torch.distributed's semantics.  Oracle
(SURVEY.md 8e): the sharded step on 2 x B rows == the single-device step on the concatenated 2B-row batch.

This covers what the 1-rank NCCL tests cannot (there every collective is an identity): the 1/B_global normalisations,
the batch-global statistics (CPQ's quantile and OOD mean, the PID / dual-variable means of BCQ-L and BEAR-L) and the
logged statistics' shares."""
import threading

import numpy as np
import pytest
import torch

from cases import Case, make_batch, make_noise
from gpu_util import build_gpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Shared:
    def __init__(self, world):
        self.world, self.slots, self.barrier = world, [None] * world, threading.Barrier(world)
        self.errors = []


def make_sim(shared, rank):
    from osrl_amd.engine.dist import DataParallel

    class SimDist(DataParallel):
        def __init__(self):  # no process group: the exchange happens through `shared`
            self.group, self.world, self.rank, self._gather_buf, self.src0 = None, shared.world, rank, None, 0

        def broadcast_(self, t):
            t.copy_(self._exchange(t)[0])
            return t

        def _exchange(self, t):
            torch.cuda.current_stream().synchronize()
            shared.slots[rank] = t
            shared.barrier.wait()
            parts = [s.clone() for s in shared.slots]
            torch.cuda.current_stream().synchronize()
            shared.barrier.wait()  # everyone holds private copies: the originals may be overwritten now
            return parts

        def all_reduce_(self, t):
            parts = self._exchange(t)
            acc = parts[0]
            for p in parts[1:]:
                acc = acc + p
            t.copy_(acc)
            return t

        def all_gather_concat(self, t):
            return torch.cat([p.reshape(-1) for p in self._exchange(t)])

    return SimDist()


def _shard(v, key, r, W, B, N, M=1):
    """Rows of rank r out of a concatenated-batch tensor; noise tensors keep their per-algorithm row order."""
    Bl = B // W
    if key == "eps_ood":  # [N, B, ad]
        return v[:, r * Bl:(r + 1) * Bl].copy()
    if key == "eps_vae_ood":  # [N*B, L], row j*B + b (sample-major, cpq.py:170-176)
        return v.reshape(N, B, -1)[:, r * Bl:(r + 1) * Bl].reshape(N * Bl, -1).copy()
    if key in ("z_c", "z_cc", "eps_c", "eps_cc"):  # [N*B, .], row b*N + j (repeat_interleave)
        return v.reshape(B, N, -1)[r * Bl:(r + 1) * Bl].reshape(Bl * N, -1).copy()
    if key == "z_mmd":  # [B, M, L]
        return v[r * Bl:(r + 1) * Bl].copy()
    if key == "eps_pi":  # [B*M, ad], row b*M + j
        return v.reshape(B, M, -1)[r * Bl:(r + 1) * Bl].reshape(Bl * M, -1).copy()
    return v[r * Bl:(r + 1) * Bl].copy()  # per-row tensors


DP_CASES = {
    "cpq": Case("dp_cpq", "cpq", od=5, ad=2, B=32, hidden=[32, 32], vae_hidden=48, N=4, steps=3, episode_len=1000, seed=7),
    # BASELINE.json C4 at its real widths: (17, 6), hidden [256,256], VAE 400, N=10, 2 x 1024 rows -- the world-2
    # equivalence through 256/400-wide tiles, the capped N*B launches and split-K dW with rows_global != rows
    "cpq_c4": Case("dp_cpq_c4", "cpq", od=17, ad=6, B=2048, hidden=[256, 256], vae_hidden=400, N=10, steps=2,
                   episode_len=1000, seed=13),
    # BASELINE.json C4 as the 8-GPU job runs it: global batch 16384 = 8 x 2048 rows, 163840 KL values under the
    # batch-global quantile (the grid select osrl_quantile_ws INSIDE a captured step), 8-way gather
    "cpq_c4_w8": Case("dp_cpq_c4_w8", "cpq", od=17, ad=6, B=16384, hidden=[256, 256], vae_hidden=400, N=10, steps=2,
                      episode_len=1000, seed=14),
    "bcql": Case("dp_bcql", "bcql", od=4, ad=2, B=32, hidden=[24, 24], vae_hidden=32, N=3, num_q=1, num_qc=2, steps=3,
                 episode_len=200, cost_limit=-4.0, max_action=1.5, seed=8),  # PID active
    "bearl": Case("dp_bearl", "bearl", od=4, ad=2, B=32, hidden=[24, 24], vae_hidden=32, N=3, num_q=1, num_qc=2, steps=3,
                  episode_len=200, cost_limit=-4.0, seed=9, hp=dict(M=4, kernel="laplacian", mmd_sigma=1.5, alpha_lr=0.05)),
    "bc": Case("dp_bc", "bc", od=8, ad=2, B=32, hidden=[32, 32], steps=3, seed=10),
    # COptiDICE: the chi loss takes a softmax over the GLOBAL batch (all-gathered ell); with and without the chi net
    "coptidice": Case("dp_dice", "coptidice", od=5, ad=2, B=32, hidden=[24, 24], steps=3, episode_len=200, seed=11,
                      hp=dict(actor_lr=1e-3, critic_lr=1e-3, scalar_lr=1e-2)),
    "coptidice_nochi": Case("dp_dice0", "coptidice", od=5, ad=2, B=32, hidden=[24, 24], num_q=1, num_qc=2, steps=3,
                            episode_len=200, cost_limit=40.0, seed=12,
                            hp=dict(f_type="kl", cost_ub_epsilon=0.0, actor_lr=1e-3, critic_lr=1e-3, scalar_lr=1e-2)),
}


@pytest.mark.parametrize("algo", [k for k in DP_CASES if k != "cpq_c4_w8"])
def test_world2_sharded_step_equals_concatenated_batch(algo):
    c = DP_CASES[algo]
    W, B, N, M = 2, c.B, c.N, int(c.hp.get("M", 1))
    Bl = B // W
    batch = make_batch(c)
    keys = ("observations", "actions") if algo == "bc" else \
        ("observations", "next_observations", "actions", "rewards", "costs", "done") + \
        (("is_init",) if c.algo == "coptidice" else ())
    step = (lambda tr, args, nz: tr.train_one_step(list(args), noise=nz)) if c.algo == "coptidice" else \
        (lambda tr, args, nz: tr.train_one_step(*args) if algo == "bc" else tr.train_one_step(*args, noise=nz))
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=DEV)  # noqa: E731

    # single device, concatenated batch
    m1, tr1, lg1 = build_gpu(c)
    for s in range(c.steps):
        nz = {k: t(v) for k, v in make_noise(c, s).items()}
        step(tr1, [t(batch[k]) for k in keys], nz)
    torch.cuda.synchronize()

    # two replicas, each on its half
    shared = _Shared(W)
    reps = [build_gpu(c) for _ in range(W)]

    def worker(r):
        try:
            m, tr, lg = reps[r]
            with torch.cuda.stream(torch.cuda.Stream()):
                sim = make_sim(shared, r)
                m.engine(Bl, rows_global=B, dist=sim)
                args = [t(batch[k][r * Bl:(r + 1) * Bl]) for k in keys]
                for s in range(c.steps):
                    nz = {k: t(_shard(v, k, r, W, B, N, M)) for k, v in make_noise(c, s).items()}
                    step(tr, args, nz)
                torch.cuda.current_stream().synchronize()
        except BaseException as e:  # noqa: BLE001
            shared.errors.append((r, repr(e)))
            shared.barrier.abort()
            raise

    th = [threading.Thread(target=worker, args=(r,)) for r in range(W)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    assert not shared.errors, shared.errors
    torch.cuda.synchronize()

    sd1 = {k: v.detach().cpu().numpy() for k, v in m1.state_dict().items()}
    big = c.B >= 1024
    for r in range(W):
        m, tr, lg = reps[r]
        for k, v in m.state_dict().items():
            d = np.abs(v.detach().cpu().numpy() - sd1[k])
            if not big:
                assert d.max() <= 2e-5, f"{algo} rank {r} param {k}: sharded vs concatenated differ by {d.max():.3e}"
            else:
                # at real widths Adam moves an element whose gradient is round-off noise around zero by ~lr per step
                # whatever its size, in either direction (tests/test_gpu_train_step.py full-size note): the parameters
                # get the loose bound + a tight median, the GRADIENTS (Adam first moments) are compared below
                assert d.max() <= 2.5 * 1e-3 * c.steps + 1e-6 and np.median(d) <= 2e-6, \
                    f"{algo} rank {r} param {k}: max {d.max():.3e} median {np.median(d):.3e}"
        if big:
            for gname, grp in m.groups.items():
                gate = 5e-3 if gname == "actor" else 5e-5  # the actor gradient is a cancelling batch sum
                for k in grp.layout:
                    if k in grp.aliases:
                        continue
                    a, b = grp._view(grp.m, k).cpu().numpy(), m1.groups[gname]._view(m1.groups[gname].m, k).cpu().numpy()
                    scale = max(np.abs(b).max(), 1e-12)
                    assert np.abs(a - b).max() <= gate * scale, \
                        f"{algo} rank {r} first moment {k}: {np.abs(a - b).max():.3e} vs scale {scale:.3e}"
        for name in ("log_alpha", "pid_state", "scalar_leaves"):
            if hasattr(m, name):
                a, b = getattr(m, name).cpu().numpy(), getattr(m1, name).cpu().numpy()
                assert np.abs(a - b).max() <= 1e-5, (algo, r, name, a, b)
        # logged statistics: the all-reduced values equal the single-device ones on every rank
        for k, vals in lg1.data.items():
            got = [float(x) for x in lg.data[k]]
            want = [float(x) for x in vals]
            assert np.allclose(got, want, rtol=1e-4, atol=1e-5), (algo, r, k, got, want)
    # the replicas stay identical to each other (bit for bit: same reduced gradients, same optimizer)
    for r in range(1, W):
        for k, v in reps[0][0].state_dict().items():
            assert torch.equal(v, reps[r][0].state_dict()[k]), f"{algo}: replicas 0 and {r} diverged in {k}"


@pytest.mark.parametrize("case", ["cdt_small", "cdt_v_norew"])
def test_world2_cdt_sharded_step_equals_concatenated_batch(case):
    """CDT: the count-normalised means ([mask > 0].mean(), accuracy) use GLOBAL counts (the two shards hold different
    numbers of valid tokens), the gradient is clipped by the norm of the REDUCED gradient, the temperature step
    sees the global entropy."""
    from cases import CDT_CASES, make_cdt_batch
    from test_gpu_cdt import build_cdt_gpu
    c = CDT_CASES[case]  # the second one: 3 tokens per timestep, add-cost feature, 2-layer stochastic head
    W, B = 2, c.B
    Bl = B // W
    batch = make_cdt_batch(c)
    batch["mask"][0, 1:] = 0  # more (tail) padding in rank 0's shard: the valid-token counts of the shards differ
    assert len({float(batch["mask"][r * Bl:(r + 1) * Bl].sum()) for r in range(W)}) == W, "shards must differ in valid tokens"
    keys = ("states", "actions", "returns", "costs_return", "time_steps", "mask", "episode_cost", "costs")
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=DEV)  # noqa: E731
    m1, tr1, lg1 = build_cdt_gpu(c)
    for s in range(3):
        tr1.train_one_step(*[t(batch[k]) for k in keys])
    torch.cuda.synchronize()

    shared = _Shared(W)
    reps = [build_cdt_gpu(c) for _ in range(W)]

    def worker(r):
        try:
            m, tr, lg = reps[r]
            with torch.cuda.stream(torch.cuda.Stream()):
                m.engine(Bl, tr.cfg, dist=make_sim(shared, r))
                args = [t(batch[k][r * Bl:(r + 1) * Bl]) for k in keys]
                for s in range(3):
                    tr.train_one_step(*args)
                torch.cuda.current_stream().synchronize()
        except BaseException as e:  # noqa: BLE001
            shared.errors.append((r, repr(e)))
            shared.barrier.abort()
            raise

    th = [threading.Thread(target=worker, args=(r,)) for r in range(W)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    assert not shared.errors, shared.errors
    torch.cuda.synchronize()
    sd1 = m1.state_dict()
    for r in range(W):
        m, tr, lg = reps[r]
        for k, v in m.state_dict().items():
            if v.dtype != torch.bool:
                d = float((v - sd1[k]).abs().max())
                assert d <= 2e-6, f"cdt rank {r} param {k}: {d:.3e}"
        assert abs(float(m.log_temperature) - float(m1.log_temperature)) < 1e-6
        for k, vals in lg1.data.items():
            assert np.allclose([float(x) for x in lg.data[k]], [float(x) for x in vals], rtol=1e-4, atol=1e-5), (r, k)


# --------------------------------------------------------------------------------------------------------------- #
# The CAPTURED data-parallel step with a peer.  Two real RCCL ranks cannot share the one GPU of the test box (RCCL
# refuses: "Duplicate GPU detected : rank 0 and rank 1 both on CUDA device"), so the peer is a second replica in this
# process and the two collectives the engines use are graph-capturable device ops on the capture stream: both
# replicas' step bodies (their forked side branches included) are captured into ONE hipGraph, the bodies interleaved
# at every collective by greenlets (replica r runs up to its next collective, parks; when all are parked the exchange
# is enqueued and every replica continues).  What this covers beyond the threaded eager test above: the data-parallel
# launch plan inside a replayed graph -- two-branch fork/join around collectives, static collective buffers, the
# split update of the two critic groups after the join -- with a peer whose values differ.  (RCCL's own kernels as
# graph nodes are covered by the 1-rank NCCL capture tests; RCCL peer traffic inside a graph needs >1 GPU.)
class _Hub:
    """The in-process process group.  Like RCCL it owns ONE stream on which every exchange runs, in the order the
    replicas issue them: an exchange waits for the issuing stream of every replica (main or a side branch: an event
    recorded where the collective is called), and each replica's issuing stream waits for the exchange -- the
    dependency structure torch's ProcessGroupNCCL puts around a collective.  ``log`` keeps, per exchange, what every
    replica deposited (label, element count): the replicas must issue the SAME sequence (round 5: two of CPQ's four
    collectives are issued from side branches, which is order-safe exactly because of this)."""

    def __init__(self, world):
        self.world, self.slots, self.parent = world, [None] * world, None
        self.xs = None
        self.log = []

    def run(self, fns):
        import greenlet
        self.parent = greenlet.getcurrent()
        if self.xs is None:
            self.xs = torch.cuda.Stream()
        # the replicas share this THREAD, hence torch's thread-local current stream: every replica starts on the caller's
        # stream, puts its own stream back when it resumes (GreenDist._exchange), and the caller gets its stream back at
        # the end -- separate processes have this for free
        base = torch.cuda.current_stream()
        gs = [greenlet.greenlet(f) for f in fns]
        for g in gs:
            torch.cuda.set_stream(base)
            g.switch()  # up to its first collective (or to the end)
        torch.cuda.set_stream(base)
        while not all(g.dead for g in gs):
            assert not any(g.dead for g in gs) and all(s is not None for s in self.slots), \
                "replicas issued different numbers of collectives"
            sig = {(lab, int(t.numel())) for (t, ev, lab) in self.slots}
            assert len(sig) == 1, f"replicas are at different collectives: {sorted(sig)}"
            self.log.append(next(iter(sig)))
            for (t, ev, lab) in self.slots:
                self.xs.wait_event(ev)
            with torch.cuda.stream(self.xs):
                parts = [t.clone() for (t, ev, lab) in self.slots]
                done = torch.cuda.Event()
                done.record(self.xs)
            self.slots = [None] * self.world
            for g in gs:
                g.switch((parts, done))
            torch.cuda.set_stream(base)


def make_green(hub, rank):
    from osrl_amd.engine.dist import DataParallel

    class GreenDist(DataParallel):
        def __init__(self):
            self.group, self.world, self.rank, self._gather_buf, self.src0 = None, hub.world, rank, None, 0
            self._probe = None

        def _exchange(self, t, label):
            mine = torch.cuda.current_stream()
            ev = torch.cuda.Event()
            ev.record(mine)  # on the stream the collective is issued from
            hub.slots[rank] = (t, ev, label)
            parts, done = hub.parent.switch()
            torch.cuda.set_stream(mine)  # (the other replicas ran on this thread meanwhile)
            mine.wait_event(done)
            return parts

        def all_reduce_(self, t):
            parts = self._exchange(t, "all_reduce")
            acc = parts[0]
            for p in parts[1:]:
                acc = acc + p
            t.copy_(acc)
            return t

        def broadcast_(self, t):
            t.copy_(self._exchange(t, "broadcast")[0])
            return t

        def all_agree(self, ok, device):
            return bool(ok)

        def all_gather_concat(self, t):
            return torch.cat([p.reshape(-1) for p in self._exchange(t, "all_gather")])

    return GreenDist()


@pytest.mark.parametrize("algo,W", [("cpq", 2), ("cpq_c4", 2), ("cpq_c4_w8", 8)])
def test_captured_data_parallel_graph_equals_concatenated_batch(algo, W):
    """W replicas' data-parallel step bodies in ONE captured graph == the single-device step on the concatenated batch.
    W = 8 is BASELINE.json's C4 job shape (8 x 2048 rows at (17, 6)): rows_global = 16384, the batch-global quantile
    over 163840 gathered KL values runs as the grid select inside the step; the single-device run's step-1 statistics
    are refereed by the fp64 oracle."""
    from osrl_amd.engine.core import Branches
    c = DP_CASES[algo]
    B, N = c.B, c.N
    Bl = B // W
    batch = make_batch(c)
    keys = ("observations", "next_observations", "actions", "rewards", "costs", "done")
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=DEV)  # noqa: E731
    m1, tr1, lg1 = build_gpu(c)
    for s in range(c.steps):
        tr1.train_one_step(*[t(batch[k]) for k in keys], noise={k: t(v) for k, v in make_noise(c, s).items()})
    torch.cuda.synchronize()
    if W == 8:  # the referee: the pinned oracle in fp64 on the 16384-row batch, first step
        from oracle_util import build_oracle, oracle_step
        ost = oracle_step(build_oracle(c, np.float64), c, 0)
        for k, r in ost.items():
            got = float(lg1.data[k][0])
            assert abs(got - r) <= 1e-4 * max(1.0, abs(r)), f"single device, 16384 rows, step 1, {k}: {got} vs oracle {r}"

    hub = _Hub(W)
    reps = [build_gpu(c) for _ in range(W)]
    engs = [None] * W

    def build(r):
        engs[r] = reps[r][0].engine(Bl, rows_global=B, dist=make_green(hub, r))
    hub.run([lambda r=r: build(r) for r in range(W)])
    pars = [Branches(True, 2) for _ in range(W)]
    bodies = [lambda r=r: engs[r].body(False, pars[r]) for r in range(W)]
    snaps = [e._snapshot() for e in engs]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hub.run(bodies)  # warm-up pass (torch requires one before capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    hub.log = []
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):  # (engine/core.py graph_capture)
        try:
            hub.run(bodies)
        except BaseException:  # (an exception inside a capture otherwise dies in the graph's destructor, unseen)
            import traceback
            traceback.print_exc()
            raise
    torch.cuda.synchronize()
    # ONE total order of the step's collectives, the same on every replica (asserted per exchange in _Hub.run): the VAE
    # gradient first, [critic | cost-critic] + the partial qc_ood mean... as all_reduce calls, the KL gather third,
    # [actor | statistics | qc_ood] last -- all four issued from the main branch
    kinds = [k for k, _ in hub.log]
    assert kinds.count("all_gather") == 1 and kinds[0] == "all_reduce" and kinds[-1] == "all_reduce", kinds
    assert kinds.index("all_gather") > 1, kinds  # behind the VAE's and the critic groups' all-reduces
    for e, sn in zip(engs, snaps):
        e._restore(sn)
    for s in range(c.steps):
        nz = make_noise(c, s)
        for r, e in enumerate(engs):
            e.load_batch(*[t(batch[k][r * Bl:(r + 1) * Bl]) for k in keys])
            e.load_noise({k: t(_shard(v, k, r, W, B, N)) for k, v in nz.items() if k in e.noise})
        graph.replay()
        for e in engs:
            e.st.host_step += 1
        torch.cuda.synchronize()
        for r, e in enumerate(engs):
            got = e.st.read_stats()
            for k, vals in lg1.data.items():
                assert abs(got[k] - float(vals[s])) <= 1e-4 * max(1.0, abs(float(vals[s]))), (algo, r, s, k, got[k], float(vals[s]))
    big = c.B >= 1024
    sd1 = {k: v.detach().cpu().numpy() for k, v in m1.state_dict().items()}
    for r in range(W):
        m = reps[r][0]
        for k, v in m.state_dict().items():
            d = np.abs(v.detach().cpu().numpy() - sd1[k])
            if big:
                assert d.max() <= 2.5 * 1e-3 * c.steps + 1e-6 and np.median(d) <= 2e-6, (algo, r, k, d.max())
            else:
                assert d.max() <= 2e-5, f"{algo} rank {r} param {k}: {d.max():.3e}"
        assert abs(float(m.log_alpha) - float(m1.log_alpha)) <= 1e-5
    for r in range(1, W):
        for k, v in reps[0][0].state_dict().items():
            assert torch.equal(v, reps[r][0].state_dict()[k]), f"{algo}: replicas 0 and {r} diverged in {k}"
