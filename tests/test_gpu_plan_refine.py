"""CEM refinement of the act-time planner on the GPU (csrc/plan_refine.hip ``osrl_plan_refit``, engine/mpc.py
``ModelPlanner(refine_rounds=)``).  The kernel test compares with the fp64 restatement below, bit for bit: the ranking is
integer work under a total order, the sums are fp64 in ascending rank with one rounding per operation and one rounding
to fp32 (``np.cumsum`` adds in order, where ``np.sum`` would add pairwise), and the redraw is one fma of fp32 values."""
import itertools
import zlib

import numpy as np
import pytest
import torch

import plan_cases as P
from test_gpu_plan import DEV, bits, dev, menv, trainer

pytestmark = pytest.mark.gpu

NAN = np.float32("nan")
PATTERNS = ("all_feasible", "none_feasible", "mixed", "tie_in_j", "one_nan", "all_nan", "candidate_0_elite")
SHAPES = list(itertools.product((1, 3), (1, 3, 6), (1, 3)))  # (H, ad, N)


def refit_oracle(disc, budget, eps, mu, sd, z, N, K, H, ad, n_elite, momentum, min_std):
    """``osrl_plan_refit`` for round >= 1 in fp64: sort by the key tuple, then mean / std / mix / fma."""
    J, C = disc[:, 0].reshape(N, K), disc[:, 1].reshape(N, K)
    eps = eps.reshape(H, N, K, ad)
    mom, rank = np.float64(np.float32(momentum)), np.zeros((N, K), np.int32)
    mu, sd = mu.astype(np.float64), sd.astype(np.float64)
    for n in range(N):
        def key(k):
            j, c = float(J[n, k]), float(C[n, k])
            if j != j or c != c:
                return (2, 0.0, 0.0, k)
            return (0, 0.0, -j, k) if c <= budget[n] else (1, c, -j, k)
        order = sorted(range(K), key=key)
        rank[n, order] = np.arange(K)
        n_e = min(n_elite, sum(key(k)[0] < 2 for k in range(K)))
        if n_e == 0:
            continue
        el = np.array(order[:n_e])
        u = eps[:, n, el, :].astype(np.float64)  # [H, n_e, ad], ascending rank
        u[:, el == 0, :] = 0.0
        m = np.cumsum(u, 1)[:, -1] / n_e
        s = np.sqrt(np.cumsum((u - m[:, None]) * (u - m[:, None]), 1)[:, -1] / n_e)
        mu[n] = mom * mu[n] + (1.0 - mom) * m
        sd[n] = np.maximum(mom * sd[n] + (1.0 - mom) * s, np.float64(np.float32(min_std)))
    mu, sd = mu.astype(np.float32), sd.astype(np.float32)
    m4, s4 = mu.transpose(1, 0, 2)[:, :, None, :], sd.transpose(1, 0, 2)[:, :, None, :]  # [H, N, 1, ad]
    out = (s4.astype(np.float64) * z.reshape(H, N, K, ad) + m4).astype(np.float32)
    out[:, :, 0] = 0.0
    if K >= 2:
        out[:, :, 1] = m4[:, :, 0]
    return rank, mu, sd, out.reshape(H, N * K, ad)


def scores(pattern, N, K, rng):
    """(disc [N K, 4], budget [N]): costs on quarters, so that ties in C and ``C == budget`` both occur."""
    J = rng.standard_normal((N, K)).astype(np.float32)
    C = (rng.integers(0, 8, (N, K)) / 4).astype(np.float32)
    budget = np.full(N, {"all_feasible": 100.0, "none_feasible": -1.0}.get(pattern, 1.0), np.float32)
    if pattern == "tie_in_j":
        J[:, 1:3], C[:, 1:3] = 5.0, 0.0
    elif pattern == "one_nan":
        J[:, K - 1] = NAN
    elif pattern == "all_nan":
        J[:], C[:, ::2] = NAN, NAN
    elif pattern == "candidate_0_elite":
        J[:, 0], C[:, 0] = 9.0, 0.0
    disc = np.zeros((N * K, 4), np.float32)
    disc[:, 0], disc[:, 1], disc[:, 2] = J.reshape(-1), C.reshape(-1), 0.5
    return disc, budget


def launch(disc, budget, eps, mu, sd, z, N, K, H, ad, n_elite, momentum, min_std, rnd=1, seed=None, base=0):
    """One ``osrl_plan_refit`` on copies of the inputs, each output a guard element longer than it may write."""
    from osrl_amd import _lib as L
    from osrl_amd.engine.core import cur_stream

    def padded(a, dtype=torch.float32):
        t = torch.full((a.size + 8,), 77, dtype=dtype, device=DEV)
        t[:a.size] = dev(a.reshape(-1))
        return t
    e, m, s = padded(eps), padded(mu), padded(sd)
    r = torch.full((N * K + 8,), -7, dtype=torch.int32, device=DEV)
    zd, dd, bd = None if z is None else dev(z), dev(disc), dev(budget)
    sw = None if seed is None else torch.tensor([seed], dtype=torch.int64, device=DEV)
    L.check(L.load().osrl_plan_refit(dd.data_ptr(), bd.data_ptr(), e.data_ptr(), m.data_ptr(), s.data_ptr(),
                                     N, K, H, ad, n_elite, momentum, min_std, rnd, None if sw is None else sw.data_ptr(),
                                     base, None if zd is None else zd.data_ptr(), r.data_ptr(), cur_stream()),
            "osrl_plan_refit")
    torch.cuda.synchronize()
    assert (e[-8:] == 77).all() and (m[-8:] == 77).all() and (s[-8:] == 77).all() and (r[-8:] == -7).all()
    return (r[:-8].cpu().numpy().reshape(N, K), m[:-8].cpu().numpy().reshape(N, H, ad),
            s[:-8].cpu().numpy().reshape(N, H, ad), e[:-8].cpu().numpy().reshape(H, N * K, ad))


@pytest.mark.parametrize("K", (3, 64, 65, 257, 1024))
@pytest.mark.parametrize("pattern", PATTERNS)
def test_refit_against_the_fp64_restatement(pattern, K):
    rng = np.random.default_rng(zlib.crc32(f"{pattern}{K}".encode()))
    for (H, ad, N), n_elite, momentum in itertools.product(SHAPES, (1, K), (0.0, 0.5)):
        disc, budget = scores(pattern, N, K, rng)
        eps, z = (rng.standard_normal((H, N * K, ad)).astype(np.float32) for _ in range(2))
        mu = (0.3 * rng.standard_normal((N, H, ad))).astype(np.float32)
        sd = rng.uniform(0.5, 1.5, (N, H, ad)).astype(np.float32)
        args = (disc, budget, eps, mu, sd, z, N, K, H, ad, n_elite, momentum, 0.05)
        want, got, tag = refit_oracle(*args), launch(*args), f"{pattern} K={K} H={H} ad={ad} N={N} n_e={n_elite} m={momentum}"
        np.testing.assert_array_equal(got[0], want[0], err_msg="elite_rank " + tag)
        for name, g, w in zip(("mu", "sd", "eps"), got[1:], want[1:]):
            np.testing.assert_array_equal(bits(g), bits(w), err_msg=f"{name} {tag}")
        if pattern == "all_nan":
            np.testing.assert_array_equal(bits(got[1]), bits(mu))
            np.testing.assert_array_equal(bits(got[2]), bits(sd))
        elif pattern == "candidate_0_elite":
            assert (got[0][:, 0] == 0).all()
    # round 0: the start of a call, whatever the scores hold
    r0 = launch(*args[:10], 1, 0.5, 0.05, rnd=0)
    assert (r0[0] == np.arange(K)).all() and (r0[1] == 0).all() and (r0[2] == 1).all()
    e0 = z.copy()
    e0[:, 0::K], e0[:, 1::K] = 0.0, 0.0
    np.testing.assert_array_equal(bits(r0[3]), bits(e0))


def test_the_drawn_table():
    """``z_in = None``: the same (seed, round) gives the same bits, another round or seed others; a row does not depend
    on N; and the draws are standard normal -- mean and variance of the 1024 x 3 x 6 table's ``(eps' - mu') / sd'`` within 5
    standard errors (1 / sqrt(n) and sqrt(2 / n), n = 1022 x 3 x 6 drawn values); on the CPU, 200 numpy tables of that
    count stayed within 3.1 standard errors of the mean and 2.5 of the variance."""
    K, H, ad, rng = 1024, 3, 6, np.random.default_rng(7)

    def draw(N, seed, rnd):  # (no valid score: mu' = mu and sd' = sd, whatever N is)
        disc, budget = scores("all_nan", N, K, rng)
        eps = rng.standard_normal((H, N * K, ad)).astype(np.float32)
        mu, sd = np.full((N, H, ad), 0.25, np.float32), np.full((N, H, ad), 0.5, np.float32)
        return launch(disc, budget, eps, mu, sd, None, N, K, H, ad, 100, 0.0, 0.05, rnd=rnd, seed=seed, base=11)[3]
    a = draw(1, 5, 1)
    np.testing.assert_array_equal(bits(draw(1, 5, 1)), bits(a))  # (eps differs between the two: z does not read it)
    for other in (draw(1, 5, 2), draw(1, 6, 1), draw(1, 5 + (1 << 32), 1)):
        assert (bits(other[:, 2:]) != bits(a[:, 2:])).mean() > 0.99
    np.testing.assert_array_equal(bits(draw(3, 5, 1)[:, :K]), bits(a))  # slot 0 of three
    assert (a[:, 0] == 0).all() and (a[:, 1] == 0.25).all()
    zz = ((a.astype(np.float64) - 0.25) / 0.5)[:, 2:].reshape(-1)  # (the fma's one rounding is far below a standard error)
    n = zz.size
    print(f"drawn table: n = {n}, mean {zz.mean():+.5f} (se {n ** -0.5:.5f}), variance {zz.var():.5f} (se {(2 / n) ** 0.5:.5f})")
    assert abs(zz.mean()) <= 5 * n ** -0.5 and abs(zz.var() - 1.0) <= 5 * (2.0 / n) ** 0.5
    assert len(np.unique(bits(a[:, 2:]))) > 0.99 * n


def test_the_planner_with_refinement_rounds():
    H, N, K, b = 3, P.FAN_N, P.FAN_K, P.CS + 0.125
    tr, _ = trainer("bc", H)
    s = P.fan_states(seed=8)
    kw = dict(noise_std=0.3, seed=5)
    p0, pz = tr.planner(menv(N * K, H, mode="mean"), N, H, **kw), tr.planner(menv(N * K, H, mode="mean"), N, H, refine_rounds=0, **kw)
    a0 = p0.act(s, b)
    np.testing.assert_array_equal(bits(pz.act(s, b)), bits(a0))
    assert torch.equal(pz.last_J, p0.last_J) and torch.equal(pz.last_C, p0.last_C)
    assert pz.plan_mean is None and pz.plan_std is None and pz.last_eps is None
    out = []
    for _ in range(2):  # two planners, the same seed: every output bit
        p = tr.planner(menv(N * K, H, mode="mean"), N, H, refine_rounds=2, num_elites=2, **kw)
        a = p.act(s, b)
        out.append([a] + [t.clone() for t in (p.last_J, p.last_C, p.last_first_actions, p.last_eps, p.plan_mean,
                                              p.plan_std, p.elite_rank, p.chosen, p.n_feasible)])
        assert p.guards_intact() and p.graph is not None
    for x, y in zip(*out):
        np.testing.assert_array_equal(bits(x), bits(y))
    a, J, C, first, eps, mean, std, rank, chosen, _ = out[0]
    np.testing.assert_array_equal(bits(J[:, 0]), bits(p0.last_J[:, 0]))  # the policy's proposal does not read the table
    np.testing.assert_array_equal(bits(C[:, 0]), bits(p0.last_C[:, 0]))
    np.testing.assert_array_equal(bits(eps[:, :, 1]), bits(mean.transpose(0, 1)))
    np.testing.assert_array_equal(bits(a), bits(first[torch.arange(N), chosen.long()]))
    assert (std >= 0.05).all() and not torch.equal(J[:, 2:], p0.last_J[:, 2:])
    assert (np.sort(rank.cpu().numpy(), 1) == np.arange(K)).all()
    a_again = p.act(s, b)  # call 1 of the same planner: another seed word, the graph kept
    assert p.calls == 2 and np.isfinite(a_again).all() and p.guards_intact()
