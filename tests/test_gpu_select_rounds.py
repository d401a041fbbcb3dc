"""The register-resident quantile select (csrc/glue.hip bit_select / quantile_rows) behind osrl_quantile,
osrl_cpq_ood_select and osrl_cpq_ood_stat, against ``torch.quantile(x, 0.75)`` and ``torch.nonzero(x >= q)``: sizes around
the per-thread row counts (4 / 12 / 20 / 32 rows of 1024) and inputs that exercise the key order -- keys that share no
leading bit (normal, +-inf), keys that share most of them (KL-like), all equal, two neighbouring values with the quantile
position between them and on either, the two keys of +-0.0.  (n = 5 with one +inf puts an infinite value right above a
whole quantile position: torch takes ceil(pos) as the upper neighbour, so the result is the finite element.)"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 5, 1023, 1024, 1025, 20480, 32768]
Q = 0.75


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", torch.cuda.current_device())


def _two_values(n, n_low, g):
    x = torch.full((n,), 0.3125)
    x[torch.randperm(n, generator=g)[:n_low]] = 0.31249997  # (the neighbouring float)
    return x


def _inputs(n):
    """[(name, cpu tensor)] for one size."""
    g = torch.Generator(device="cpu").manual_seed(1000 + n)
    out = [("normal", torch.randn(n, generator=g)),
           ("kl_like", 3.0 + 1e-3 * torch.rand(n, generator=g)),
           ("all_equal", torch.full((n,), 0.7071)),
           ("zeros", torch.where(torch.rand(n, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0)))]
    if n >= 2:
        lo = int(math.floor(Q * (n - 1)))
        # sorted = n_low copies of the smaller value, then the larger: position lo is the last small one (the quantile lies
        # between the two values), the first large one (on the larger), or well inside the small run (on the smaller)
        for name, n_low in (("two_between", lo + 1), ("two_on_upper", lo), ("two_on_lower", min(n, lo + 2))):
            out.append((name, _two_values(n, n_low, g)))
    if n >= 5:
        x = torch.randn(n, generator=g)
        i = torch.randperm(n, generator=g)[:2]
        x[i[0]], x[i[1]] = float("inf"), float("-inf")
        out.append(("infs", x))
    return out


CASES = [(n, name) for n in SIZES for name, _ in _inputs(n)]


@pytest.mark.parametrize("n,name", CASES)
def test_select_matches_torch_quantile_and_nonzero(n, name):
    from osrl_amd.engine import glue as G
    dev = _dev()
    x = dict(_inputs(n))[name].to(dev)
    ref = torch.quantile(x, Q)
    want = torch.nonzero(x >= ref).flatten().to(torch.int32)
    q0, q1, q2, m2 = (torch.full((4,), -5.0, device=dev) for _ in range(4))
    G.quantile(x, n, Q, q0)
    lst = torch.full((n,), -1, dtype=torch.int32, device=dev)
    cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    G.cpq_ood_select(x, n, Q, q1, lst, cnt)
    qc = torch.randn(1, n, generator=torch.Generator(device="cpu").manual_seed(n)).to(dev)
    G.cpq_ood_stat(qc, 1, x, Q, 1, n, n, q2, m2)  # one sample of n rows
    torch.cuda.synchronize()
    r = ref.item()
    print(f"n={n} {name}: torch {r!r} quantile {q0[0].item()!r} select {q1[0].item()!r} stat {q2[0].item()!r} "
          f"count {int(cnt[0].item())} want {want.numel()}")
    assert q0[0].item() == r and q1[0].item() == r and q2[0].item() == r
    c = int(cnt[0].item())
    assert c == want.numel()
    assert torch.equal(lst[:c], want) and bool((lst[c:] == -1).all())
    mean = (torch.where(x >= ref, qc[0], torch.zeros_like(qc[0])).double().sum() / n).item()
    assert abs(m2[0].item() - mean) <= 1e-5 * max(1.0, abs(mean))


@pytest.mark.parametrize("n", [5, 1025, 20480])
def test_list_follows_a_given_quantile(n):
    """quantile_in given: no select runs, the list is the rows that reach THAT value."""
    from osrl_amd.engine import glue as G
    dev = _dev()
    x = torch.randn(n, generator=torch.Generator(device="cpu").manual_seed(n)).to(dev)
    for qv in (-0.5, 0.0, 10.0, -10.0):
        qin = torch.full((4,), qv, device=dev)
        lst = torch.full((n,), -1, dtype=torch.int32, device=dev)
        cnt = torch.zeros(4, dtype=torch.int32, device=dev)
        G.cpq_ood_select(x, n, Q, None, lst, cnt, quantile_in=qin)
        torch.cuda.synchronize()
        want = torch.nonzero(x >= qv).flatten().to(torch.int32)
        c = int(cnt[0].item())
        assert c == want.numel() and torch.equal(lst[:c], want) and bool((lst[c:] == -1).all())
