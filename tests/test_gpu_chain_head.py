"""The one-output Q head of the 8-wave forward chain kernels as an fmaf chain (csrc/mlp.hip: narrow_layer_chain) against
the layer form it replaces (OSRL_CHAIN_HEAD=0): bit for bit, and both against fp64 (forward, and the backward that starts
from the forward's saved activations).  The order itself is pinned without a GPU by tests/test_chain_head_cpu.py."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ACTS = ["relu", "relu", "id"]
DIMS = {"144": [21, 144, 144, 1],   # head nk = 9: parts of one and of two k-steps
        "256": [78, 256, 256, 1]}   # the Q networks of the CPQ step
ROWS = [40, 16]                     # three tiles with a ragged last one; one full tile
NETS = [2, 4]                       # blockIdx.y enters the k-walk's rotation


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _takes_the_8_wave_chain_form(dims, rows, E, extra=0):
    """choose_tile of csrc/mlp.hip restated: 16-row tiles, 8 waves, two column blocks per wave -- and the head's narrow
    path (nk >= 4, lda >= 128).  The comparison below must not pass on another kernel silently."""
    maxw = max(list(dims) + [extra])
    nblk = (maxw + 15) // 16
    cpw = (nblk + 3) // 4
    lda = (maxw + 15) // 16 * 16 + 8
    wg32, wg16 = (rows + 31) // 32 * E, (rows + 15) // 16 * E
    eight = cpw > 2 and cpw <= 4 and wg32 < 1024 and wg16 <= 512 and lda >= 128
    return eight and (nblk + 7) // 8 <= 2 and dims[-1] == 1 and (dims[-2] + 15) // 16 >= 4 and maxw > 128


def _mk(E, dims, seed, dev, name="q"):
    from osrl_amd.engine.core import FlatGroup, LayerRef, NetDesc
    rs = np.random.RandomState(seed)
    grp = FlatGroup(name, dev)
    for e in range(E):
        for l in range(len(dims) - 1):
            grp.add(f"{e}.{l}.w", (dims[l + 1], dims[l]))
            grp.mark_weight(f"{e}.{l}.w")
            grp.add(f"{e}.{l}.b", (dims[l + 1],))
    grp.finalize()
    refs, host = [], []
    for e in range(E):
        rr, hh = [], []
        for l in range(len(dims) - 1):
            k = 1 / math.sqrt(dims[l])
            W, b = grp.view(f"{e}.{l}.w"), grp.view(f"{e}.{l}.b")
            W.copy_(torch.tensor(rs.uniform(-k, k, W.shape), dtype=torch.float32))
            b.copy_(torch.tensor(rs.uniform(-k, k, b.shape), dtype=torch.float32))
            rr.append(LayerRef(W, b, grp, f"{e}.{l}.w", f"{e}.{l}.b"))
            hh.append((W.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)))
        refs.append(rr)
        host.append(hh)
    grp.repack()
    return grp, NetDesc(refs, ACTS, 1.0), host


def _setting(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("OSRL_CHAIN_HEAD", raising=False)  # the default: the chain forms
    else:
        monkeypatch.setenv("OSRL_CHAIN_HEAD", value)          # (read by the library at every launch)


def _fwd_tensors(run):
    out = [run.y, run.x]
    for e in range(run.net.E):
        out += [run.h[e][l] for l in range(run.net.nl)]
    return [t.clone() for t in out]


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dk", list(DIMS))
def test_forward_is_bit_equal_to_the_layer_form(monkeypatch, dk, rows):
    from osrl_amd.engine.core import MlpRun
    dev, dims = _dev(), DIMS[dk]
    g = torch.Generator().manual_seed(3)
    for E in NETS:
        assert _takes_the_8_wave_chain_form(dims, rows, E)
        _, net, _ = _mk(E, dims, 11 + E, dev)
        x = torch.randn(rows, dims[0], generator=g).to(dev)
        got = {}
        for s in ("0", None):
            _setting(monkeypatch, s)
            run = MlpRun(net, rows, True, dev)
            run.forward(x)
            torch.cuda.synchronize()
            got[s] = _fwd_tensors(run)
        assert len(got["0"]) == 2 + E * 3
        for a, b in zip(got["0"], got[None]):
            assert torch.equal(a, b), (dk, rows, E, (a - b).abs().max().item())
        assert got[None][0].abs().max().item() > 0
    # the pair launch: 2 + 4 nets, the second problem's nets behind the first's on blockIdx.y, unequal rows
    _, n0, _ = _mk(2, dims, 21, dev, "a")
    _, n1, _ = _mk(4, dims, 22, dev, "b")
    r1 = rows + 7
    assert _takes_the_8_wave_chain_form(dims, rows, 2) and _takes_the_8_wave_chain_form(dims, r1, 4)
    x0, x1 = torch.randn(rows, dims[0], generator=g).to(dev), torch.randn(r1, dims[0], generator=g).to(dev)
    got = {}
    for s in ("0", None):
        _setting(monkeypatch, s)
        p0, p1 = MlpRun(n0, rows, True, dev), MlpRun(n1, r1, True, dev)
        p0.forward_with((x0,), p1, (x1,))
        torch.cuda.synchronize()
        got[s] = _fwd_tensors(p0) + _fwd_tensors(p1)
    for a, b in zip(got["0"], got[None]):
        assert torch.equal(a, b), (dk, rows, "pair", (a - b).abs().max().item())


@pytest.mark.parametrize("setting", ["0", None])
@pytest.mark.parametrize("dk", list(DIMS))
def test_both_forms_against_fp64(monkeypatch, dk, setting):
    """What tells a wrong emulation from a wrong baseline should the bit comparison fail.  Bounds: those of
    test_gpu_kernels.py::test_mlp_fwd_bwd (2e-5 forward, 3e-5 backward, relative to the largest reference value)."""
    from osrl_amd.engine.core import MlpRun
    dev, dims, rows, E = _dev(), DIMS[dk], 40, 2
    _setting(monkeypatch, setting)
    _, net, host = _mk(E, dims, 41, dev)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(rows, dims[0], generator=g).to(dev)
    dy = torch.randn(E, rows, 1, generator=g).to(dev)
    dxc = (dims[0] - 6, 6)
    assert _takes_the_8_wave_chain_form(dims, rows, E, extra=dxc[1])
    run = MlpRun(net, rows, True, dev)
    run.forward(x)
    run.setup_backward(dy, need_dz=True, dx_cols=dxc)
    run.backward_dz()
    torch.cuda.synchronize()
    X = x.cpu().numpy().astype(np.float64)
    for e in range(E):
        h, cache = X, [X]
        for l, a in enumerate(ACTS):
            W, b = host[e][l]
            h = h @ W.T + b
            h = np.maximum(h, 0) if a == "relu" else h
            got = run.h[e][l].cpu().numpy()
            err = np.abs(got - h).max()
            assert err < 2e-5 * max(1.0, np.abs(h).max()), (dk, setting, "fwd", e, l, err)
            h = got.astype(np.float64)  # (relu masks from the device's own activations, as test_mlp_fwd_bwd does)
            cache.append(h)
        gr = dy[e].cpu().numpy().astype(np.float64)
        for l in range(2, -1, -1):
            dz = gr * ((cache[l + 1] > 0) if ACTS[l] == "relu" else 1.0)
            got = run.dz[e][l].cpu().numpy()
            err = np.abs(got - dz).max()
            assert err < 3e-5 * max(1.0, np.abs(dz).max()), (dk, setting, "dz", e, l, err)
            gr = dz @ host[e][l][0]
        ref = gr[:, dxc[0]:dxc[0] + dxc[1]]
        err = np.abs(run.dx[e].cpu().numpy() - ref).max()
        assert err < 3e-5 * max(1.0, np.abs(ref).max()), (dk, setting, "dx", e, err)
