"""osrl_linear_split / osrl_split_planes (csrc/linear_split.hip) on the device against an fp64 product of the same fp32
inputs: the derived per-output bound, the error class of fp32 sgemm, determinism, and the engine's fallback for a shape
the kernel does not take."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M_ROWS = 333  # two full 128-row tiles and a ragged tail of 77 rows

# C5's projections (K, N, residual): in_proj / mlp.0 / mlp.2 + resid / out_proj + resid / the dX of in_proj
C5_SHAPES = [(256, 1024, False), (256, 768, False), (1024, 256, True), (256, 256, True), (768, 256, False)]


def bound_factor(K):
    return (6 * K + 2) * 2.0 ** -24 * 1.01 + 2.0 ** -23 + 2.0 ** -32


def make_planes(W, transpose=False):
    """The three bf16 planes of W [out,in] (``transpose``: of W^T [in,out]) by ONE osrl_split_planes launch."""
    from osrl_amd import _lib as L
    from osrl_amd.engine.core import cur_stream
    out, in_ = W.shape
    ents = (L.PackEntryT * 1)()
    ents[0].src_off, ents[0].out, ents[0].in_ = 0, out, in_
    ents[0].f_off, ents[0].b_off = (-1, 0) if transpose else (0, -1)
    d_ents = torch.frombuffer(bytearray(bytes(ents)), dtype=torch.uint8).to(DEV)
    planes = torch.zeros(3 * out * in_, dtype=torch.int16, device=DEV)
    L.check(L.load().osrl_split_planes(W.data_ptr(), None if transpose else planes.data_ptr(),
                                       planes.data_ptr() if transpose else None, d_ents.data_ptr(), 1, out * in_,
                                       cur_stream()), "osrl_split_planes")
    torch.cuda.synchronize()
    return planes


def run_split(A, lda, M, K, planes, N, bias, resid, ldr, Y, ldy):
    from osrl_amd import _lib as L
    from osrl_amd.engine.core import cur_stream
    L.check(L.load().osrl_linear_split(A.data_ptr(), lda, M, K, planes.data_ptr(), N * K, N,
                                       None if bias is None else bias.data_ptr(),
                                       None if resid is None else resid.data_ptr(), ldr, Y.data_ptr(), ldy, cur_stream()),
            "osrl_linear_split")


def inputs(K, N, seed, M=M_ROWS):
    rs = np.random.RandomState(seed)
    A = (rs.randn(M, K) * 1.5).astype(np.float32)
    W = (rs.randn(N, K) * 0.05).astype(np.float32)
    b = (rs.randn(N) * 0.1).astype(np.float32)
    R = rs.randn(M, N).astype(np.float32)
    return A, W, b, R


def ref64(A, W, b, R):
    y = A.astype(np.float64) @ W.astype(np.float64).T
    s = np.abs(A.astype(np.float64)) @ np.abs(W.astype(np.float64)).T
    if b is not None:
        y, s = y + b.astype(np.float64), s + np.abs(b.astype(np.float64))
    if R is not None:
        y, s = y + R.astype(np.float64), s + np.abs(R.astype(np.float64))
    return y, s


def test_planes_are_the_exact_split_in_both_orientations():
    rs = np.random.RandomState(1)
    W = (rs.randn(96, 160) * 0.3).astype(np.float32)  # ragged 32 x 32 tiles in both dimensions
    W[0, :4] = [0.0, -0.0, 3.0e38, -1e-30]
    Wd = torch.from_numpy(W).to(DEV)
    for tr in (False, True):
        p = make_planes(Wd, transpose=tr).cpu().numpy().view(np.uint16).reshape(3, *(W.T.shape if tr else W.shape))
        f = (p.astype(np.uint32) << 16).view(np.float32)
        want = W.T if tr else W
        assert np.array_equal(f[0], (np.ascontiguousarray(want).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32))
        assert np.array_equal(f[0].astype(np.float64) + f[1].astype(np.float64) + f[2].astype(np.float64),
                              want.astype(np.float64))


@pytest.mark.parametrize("K,N,res", C5_SHAPES)
@pytest.mark.parametrize("with_bias", [True, False])
def test_split_gemm_bound_and_class(K, N, res, with_bias):
    """Per output |y - y64| <= ((6K + 2) 2^-24 1.01 + 2^-23 + 2^-32) (sum_k |a_k||w_k| + |bias| + |resid|), y64 the fp64
    product of the same fp32 inputs.  Derivation: every fp32 input is the exact sum of three bf16 pieces that carry its
    sign, so sum over the kept piece products of |a_i w_j| <= |a||w|; each of the 6K kept products is exact in fp32 (8 x
    8 significant bits) and the matrix unit adds them in fp32: at most 6K roundings of 2^-24 relative to a partial sum
    that never exceeds sum |a||w|, plus one rounding each for the bias and the residual add (the + 2; 1.01 covers the
    second-order terms).  The three dropped products are m l + l m + l l <= (2^-8 2^-16 + 2^-16 2^-8 + 2^-32)|a||w| <
    (2^-23 + 2^-32)|a||w|.  Nothing in it is measured.

    Class: the rms error against fp64 is at most twice that of torch.nn.functional.linear in fp32 on the CPU on the same
    inputs (what the reference runs); a split with a missing product or plain bf16 is orders away."""
    from osrl_amd import _lib as L
    lib = L.load()
    M = M_ROWS
    assert M % 128 != 0 and int(lib.osrl_linear_split_supported(M, K, N)) == 1
    A, W, b, R = inputs(K, N, seed=K + N)
    b_, R_ = (b if with_bias else None), (R if res else None)
    At, Wt = torch.from_numpy(A).to(DEV), torch.from_numpy(W).to(DEV)
    planes = make_planes(Wt)
    Y = torch.full((M + 1, N), float("nan"), device=DEV)  # (row M must stay untouched: the tail is masked)
    run_split(At, K, M, K, planes, N, None if b_ is None else torch.from_numpy(b_).to(DEV),
              None if R_ is None else torch.from_numpy(R_).to(DEV), N, Y, N)
    torch.cuda.synchronize()
    assert torch.isnan(Y[M]).all()
    y = Y[:M].cpu().numpy().astype(np.float64)
    y64, s = ref64(A, W, b_, R_)
    err = np.abs(y - y64)
    tol = bound_factor(K) * s
    print(f"K={K} N={N} bias={with_bias} resid={res}: max err / bound = {(err / tol).max():.3e}")
    assert (err <= tol).all(), f"worst err / bound {(err / tol).max():.3e}"
    yc = torch.nn.functional.linear(torch.from_numpy(A), torch.from_numpy(W), None if b_ is None else torch.from_numpy(b_))
    if R_ is not None:
        yc = yc + torch.from_numpy(R_)
    rms = float(np.sqrt(np.mean(err ** 2)))
    rms_cpu = float(np.sqrt(np.mean((yc.numpy().astype(np.float64) - y64) ** 2)))
    print(f"K={K} N={N}: rms err split {rms:.3e}, fp32 F.linear on the CPU {rms_cpu:.3e}")
    assert rms <= 2 * rms_cpu, (rms, rms_cpu)


def test_split_gemm_non_contiguous_leading_dimensions():
    K, N, M = 256, 256, M_ROWS
    A, W, b, R = inputs(K, N, seed=5)
    lda, ldr, ldy = K + 12, N + 7, N + 5  # (lda a multiple of 4: the kernel reads 16-byte chunks of A)
    Ab = torch.full((M, lda), float("nan"), device=DEV)
    Ab[:, :K] = torch.from_numpy(A).to(DEV)
    Rb = torch.full((M, ldr), float("nan"), device=DEV)
    Rb[:, :N] = torch.from_numpy(R).to(DEV)
    Yb = torch.full((M, ldy), 7.0, device=DEV)
    planes = make_planes(torch.from_numpy(W).to(DEV))
    run_split(Ab, lda, M, K, planes, N, torch.from_numpy(b).to(DEV), Rb, ldr, Yb, ldy)
    torch.cuda.synchronize()
    assert (Yb[:, N:] == 7.0).all()
    y64, s = ref64(A, W, b, R)
    assert (np.abs(Yb[:, :N].cpu().numpy().astype(np.float64) - y64) <= bound_factor(K) * s).all()
    # the same bits as the dense call: the order of accumulation does not depend on the strides
    Yd = torch.zeros(M, N, device=DEV)
    run_split(torch.from_numpy(A).to(DEV), K, M, K, planes, N, torch.from_numpy(b).to(DEV), torch.from_numpy(R).to(DEV), N,
              Yd, N)
    assert torch.equal(Yd, Yb[:, :N])


@pytest.mark.parametrize("in_,out", [(256, 1024), (256, 768), (1024, 256), (256, 256)])
def test_split_gemm_dx_orientation(in_, out):
    """dX [M,in] = dY [M,out] W with W [out,in]: the same kernel on the planes of W^T (K = out, N = in), with and
    without the residual the state-head gradient adds."""
    from osrl_amd import _lib as L
    M = M_ROWS
    assert int(L.load().osrl_linear_split_supported(M, out, in_)) == 1
    rs = np.random.RandomState(in_ + 3 * out)
    dY = rs.randn(M, out).astype(np.float32)
    W = (rs.randn(out, in_) * 0.05).astype(np.float32)
    R = rs.randn(M, in_).astype(np.float32)
    planes_t = make_planes(torch.from_numpy(W).to(DEV), transpose=True)
    for resid in (None, R):
        Y = torch.zeros(M, in_, device=DEV)
        run_split(torch.from_numpy(dY).to(DEV), out, M, out, planes_t, in_, None,
                  None if resid is None else torch.from_numpy(resid).to(DEV), in_, Y, in_)
        torch.cuda.synchronize()
        y64, s = ref64(dY, np.ascontiguousarray(W.T), None, resid)
        err = np.abs(Y.cpu().numpy().astype(np.float64) - y64)
        assert (err <= bound_factor(out) * s).all(), (err / (bound_factor(out) * s)).max()


def test_split_gemm_is_deterministic_and_row_independent():
    K, N = 1024, 256
    A, W, b, R = inputs(K, N, seed=9)
    At, bt, Rt = (torch.from_numpy(x).to(DEV) for x in (A, b, R))
    planes = make_planes(torch.from_numpy(W).to(DEV))
    outs = []
    for _ in range(2):
        Y = torch.zeros(M_ROWS, N, device=DEV)
        run_split(At, K, M_ROWS, K, planes, N, bt, Rt, N, Y, N)
        outs.append(Y)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    Y1 = torch.zeros(100, N, device=DEV)  # another M: the same rows get the same bits
    run_split(At, K, 100, K, planes, N, bt, Rt, N, Y1, N)
    assert torch.equal(Y1, outs[0][:100])


def test_non_finite_inputs_give_non_finite_outputs():
    K, N, M = 256, 128, 40
    A, W, b, R = inputs(K, N, seed=11, M=M)
    A[3, 17], A[5, 200], A[7, 0] = np.inf, -np.inf, np.nan
    W[9, 31] = np.inf
    planes = make_planes(torch.from_numpy(W).to(DEV))
    Y = torch.zeros(M, N, device=DEV)
    run_split(torch.from_numpy(A).to(DEV), K, M, K, planes, N, None, None, 0, Y, N)
    y = Y.cpu().numpy()
    bad = np.zeros((M, N), bool)
    bad[[3, 5, 7], :] = True
    bad[:, 9] = True
    assert not np.isfinite(y[bad]).any()
    assert np.isfinite(y[~bad]).all()


def test_unsupported_shape_is_refused_and_the_engine_keeps_osrl_linear():
    """The action head's N = 2 * action_dim columns: osrl_linear_split_supported is 0, the entry point itself returns -1,
    and an engine built with matmul="bf16x3" routes that layer (and its input gradient) to osrl_linear."""
    from osrl_amd import _lib as L
    from cases import CDT_CASES
    from test_gpu_cdt import build_cdt_gpu
    lib = L.load()
    c = CDT_CASES["cdt_mid"]
    BT, E, nh = c.B * c.T, c.E, 2 * c.ad
    assert int(lib.osrl_linear_split_supported(BT, E, nh)) == 0
    x = torch.zeros(BT, E, device=DEV)
    assert lib.osrl_linear_split(x.data_ptr(), E, BT, E, x.data_ptr(), nh * E, nh, None, None, 0, x.data_ptr(), nh, None) == -1
    m, tr, _ = build_cdt_gpu(c, matmul="bf16x3")
    e = m.engine(c.B, tr.cfg)
    assert e.plan.matmul == "bf16x3"
    assert e.linear_kernel(e.head_out) == "osrl_linear"
    assert e.linear_kernel("cdt.state_pred_head.weight") == "osrl_linear"
    assert e.linear_kernel(e.head_out, dx=True) == "osrl_linear"             # K = 6 -> N = 128: not a K the kernel takes
    assert e.linear_kernel("cdt.blocks.0.mlp.0.weight") == "osrl_linear_split"
    assert e.linear_kernel("cdt.blocks.0.mlp.0.weight", dx=True) == "osrl_linear_split"
    assert m.groups["cdt"].planes_w is not None and "cdt.blocks.0.mlp.0.weight" in m.groups["cdt"].pw_off
    assert e.head_out not in m.groups["cdt"].pw_off
