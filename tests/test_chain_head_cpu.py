"""The summation order of the one-output head of the 8-wave chain kernels (csrc/mlp.hip), without a GPU.

Two numpy float32 models of the same sum, written independently of each other from the kernels' description:

* ``splitk_mfma``: the layer form (narrow_layer_splitk).  Wave p of the 8 owns the k-steps [nk p / 8, nk (p + 1) / 8) and
  walks them from a start that depends on the workgroup and the wave (k_rot / k_at); every k-step is four
  v_mfma_f32_16x16x4_f32 on a 16 x 16 tile, lane (m, kq) feeding A[m][16 ks + 4 kq + t] and the packed weight
  W[16 ks + 4 kq + t][n] to the t-th of them; an MFMA is D = fma(a_k3, b_k3, fma(a_k2, b_k2, fma(a_k1, b_k1, fma(a_k0,
  b_k0, C)))), one rounding per product.  The eight partial tiles are then added in wave order, from 0.
* ``chain``: narrow_layer_chain.  One scalar fmaf chain per (row, part) in the order t outside, kq inside, per k-step,
  from +0; a part without k-steps contributes +0; the partials are added in part order, from 0.

The two must agree bit for bit for every row, part split and workgroup index: that pins the index arithmetic of the
chain here, so that a device failure of tests/test_gpu_chain_head.py is about the instruction, not the order."""
import numpy as np
import pytest

NW = 8


def fma32(a, b, c):
    """Correctly rounded float32 fma on arrays: the exact product and a round-to-odd float64 sum, then one rounding to
    float32 (53 >= 2 * 24 + 2 bits: no double rounding)."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b  # exact: 24 x 24 bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # TwoSum: p + c == s + err exactly
    bits = s.view(np.int64)
    even = (bits & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def add32(a, b):
    return (np.asarray(a, dtype=np.float32) + np.asarray(b, dtype=np.float32)).astype(np.float32)


def k_rot(nk, bx, by, w):
    return (bx * 5 + by * 3 + w) % nk


def k_at(kc, rot, nk, kc0):
    k = kc + rot
    return kc0 + (k - nk if k >= nk else k)


def mfma_16x16x4(a_lane, b_lane, C):
    """v_mfma_f32_16x16x4_f32: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]; D[i][j] is the k-ordered fma chain
    over the four k-slots on top of C[i][j]."""
    A = np.zeros((16, 4), np.float32)
    B = np.zeros((4, 16), np.float32)
    for l in range(64):
        A[l & 15, l >> 4] = a_lane[l]
        B[l >> 4, l & 15] = b_lane[l]
    D = C.copy()
    for k in range(4):
        D = fma32(A[:, k][:, None], B[k, :][None, :], D)
    return D


def splitk_mfma(act, w_col, nk, bx, by):
    """act [16, 16 nk], w_col [16 nk] (the one real column; the pack's other 15 columns are zero)."""
    W = np.zeros((16 * nk, 16), np.float32)
    W[:, 0] = w_col
    partial = []
    for wave in range(NW):
        k_lo, k_hi = (nk * wave) // NW, (nk * (wave + 1)) // NW
        k_n = k_hi - k_lo
        acc = np.zeros((16, 16), np.float32)
        if k_n > 0:
            rot = k_rot(k_n, bx, by, wave)
            for kc in range(k_n):
                ks = k_at(kc, rot, k_n, k_lo)
                for t in range(4):
                    a_lane = np.array([act[l & 15, 16 * ks + 4 * (l >> 4) + t] for l in range(64)], np.float32)
                    b_lane = np.array([W[16 * ks + 4 * (l >> 4) + t, l & 15] for l in range(64)], np.float32)
                    acc = mfma_16x16x4(a_lane, b_lane, acc)
        partial.append(acc)
    s = np.zeros((16, 16), np.float32)
    for q in range(NW):
        s = add32(s, partial[q])
    return s


def chain(act, w_col, nk, bx, by):
    out = np.zeros(16, np.float32)
    for r in range(16):
        partial = []
        for p in range(NW):
            k_lo = (nk * p) // NW
            k_n = (nk * (p + 1)) // NW - k_lo
            acc = np.float32(0.0)
            if k_n > 0:
                rot = k_rot(k_n, bx, by, p)
                for kc in range(k_n):
                    ks = k_at(kc, rot, k_n, k_lo)
                    for t in range(4):
                        for kq in range(4):
                            k = 16 * ks + 4 * kq + t
                            acc = fma32(act[r, k], w_col[k], acc)[()]
            partial.append(acc)
        s = np.float32(0.0)
        for q in range(NW):
            s = add32(s, partial[q])[()]
        out[r] = s
    return out


def test_fma32_is_one_rounding():
    # a * b + c with the product's low bits exactly at a float32 tie that a float64 sum would break the wrong way
    a, b = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)  # product = 1 + 2^-11 + 2^-24
    c = np.float32(2.0 ** -60)
    assert fma32(a, b, c) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)  # above the tie: rounds up
    assert fma32(a, b, -c) == np.float32(1 + 2.0 ** -11)              # below the tie: rounds down
    assert fma32(a, b, np.float32(0)) == np.float32(1 + 2.0 ** -11)   # the tie itself: to even
    rs = np.random.RandomState(0)
    x, y, z = (rs.randn(1000).astype(np.float32) for _ in range(3))
    from fractions import Fraction
    for i in range(0, 1000, 37):
        exact = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i]))
        lo = np.nextafter(fma32(x[i], y[i], z[i]), np.float32(-np.inf), dtype=np.float32)
        hi = np.nextafter(fma32(x[i], y[i], z[i]), np.float32(np.inf), dtype=np.float32)
        got = Fraction(float(fma32(x[i], y[i], z[i])))
        assert abs(exact - got) <= abs(exact - Fraction(float(lo))) and abs(exact - got) <= abs(exact - Fraction(float(hi)))


@pytest.mark.parametrize("nk", [4, 9, 16])
def test_part_split_covers_every_k_step_once(nk):
    seen = []
    for p in range(NW):
        k_lo = (nk * p) // NW
        k_n = (nk * (p + 1)) // NW - k_lo
        for bx, by in ((0, 0), (2, 1), (7, 3)):
            if k_n:
                walk = [k_at(kc, k_rot(k_n, bx, by, p), k_n, k_lo) for kc in range(k_n)]
                assert sorted(walk) == list(range(k_lo, k_lo + k_n)), (nk, p, bx, by, walk)
        seen += list(range(k_lo, k_lo + k_n))
    assert seen == list(range(nk))


@pytest.mark.parametrize("nk", [4, 9, 16])
@pytest.mark.parametrize("bx,by", [(0, 0), (1, 0), (2, 3), (5, 1)])
def test_chain_order_equals_the_mfma_split_k_order(nk, bx, by):
    rs = np.random.RandomState(100 * nk + 10 * bx + by)
    act = np.maximum(rs.randn(16, 16 * nk), 0).astype(np.float32)  # a relu layer's output: exact zeros among the values
    w = rs.uniform(-0.1, 0.1, 16 * nk).astype(np.float32)
    K = 16 * nk - 5  # a ragged width: the k-padding is zero in both operands
    act[:, K:] = 0
    w[K:] = 0
    ref = splitk_mfma(act, w, nk, bx, by)
    got = chain(act, w, nk, bx, by)
    assert ref[:, 0].tobytes() == got.tobytes(), np.abs(ref[:, 0] - got).max()
    assert not ref[:, 1:].any() and not np.signbit(ref[:, 1:]).any()  # the pad columns are +0 (the element loop rewrites them)
    # the order matters at all: the plain ascending-k chain differs somewhere, or the test would pin nothing
    plain = np.zeros(16, np.float32)
    for k in range(16 * nk):
        plain = fma32(act[:, k], w[k], plain)
    if nk >= 9:
        assert plain.tobytes() != got.tobytes()
