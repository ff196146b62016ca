"""The error bound of one operator sweep Y = L_A X per form, the test blocks X, and a numpy emulation of the stored split-f16 sweep.
Shared by tests/test_operator_bound.py (CPU) and tests/test_gpu_operator.py.

Reference: Yref = alpha (diag(D) X - K_A X) in float64 (stored forms: the stored matrix, f32 bits widened, times X).
Bound, componentwise:  |Y - Yref|_ij <= gamma (|L| |X|)_ij + a_ij,   |L| = alpha (diag(D) + K_A),
gamma = (K + c) u + s v,  u = 2^-24 (one f32 rounding), v = 2^-22 (one rounding of a split f16 (hi, lo) operand: |x - hi - lo| <=
2^-22 |x|, and the lo x lo product the three-product scheme leaves out: 2^-11 * 2^-11).

K counts the links of the longest f32 accumulation chain of one output, ONE LINK PER MFMA INSTRUCTION (and one per explicit f32
add): the products of f16 operands are exact in f32, and an instruction is taken to add its 16 (f16) or 2 (f32) products to the
accumulator with an error of at most u of the magnitudes summed. The instruction's internal order and rounding are not documented;
this is the model, not a derived fact. profiles/operator_error.json records how far below the bound the kernels stay.

form      K (links)                                   s   c   where (csrc/, line numbers as of this commit)
f32       p64 / 2 + 1                                 0   0   k_block_matvec: eigen.hip:85, one mfma_f32_32x32x2f32 per 2 k over p64 =
                                                              round_up(p, 64) (the loop :66 over ntiles = p32 / 32 tiles, 16 MFMAs each);
                                                              +1: the products themselves are rounded f32
f16s      12 ceil(T / ksplit) + ksplit                3   0   k_block_matvec_f16s: T = p64 / 64 K tiles, 4 steps (eigen.hip:268) x 3 MFMAs
                                                              (:285-287) per tile, a slab of ceil(T / ksplit) tiles per chain (:301,
                                                              mv_ksplit :353), then k_mv_sum_splits' (:349) or the skipping walk's
                                                              `run +=` (:323) ksplit adds; s: A split (:272-279), X split (k_mv_x_split,
                                                              :152-153), lo x lo
grid      3 ks + 3 ksc                                6   25  k_grid_rowpass (nystroem_grid.inc:182, 247-249; the row-tile form :303
                                                              likewise): ks = ceil(nr / 16) steps x 3 MFMAs; k_grid_colpass (:860-862):
                                                              ksc = ceil(nc / 16) steps x 3; s: (P :58-60, Er X :229-233) and (Ec
                                                              :620-622, T :843-849) split + lo x lo each; c = 17 + 3 (entries, below)
                                                              + 1 (y = Er * X, :220) + 4 (epilogue, :1311)
rank      3 ks + 3 R / 16 + 3 ksc                     9   26  the same row pass on R <= 64 terms, T' = F S (nystroem_rank.inc:450 / :825,
                                                              R / 16 steps x 3) and the Ec contraction (:495 / :888; k_rank_samples
                                                              :1121). Three GEMMs in a row, and in each BOTH operands are split pairs
                                                              (Er and f X; F and S; Ec and T'): 3 roundings x 3 = 9. The issue's s <= 8
                                                              cannot hold for this form short of changing its arithmetic.
band      3 nr ksc                                    3   26  k_band (nystroem_band.inc:472-474): one k-step x 3 MFMAs per (grid row in
                                                              the band, block of 16 sample columns in the window); on images smaller
                                                              than the radius the band is the whole grid, so the chain is nr ksc steps
                                                              -- the entries are generated, not factored, hence no shorter chain;
                                                              c = 17 + 3 (entries) + 2 (y = (era ec) pp, :444) + 4 (epilogue, :690)
pix band  3 nr ksc                                    3   132 the same with P = v_exp_f32(dist2 * -s_val) generated per entry: up to 7
                                                              roundings enter the exponent (below), 1 u each amplified by t ln 2
epilogue (c = 4, k_gridop_finish / k_band's SAMPLES epilogue): float(D), one fmaf, float(alpha), one multiply.
entries (factored forms; the stored forms are compared with their own stored entries): the tables hold exp2(-s q) with s rounded
to f32 once (make_coef), a relative error of t ln 2 u on an entry 2^-t: <= 17 u for t <= 24; beyond, K < 2^-24 and the error is
below 2^-44 absolutely, which the floors below cover. +1 u per table (Er, Ec, P) for its own rounding to f32.

a_ij, the parts the forms drop by design. An f16 (hi, lo) pair cannot hold less than 2^-25 (half the subnormal step): an operand
scaled so that its column stays below 2^14 loses up to 2^-39 of that column's largest magnitude, absolutely.
f16s      2^-35 sum_k |X_kj| (entries with |2^10 L_ik| < 2^-25 are zero pairs: what exact-zero skipping relies on) + 2^-38 max|X_:j|
          sum_k |L_ik| (X scaled into [2^13, 2^14) by k_mv_col_absmax)
grid,band alpha p 2^-36 max|X_:j|: 2^15 P, 2^15 Ec (and the band's 2^15 Er Ec: the samples beyond its radius) floor at 2^-40, X
          scaled below 2^14 at 2^-39, T scaled below 2^14 with the bound nr max|X| (k_gridop_scales) at 2^-38 nr per entry, nc
          entries per output: together below p 2^-37 max|X_:j|, taken with a factor 2
rank      alpha p 2^-25 max|X_:j| + 2^-30 alpha (K_sp |X|)_ij. S is scaled into [2^6, 2^7) of its bound nr max|X| (RANK_S_SCALE,
          nystroem_rank.inc:39) and so floors at 2^-25 / 2^6 = 2^-31 nr max|X|; a T' entry sums R of them weighted by f_k(v),
          sum_k |f_k| <= sqrt(R) = 8 (sum_k f_k^2 = P(0) = 1): 2^-28 nr max|X|. 2^8 F (RANK_F_SCALE, :38) floors at 2^-33 per
          entry of F, times |S| <= nr max|X|, R = 64 terms: 2^-27 nr max|X|. nc entries of T' per output (Ec <= 1): p (2^-28 +
          2^-27) max|X| = 1.5 p 2^-27, plus the row pass' and T' split's floors of the grid form (below p 2^-37): under p 2^-26,
          taken with the same factor 2 as the grid and band forms: p 2^-25. RANK_TOL = 2^-30 = max |F F^T - P| (:32). The rank
          form's roundings are relative to sum_k |f_k(v) f_k(w)| <= 1, not to P(|v - w|): its gamma term is taken against
          |L|_sp = alpha (diag(D) + K_sp), K_sp the spatial factor of the kernel alone. The order in which k_rank_colpass
          accumulates T' over its segments was not traced instruction by instruction: K counts its MFMAs per output, as above.
"""
import numpy as np

U = 2.0 ** -24
V = 2.0 ** -22


def round_up(x, m):
    return (x + m - 1) // m * m


def grid_shape(idx, width):
    """(nr, nc) of a tensor-grid sample set."""
    idx = np.asarray(idx, dtype=np.int64)
    nr, nc = np.unique(idx // width).size, np.unique(idx % width).size
    assert nr * nc == idx.size
    return nr, nc


def counts(form, p, nr=0, nc=0, ksplit=1, R=64):
    """(K, s, c) of the table above."""
    p64 = round_up(p, 64)
    ks, ksc = -(-nr // 16), -(-nc // 16)
    if form == "f32":
        return p64 // 2 + 1, 0, 0
    if form == "f16s":
        return 12 * -(-(p64 // 64) // max(ksplit, 1)) + max(ksplit, 1), 3, 0
    if form == "grid":
        return 3 * ks + 3 * ksc, 6, 25
    if form == "rank":
        return 3 * ks + 3 * (R // 16) + 3 * ksc, 9, 26
    if form == "band":
        return 3 * nr * ksc, 3, 26
    if form == "pix_band":
        return 3 * nr * ksc, 3, 132
    raise ValueError(form)


def gamma(form, p, **kw):
    K, s, c = counts(form, p, **kw)
    return (K + c) * U + s * V


def bound(form, g, absL_X, X, p, alpha=None, absL_rowsum=None, Ksp_X=None):
    """gamma (|L| |X|) + a for the rows < p of X (float64 [p, ld]). absL_X = |L| |X| (rank: |L|_sp |X|); stored f16s: absL_rowsum
    = sum_k |L_ik|; rank: Ksp_X = K_sp |X|."""
    aX = np.abs(X[:p])
    colmax, col1 = aX.max(axis=0), aX.sum(axis=0)
    b = g * absL_X
    if form == "f16s":
        b = b + 2.0 ** -35 * col1[None, :] + 2.0 ** -38 * absL_rowsum[:, None] * colmax[None, :]
    elif form in ("grid", "band", "pix_band"):
        b = b + alpha * p * 2.0 ** -36 * colmax[None, :]
    elif form == "rank":
        b = b + alpha * p * 2.0 ** -25 * colmax[None, :] + 2.0 ** -30 * alpha * Ksp_X
    return b


def make_block(p, ld, m, seed, rows=None):
    """The test block X, float32 [rows = round_up(p, 64), ld], m < ld real columns: normal columns scaled by 2^e, e spread evenly over
    -30 .. +30 in shuffled order; column 1 all zero; column 2 the unit vector e_(p // 2); column 3 zero on the even rows (there
    the diagonal of L contributes nothing to the bound: only the contraction with K_A is left); rows >= p and columns >= m zero."""
    assert 4 <= m < ld
    rng = np.random.default_rng(seed)
    rows = round_up(p, 64) if rows is None else rows
    X = np.zeros((rows, ld), dtype=np.float32)
    e = np.round(np.linspace(-30, 30, m)).astype(int)
    rng.shuffle(e)
    X[:p, :m] = (rng.normal(size=(p, m)) * 2.0 ** e[None, :]).astype(np.float32)
    X[:, 1] = 0.0
    X[:, 2] = 0.0
    X[p // 2, 2] = 1.0
    X[0::2, 3] = 0.0
    return X


# ---- numpy emulation of the stored split-f16 sweep (k_mv_col_absmax, k_mv_x_split, k_block_matvec_f16s, k_mv_sum_splits) --------

def _split(v32):
    hi = v32.astype(np.float16)
    lo = (v32 - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def emulate_f16s(A, X, p, ksplit=1, defect=None):
    """Y = A X as the kernel computes it. A: float32 [p, p] symmetric; X: float32 [round_up(p, 64), ld]. One MFMA = the exact sum
    of its 16 products added to the f32 accumulator with one rounding (the model of the bound). defect: None, "drop_lo_hi" (the
    A-lo x X-hi product left out), "last_tile_scale" (the last K tile taken one binade too large)."""
    p64, ld = X.shape
    assert p64 == round_up(p, 64) and A.shape == (p, p)
    mx = np.abs(X[:p]).max(axis=0)
    ex = np.zeros(ld, dtype=int)
    ok = (mx > 0) & (mx < 3.0e38)
    ex[ok] = 13 - (np.frexp(mx[ok])[1] - 1)   # 13 - ilogbf(max)
    ex = np.clip(ex, -100, 100)
    scale, inv = np.ldexp(np.float32(1), ex).astype(np.float32), np.ldexp(np.float32(1), -ex - 10).astype(np.float32)
    xh, xl = _split((X * scale[None, :]).astype(np.float32))
    Ap = np.zeros((p, p64), dtype=np.float32)
    Ap[:, :p] = A * np.float32(1024.0)
    ah, al = _split(Ap)
    f8 = np.float64
    ntiles = p64 // 64
    parts = []
    for sl in range(ksplit):
        acc = np.zeros((p, ld), dtype=np.float32)
        for kt in range(ntiles * sl // ksplit, ntiles * (sl + 1) // ksplit):
            w = 2.0 if (defect == "last_tile_scale" and kt == ntiles - 1) else 1.0
            for t in range(4):
                k = np.r_[kt * 64 + 8 * t:kt * 64 + 8 * t + 8, kt * 64 + 32 + 8 * t:kt * 64 + 32 + 8 * t + 8]
                prods = [(ah, xh), (ah, xl)] + ([] if defect == "drop_lo_hi" else [(al, xh)])
                for a, x in prods:
                    acc = (acc.astype(f8) + w * (a[:, k].astype(f8) @ x[k, :].astype(f8))).astype(np.float32)
        parts.append(acc)
    if ksplit == 1:
        tot = parts[0]
    else:
        tot = np.zeros((p, ld), dtype=np.float32)
        for acc in parts:
            tot = (tot + acc).astype(np.float32)
    Y = np.zeros((p64, ld), dtype=np.float32)
    Y[:p] = tot * inv[None, :]
    return Y


def check(Y, Yref, B, p):
    """(worst ratio |Y - Yref| / B over the rows < p where B > 0, all elements within the bound)."""
    err = np.abs(Y[:p].astype(np.float64) - Yref)
    pos = B > 0
    ratio = float((err[pos] / B[pos]).max()) if pos.any() else 0.0
    return ratio, bool((err <= B).all())
