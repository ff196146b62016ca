"""float64 references for the two blocks of the eigen-solve beside the operator sweep -- classical Gram-Schmidt and the residual
|| A X - X (X^T A X) ||_F -- with numpy emulations of the rounding points of each device form, the test blocks, the tolerance rule
and the residual's error bound. Shared by tests/test_eigen_ref.py (CPU), tests/test_gpu_orthonormalise.py, tests/test_gpu_residual.py,
the two stage tests of tests/test_gpu_parity.py and tools/eigen_blocks_error.py. Plain numpy; blocks are [n, m], one COLUMN per vector
(the device layout). Line numbers: csrc/eigen.hip as of this commit.

Classical Gram-Schmidt as the library defines it (hpc/gram_schmidt.c:29-64): u_k = v_k - sum_{j<k} c_jk u_j with every coefficient
c_jk = <v_k, u_j> / <u_j, u_j> taken from the ORIGINAL v_k, 0 where <u_j, u_j> == 0; Q_k = u_k / |u_k|, a zero-norm column left
unscaled. cgs() is that in float64, in the order of operations of the fp64 oracle (oracle/glf_oracle.c, orc_orthonormalise: a column
is normalised as soon as it is finished and the projections are taken on the normalised columns -- the same projections; sums run
front to back). Two float64 evaluations that sum in different orders differ by cond^2 2^-53, 1e-11 on the graded blocks below,
where an 80-bit evaluation lies 4e-13 to 9e-12 from either: following the oracle's order is what lets the two agree to 1e-12 on
every block without a zero column, which the oracle cannot take (it divides by <u_j, u_j>).

Rounding points the emulations encode
  column-by-column sweep (cgs_sweep_f32; GS=seq and the ill-conditioning fallback):
    dots      <v_k, u_j> in f64 from the f32 values of column k and of the stored u_j     k_gs_dots :978
    coef      c_j = (float)(dot / q_j), 0 where q_j == 0                                  k_gs_fin :1024
    row sum   s_i = sum_j u_ij c_j accumulated in f32 (fused multiply-adds)               k_gs_apply :1048-1049
    update    u_ik = x_ik - s_i in f32, stored as f32                                      k_gs_apply :1051-1052
    q_k       sum_i u_ik^2 in f64 of the stored f32 values                                k_gs_apply :1053, k_gs_fin :1002-1010
    scaling   norms = sqrt(q) (k_gs_norms :1067); X = (float)((double)X / norm) where the norm is not 0   k_scale_all :1102
  Gram-matrix form (the default): G, the LDL^T recurrence, T = C^-1 and X T are all f64 (k_gsf_gram_mfma :1210, gsf_recur_body
    :1293-1318 / :1338-1378, k_gsf_apply :1442 / k_gsf_apply_mfma :1489); the one rounding is the store (float)acc (:1450, :1497).
    Its emulation is cgs() rounded to f32 once: d <= 2^-24.
  panels, more than 256 vectors (cgs_panels; panels_orthonormalise :2120-2137):
    a finished panel is held in f32 (it is the X operand of panel_gram :2128 and of k_gsf_sub :2130 for every later panel);
    C_jq = X_j^T V_q in f64 from the original V_q (k_gsf_gram :1151) for ALL earlier panels j first, then one k_gsf_sub launch per
    earlier panel, each storing V_q = (float)((double)V_q - X_j C_jq) (:1534); then the panel's own Gram-matrix form (or sweep).

Tolerance rule (q_tol, norm_rtol): d = the largest deviation of a form's emulation from cgs() over the columns, each column relative to
its largest magnitude in the reference. The device must agree with cgs() within 4 max(d, 2^-23) max|Q_ref[:, k]| in every entry of
column k: the kernels sum in another order than the emulation, which contributes roundings of the size of the emulation's own (the
factor 4), and 2^-23 is one f32 rounding of an entry next to the column's largest. Norms: relative 2^-24 for the Gram-matrix form
(f64 throughout), 4 max(d_norm, 2^-24) for the sweep.

The residual's bound (residual_bound): componentwise |R_gpu - R_ref| <= B for R = A X - X G, G = X^T A X, so that
| ||R_gpu||_F - ||R_ref||_F | <= ||B||_F. One link per MFMA instruction or explicit f32 add, as in tests/operator_ref.py; u = 2^-24.
  B_op                                   the operator sweep's own bound (operator_ref.bound for the stored form in use, ksplit = 1 as
                                         the longest chain)
  |X| (g_G |X|^T |AX| + |X|^T B_op)      G: k_gram is one chain of min(p, 256) / 2 mfma_f32_32x32x2f32 per 256-row chunk (:1740-1752,
                                         GRAM_ROWS :1721), +1 the rounded f32 products, the chunks summed in f64 (k_gram_sum :1776-1778)
                                         and rounded to f32 once (:1782): g_G = (ceil(min(p, 256) / 2) + 2) u; and the error of AX
  (L + 1) u (|AX| + |X| |G|)             X G and the subtraction: k_resid_mfma is a chain of ld / 2 MFMAs (:1850-1853), +1 the rounded
                                         products, then Y - acc (:1862): L = ld / 2 + 1. The vector k_resid (ld 128, 256) is a chain of m
                                         fmaf starting from Y (:1807-1808): L = m there -- RESID_VECTOR_CHAIN, not the ld / 2 links of
                                         the matrix-pipe form
  |A| E + E |G| + |X| (E^T |A| |X| + |X|^T |A| E)
                                         the difference E >= |X_gpu - X_ref| between the device's f32 X and the test's. K = 0: the
                                         returned block is the orthonormal one after NormaliseVecs, one division by a norm within 2 u of
                                         1 and one rounding: E = 4 u |V|. K >= 1: the tolerance rule above for cgs() of the returned
                                         block. RENORMALISED_INPUT: the returned block is the solver's pre-orthonormalisation block
                                         after one more rounding per entry (NormaliseVecs, k_scale_all :1102), so the test's Q is cgs()
                                         of a block 2^-24 away from the device's input; d includes the deviation of cgs() under one
                                         such rounding (renorm_deviation), which the rule of part 2 alone does not hold.
The sums of squares (:1863, k_sum_partials) are f64 of f32 values and contribute nothing at this scale.
Derived against explicit sweep (derived_bound): per PCG step R -= alpha AP takes two roundings, Y += alpha P two, and one operator
application: |r_derived - r_sweep| <= 2 its (gamma_op + 4 u) || |A| |Y| |T| ||_F.
Both bounds are models, as the operator's is; profiles/eigen_blocks_error.json records how far below them the kernels stay."""
import json
from collections import namedtuple

import numpy as np

import operator_ref as oref

U = 2.0 ** -24
PANEL = 256
GSF_COND_FLOOR = 1e-10          # eigen.hip:1117
f4, f8 = np.float32, np.float64

Cgs = namedtuple("Cgs", "Q norms q T")


# ---- references -----------------------------------------------------------------------------------------------------------------

def cgs(X):
    """Classical Gram-Schmidt in float64. Returns Q [n, m], norms |u_k|, q = <u_k, u_k> and the upper-triangular T with Q = X T."""
    X = np.asarray(X, dtype=f8)
    n, m = X.shape
    Q, q, T = np.zeros((n, m)), np.zeros(m), np.zeros((m, m))
    for k in range(m):
        v, t = X[:, k], np.zeros(m)
        t[k] = 1.0
        if k:
            Qk = Q[:, :k]
            num, den = np.cumsum(Qk * v[:, None], axis=0)[-1], np.cumsum(Qk * Qk, axis=0)[-1]
            f = np.divide(num, den, out=np.zeros(k), where=den != 0)
            u = -1.0 * np.cumsum(Qk * f[None, :], axis=1)[:, -1] + v
            t -= T[:, :k] @ f                 # u_k = v_k - sum_j f_j Q_j  =>  T[:, k] = e_k - sum_j f_j T[:, j]
        else:
            u = v.copy()
        q[k] = np.cumsum(u * u)[-1]
        inv = 1.0 / np.sqrt(q[k]) if q[k] != 0 else 1.0
        Q[:, k], T[:, k] = u * inv, t * inv
    return Cgs(Q, np.sqrt(q), q, T)


def cgs_sweep_f32(X32):
    """The column-by-column sweep with its rounding points (module docstring). Returns (Q float32, norms float64)."""
    X = np.array(X32, dtype=f4)
    n, m = X.shape
    q = np.zeros(m)
    for k in range(m):
        if k:
            dots = X[:, :k].astype(f8).T @ X[:, k].astype(f8)
            coef = np.divide(dots, q[:k], out=np.zeros(k), where=q[:k] != 0).astype(f4)
            s = np.zeros(n, dtype=f4)
            for j in range(k):
                s = (s.astype(f8) + X[:, j].astype(f8) * f8(coef[j])).astype(f4)
            X[:, k] = X[:, k] - s
        xk = X[:, k].astype(f8)
        q[k] = xk @ xk
    norms = np.sqrt(q)
    nz = norms != 0
    X[:, nz] = (X[:, nz].astype(f8) / norms[nz]).astype(f4)
    return X, norms


def cgs_gram_f32(X32):
    """The Gram-matrix form: cgs() of the f32 block, rounded to f32 once."""
    r = cgs(X32)
    return r.Q.astype(f4), r.norms


def cgs_panels(X32, seq=(), cond=None):
    """More than 256 vectors, panel by panel, with the panel path's two rounding points (module docstring). seq: the panels that run
    the sweep instead of the Gram-matrix form (GS=seq: all; an ill-conditioned panel falls back). Returns (Q float32, norms).
    cond: a list that receives, per panel, min_k q_k / G_kk of the block the panel's own Gram-matrix form sees (after the cross-panel
    subtraction): what its fallback decision compares with GSF_COND_FLOOR."""
    X = np.array(X32, dtype=f4)
    n, m = X.shape
    norms = np.zeros(m)
    for q in range(-(-m // PANEL)):
        c0, c1 = q * PANEL, min((q + 1) * PANEL, m)
        V = X[:, c0:c1].copy()
        C = [X[:, j * PANEL:(j + 1) * PANEL].astype(f8).T @ V.astype(f8) for j in range(q)]
        for j in range(q):
            V = (V.astype(f8) - X[:, j * PANEL:(j + 1) * PANEL].astype(f8) @ C[j]).astype(f4)
        if cond is not None:
            G = (V.astype(f8) ** 2).sum(axis=0)
            cond.append(float((cgs(V).q[G > 0] / G[G > 0]).min()))
        X[:, c0:c1], norms[c0:c1] = cgs_sweep_f32(V) if q in seq else cgs_gram_f32(V)
    return X, norms


def residual(A, X):
    """|| A X - X (X^T A X) ||_F in float64; X [p, m]."""
    A, X = np.asarray(A, dtype=f8), np.asarray(X, dtype=f8)
    AX = A @ X
    return float(np.linalg.norm(AX - X @ (X.T @ AX)))


# ---- the tolerance rule ---------------------------------------------------------------------------------------------------------

def deviation(Q, norms, ref, cols=None):
    """(d, d_norm) of a result against cgs()'s over the columns `cols` (default: all) whose reference is not zero."""
    cm = np.abs(ref.Q).max(axis=0)
    use = cm > 0
    if cols is not None:
        use &= np.isin(np.arange(cm.size), np.arange(cm.size)[cols])
    if not use.any():
        return 0.0, 0.0
    err = np.abs(np.asarray(Q, dtype=f8)[:, use] - ref.Q[:, use]).max(axis=0)
    return float((err / cm[use]).max()), float((np.abs(np.asarray(norms)[use] - ref.norms[use]) / ref.norms[use]).max())


def q_tol(ref, d):
    """Per column: the largest |Q_gpu - Q_ref| allowed in that column."""
    return 4.0 * max(d, 2.0 ** -23) * np.abs(ref.Q).max(axis=0)


def norm_rtol(d_norm=None):
    """Relative tolerance of the norms: the Gram-matrix form (d_norm None) or the sweep."""
    return U if d_norm is None else 4.0 * max(d_norm, U)


def renorm_deviation(Y32, ref):
    """d of cgs() under one more f32 rounding per entry of its input: the block scaled by 1 / 3 in f32 (a fresh rounding of every
    entry; the column scale itself leaves Q unchanged)."""
    return deviation(cgs((np.asarray(Y32, dtype=f4) / f4(3.0)).astype(f4)).Q, ref.norms, ref)[0]


# ---- test blocks ----------------------------------------------------------------------------------------------------------------

CLASSES = ("white", "graded", "zero", "dup_last", "sum_last")


def graded_exponents(m):
    return np.round(np.linspace(-20, 20, m)).astype(int)


def make_case(cls, n, m, seed):
    """float32 [n, m]; the table in the module docstring of tests/test_eigen_ref.py."""
    rng = np.random.default_rng(seed)
    if cls == "graded":
        assert 2 <= m <= n
        Uo, _ = np.linalg.qr(rng.normal(size=(n, m)))
        Vo, _ = np.linalg.qr(rng.normal(size=(m, m)))
        X = ((Uo * np.logspace(0, -3, m)) @ Vo.T).astype(f4)
        return np.ldexp(X, graded_exponents(m)[None, :]).astype(f4)
    X = rng.normal(size=(n, m)).astype(f4)
    if cls == "zero":
        X[:, m // 2] = 0.0
    elif cls == "dup_last":
        assert m >= 3
        X[:, m - 1] = X[:, 1]
    elif cls == "sum_last":
        assert m > 8
        X[:, m - 1] = X[:, 2] + X[:, 7]
    else:
        assert cls == "white"
    return X


def ld_for(m):
    ld = 32
    while ld < min(m, 256):
        ld *= 2
    return ld


# (n, m, ld): the smallest shapes that reach each kernel and each edge (the issue's tables)
SHAPES = [(13, 1, 32), (77, 5, 32), (40, 32, 32),
          (200, 33, 64), (129, 64, 64), (200, 5, 64),
          (517, 100, 128), (300, 128, 128),
          (257, 200, 256), (600, 256, 256), (200, 12, 256),
          (4225, 12, 32),            # 34 Gram chunks of 128 rows: the unrolled 32-chunk loop of k_gsf_sum and its tail
          (33000, 5, 32),            # launch_gsf_apply tiles = 3; 258 row blocks: k_gs_fin's second trip over the blocks
          (128, 12, 32), (127, 12, 32)]
STRUCT_SHAPES = [(200, 12, 32), (200, 64, 64), (300, 200, 256)]
WIDE_SHAPES = [(600, 257), (700, 300), (600, 513)]
WIDE_DUP = (600, 300)
PAD_SHAPES = [(77, 5, 32), (200, 33, 64), (517, 100, 128), (257, 200, 256)]      # one per ld


def _seed(cls, n, m, ld):
    return 1000 * CLASSES.index(cls) + 7 * n + 13 * m + ld


def cases():
    """The shared table: (cls, n, m, ld, seed) of every block the GPU tests orthonormalise (ld 0: more than 256 vectors)."""
    out = []
    for n, m, ld in SHAPES:
        out.append(("white", n, m, ld))
        if m >= 2:
            out.append(("graded", n, m, ld))
    for n, m, ld in STRUCT_SHAPES:
        out += [(cls, n, m, ld) for cls in ("zero", "dup_last", "sum_last") if not (cls == "sum_last" and m < 9)]
    out += [("white", n, m, 0) for n, m in WIDE_SHAPES]
    out.append(("dup_last",) + WIDE_DUP + (0,))
    return [c + (_seed(*c),) for c in out]


_MEMO = {}


def case(cls, n, m, ld, seed):
    """(X float32, cgs(X)) of one row of the table, computed once and left unchanged."""
    key = (cls, n, m, seed)
    if key not in _MEMO:
        X = make_case(cls, n, m, seed)
        X.setflags(write=False)
        _MEMO[key] = (X, cgs(X))
    return _MEMO[key]


def emulated(cls, n, m, ld, seed, form):
    """(d, d_norm) of a form's emulation for one row of the table ("gram", "seq", "panels", "panels_seq": GS=seq), over the columns that
    are compared (all but the last one of dup_last / sum_last), computed once."""
    key = (cls, n, m, seed, form)
    if key not in _MEMO:
        X, ref = case(cls, n, m, ld, seed)
        npan = -(-m // PANEL)
        Q, nr = {"gram": lambda: cgs_gram_f32(X), "seq": lambda: cgs_sweep_f32(X), "panels": lambda: cgs_panels(X),
                 "panels_seq": lambda: cgs_panels(X, seq=range(npan))}[form]()
        _MEMO[key] = deviation(Q, nr, ref, cols=compared(cls, m))
    return _MEMO[key]


def compared(cls, m):
    """The columns whose direction is defined: the last one of dup_last / sum_last is rounding noise."""
    return slice(0, m - 1) if cls in ("dup_last", "sum_last") else slice(0, m)


# ---- the residual's inputs ------------------------------------------------------------------------------------------------------

# (p, m): ld 32; m == ld; ld 64; m == ld, one row past a 256-row Gram chunk, odd p; one row past a reduction block; ld 128; ld 256
RESID_SHAPES = [(70, 5), (143, 32), (143, 33), (257, 64), (129, 128), (320, 100), (320, 200)]
RESID_WIDE = (588, 260)
RESID_IMAGE = (128, 64, 21)      # width, height, seed of glf.synth_image


def laplacian_case(p):
    """L_A (float64 oracle, rounded to float32: the matrix the device stores) on a sorted random sample set of exactly p pixels."""
    if ("LA", p) not in _MEMO:
        import glf
        import oracle as orc
        w, h, seed = RESID_IMAGE
        img = glf.synth_image(w, h, seed=seed)
        idx = np.sort(np.random.default_rng(p).choice(w * h, size=p, replace=False)).astype(np.uint32)
        KA, _ = orc.affinity(img, idx, want_KB=False)
        LA, _ = orc.laplacian(KA, orc.degree(img, idx))
        A32 = LA.astype(f4)
        A32.setflags(write=False)
        _MEMO[("LA", p)] = A32
    return _MEMO[("LA", p)]


# ---- the residual's bound -------------------------------------------------------------------------------------------------------

def resid_links(m, ld):
    return ld // 2 + 1 if ld <= 64 else m       # RESID_VECTOR_CHAIN


def residual_bound(A, X, ld, mode, E):
    """B [p, m] of the module docstring. A: the stored matrix, f32 bits widened, [p, p]; X: the test's X, float64 [p, m]; mode: "f16s"
    or "f32", the stored form in use; E >= |X_gpu - X| componentwise."""
    A, X = np.asarray(A, dtype=f8), np.asarray(X, dtype=f8)
    p, m = X.shape
    absA, aX = np.abs(A), np.abs(X)
    AX = A @ X
    G = X.T @ AX
    absA_aX = absA @ aX
    B_op = oref.bound(mode, oref.gamma(mode, p, ksplit=1), absA_aX, X, p, absL_rowsum=absA.sum(axis=1))
    g_G = (-(-min(p, 256) // 2) + 2) * U
    dG = g_G * (aX.T @ np.abs(AX)) + aX.T @ B_op
    B_res = (resid_links(m, ld) + 1) * U * (np.abs(AX) + aX @ np.abs(G))
    B_X = absA @ E + E @ np.abs(G) + aX @ (E.T @ absA_aX + aX.T @ (absA @ E))
    return B_op + aX @ dG + B_res + B_X


def start_block_E(V):
    """K = 0: E = 4 u |V| (one renormalisation)."""
    return 4.0 * U * np.abs(np.asarray(V, dtype=f8))


def orthonormalised_E(ref, d):
    """K >= 1: the tolerance rule, as a [p, m] matrix."""
    return np.broadcast_to(q_tol(ref, d)[None, :], ref.Q.shape)


def derived_bound(A, Y, T, its, mode):
    A, Y = np.asarray(A, dtype=f8), np.asarray(Y, dtype=f8)
    g = oref.gamma(mode, A.shape[0], ksplit=1)
    return 2.0 * its * (g + 4.0 * U) * float(np.linalg.norm(np.abs(A) @ np.abs(Y) @ np.abs(T)))


def residual_f32(A32, X32):
    """A plain numpy float32 evaluation of the residual (f32 products and sums in numpy's order)."""
    A32, X32 = np.asarray(A32, dtype=f4), np.asarray(X32, dtype=f4)
    AX = A32 @ X32
    R = AX - X32 @ (X32.T @ AX)
    return float(np.sqrt((R.astype(f8) ** 2).sum()))


# ---- the record behind profiles/eigen_blocks_error.json -------------------------------------------------------------------------

RECORD = {}


def record(family, mode, label, err, tol, d=None):
    """Keep the worst error / tolerance of a family (e.g. "gram ld 64", "sweep residual") under a contraction mode."""
    ratio = float(err) / float(tol) if tol > 0 else (0.0 if err == 0 else float("inf"))
    r = RECORD.get((family, mode))
    if r is None or ratio > r["ratio"]:
        RECORD[(family, mode)] = dict(family=family, contraction=mode, worst_case=label, error=float(err), tolerance=float(tol),
                                      ratio=ratio, d=None if d is None else float(d))
    return ratio


def dump(path):
    what = ("largest measured error per family and contraction mode over the cases of tests/test_gpu_orthonormalise.py and "
            "tests/test_gpu_residual.py on an MI355X (python tools/eigen_blocks_error.py), the tolerance or bound it is asserted "
            "against (tests/eigen_ref.py), their ratio, and the emulation's d of the worst case. A record only.")
    with open(path, "w") as f:
        json.dump(dict(what=what, rows=[RECORD[k] for k in sorted(RECORD)]), f, indent=1)
