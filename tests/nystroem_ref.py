"""The error bound of the Nystroem extension Phi_B = K_B^T Psi, Psi = s (phi_A Pi^-1), per form, the test blocks (phi_A, Pi^-1), and a numpy
emulation of the direct split-f16 kernel. Shared by tests/test_nystroem_bound.py (CPU) and tests/test_gpu_nystroem.py. The twin of
tests/operator_ref.py, whose U, V, round_up, grid_shape and model of an MFMA instruction it takes over.

Reference, float64: Psi = s (phi_A pinv) formed exactly from the f32 inputs (s = the f32 L_B.scale widened), Phi_ref[x, :] = sum_i
K(x, s_i) Psi[i, :] for the non-sample pixels x in raster order (the rows p .. N of the sample-first Phi), K from the kernel's definition
in chunks of image rows (K_B is never held whole); the sample rows are phi_A's bits.
Bound, componentwise:  |Phi - Phi_ref|_xj <= gamma (K_B^T |Psi|)_xj + a_xj,  gamma = (K + c) u + s v,  u = 2^-24, v = 2^-22 (operator_ref).

K counts the links of the longest f32 accumulation chain of one output, one link per MFMA instruction and per explicit f32 add.
c counts the roundings an entry of K and of Psi carries before it is contracted: 2 for k_make_psi's two multiplies (pipeline.hip:58,
scale * (phiA * pinv)), plus the form's entry generation (below). p64 = round_up(p, 64), ks = ceil(nr / 16), ksc = ceil(nc / 16).

form        K (links)                  s   c    where (csrc/, line numbers as of this commit)
f32         p64 / 2 + 1                0   316  k_nystroem<MB, PB> (any MB, PB: a pixel block and a column block have their own
                                                accumulator): nystroem.hip:204, one mfma_f32_32x32x2f32 per two samples (one of each half
                                                of the 64-sample chunk, :183-187) over p64 / 64 chunks (:180); +1: the products are
                                                rounded f32. c = 2 + 2 (v_exp_f32, 1 ulp = 2 u) + 3 x 104: the exponent t = fmaf(dv^2,
                                                s_val, q s_loc) (:196-197) carries the rounding of s_loc / s_val to f32 (make_coef), of
                                                q s_loc and of the fmaf (q = dr^2 + dc^2 and dv^2 are exact integers), each amplified by
                                                t ln 2 <= 150 ln 2 < 104: beyond t = 150 the entry is below 2^-150 (the floor below).
                                                gamma is above 2^-16 for this chain: the amplification of the exponent's roundings.
pix f32     p64 / 2 + 1                0   316 + 104 n   the same kernel, GEN != Grey: dist2 (glf_internal.hpp:331, 374-377, 410-413)
                                                adds n roundings to the exponent: rgb8 0 (integers below 2^18), u16 1 (the square of a
                                                16-bit difference), f32 3 (difference, twice in its square, the square), rgbf32 5 (as the
                                                comment at :389-391 counts)
f16s        12 p64 / 64                3   120  k_nystroem_f16s<.., LUT = false>: nystroem.hip:688-690, 4 steps (:624) x 3 MFMAs per chunk
                                                (:607); s: K' = 2^15 K split (:667-676), Psi split (k_psi_split_f16, :396-398), lo x lo;
                                                c = 2 + 2 (v_exp_f32) + 4 x 29: s, q s_loc, the fmaf and 15 - t (:663-664), amplified by
                                                |15 - t| ln 2 <= 40.5 ln 2 < 29 (t > 40.5: 2^15 K < 2^-25, a zero pair, the floor below)
f16s lut    12 p64 / 64                3   36   LUT = true: K' = (Er Ec) P (:660), tables rounded once from f64 (:801-805): 3 + 2
                                                multiplies, + 29 for s_loc and s_val rounded to f32 (t ln 2 u on an entry 2^-t), + 2
grid        3 ks + 3 ksc               6   23   operator_ref's grid row with the Nystroem passes' kernels: row pass k_grid_rowpass
                                                (ROWPASS=v1, nystroem_grid.inc:247-249) or the row-tile form (rt, :522), column pass
                                                k_grid_colpass (:860-862); c = 17 + 3 (entries, operator_ref) + 1 (y = Er X, :220) + 2; no
                                                epilogue roundings (the output scale osc, :888, is a power of two)
rank        3 ks + 3 R / 16 + 3 ksc    9   24   operator_ref's rank row (k_rank_colpass, COLPASS ws nystroem_rank.inc:450-495 / v1
                                                :825-888): + 1 for the factor table. The order in which the column pass accumulates T'
                                                over its segments was not traced instruction by instruction: K counts its MFMAs per output.
band        3 nr ksc                   3   24   k_band (nystroem_band.inc:485-487): 17 + 3 + 2 (y = (era ec) pp, :457-458) + 2; the chain of
                                                one pixel runs over the grid rows of its band and the 16-column blocks of its window, at
                                                most all nr ksc of them. Its schedule (row pairs per half-block) was not traced
                                                instruction by instruction: K counts the MFMAs per output.
pix band    3 nr ksc                   3   130  the same with P = v_exp_f32(dist2 * -s_val) per entry: operator_ref's 132 - 4 + 2

a_xj, the parts the forms drop by design (colmax_j = max_i |Psi_ij|, col1_j = sum_i |Psi_ij|, rowsum_x = sum_i K(x, s_i)):
f32, pix f32  2^-126 col1_j + p 2^-148 [col1_j > 0]: an entry below the normal range (t > 126) is a denormal or flushed, 2^-126 absolutely
              at most; a product below the normal range likewise (2^-149 per term)
f16s          2^-40 col1_j + 2^-38 colmax_j rowsum_x: an f16 (hi, lo) pair cannot hold less than 2^-25: of K' = 2^15 K that is 2^-40 of K
              (what exact-zero skipping and the window rely on), of Psi scaled into [2^13, 2^14) it is 2^-38 colmax
grid, band    p 2^-36 colmax_j (operator_ref's floor with alpha = 1: K <= 1, and s is folded into Psi); the band's and the window's
              samples beyond the radius are entries with 2^15 K below the pair's floor
rank          p 2^-25 colmax_j + 2^-30 (K_sp^T |Psi|)_xj, and its gamma term is taken against K_sp, the spatial factor of the kernel
              alone: its roundings are relative to sum_k |f_k(v) f_k(w)| <= 1, not to P(|v - w|) (operator_ref)
These numbers are derived from the code, not measured; profiles/nystroem_error.json records how far below them the kernels stay."""
import numpy as np

import u16_ref
from operator_ref import U, V, round_up, grid_shape  # noqa: F401  (grid_shape: re-exported for the tests)

PIX_EXPONENT_ROUNDINGS = {"rgb8": 0, "u16": 1, "f32": 3, "rgbf32": 5}

# the shapes of tests/test_gpu_nystroem.py: grey u8 glf.synth_image(w, h, seed), glf.Sampling(w, h, samples); p = nr x nc as realised
#           w    h    samples seed h_loc  p    nr  nc
SHAPES = {
    "tiny":   (53,  37,  20,  3, 40.0, 24,  4,  6),    # one partial chunk; N = 1961 no multiple of a workgroup's pixels; w % 64 != 0: no LUT
    "lut":    (128, 45,  120, 4, 40.0, 147, 7,  21),   # w % 64 == 0: the LUT kernel at ld 32 / 64; ragged last chunk (19); nc no multiple of 16
    "edge":   (60,  58,  120, 5, 40.0, 132, 11, 12),   # p % 64 = 4
    "mid":    (192, 64,  300, 6, 40.0, 320, 10, 32),   # whole chunks, several
    "big":    (256, 144, 700, 7, 40.0, 720, 20, 36),   # two row k-steps, three column k-steps, twelve chunks
    "narrow": (192, 160, 400, 8, 5.0,  480, 20, 24),   # radius 27 px (split f16) / 52 px (f32) against a 160 px side: a partial band, real windows
}
H_VAL = 30.0
LDS = {"big": (64, 256)}                # (the widths a shape runs at; default: all four)
ALL_LDS = (32, 64, 128, 256)


def lut_runs(shape, ld, no_lut=False):
    """launch_nystroem_f16s' rule (nystroem.hip:785-788): MB <= 2, every wave's 64 pixels in one image row, the table short enough."""
    w, h_loc = SHAPES[shape][0], SHAPES[shape][4]
    lut_r = int(np.floor(np.sqrt(150.5 / (np.log2(np.e) / h_loc ** 2)))) + 1
    return ld <= 64 and w % 64 == 0 and lut_r <= 511 and not no_lut


def bound_forms(shape):
    """Every (form of the bound, ld) the GPU test holds a kernel to at this shape."""
    out = []
    for ld in LDS.get(shape, ALL_LDS):
        out += [("f32", ld), ("f16s", ld), ("grid", ld), ("rank", ld), ("band", ld)]
        if lut_runs(shape, ld):
            out.append(("f16s_lut", ld))
    return out


def counts(form, p, nr=0, nc=0, R=64, fmt=None):
    """(K, s, c) of the table above. form: f32, pix_f32 (fmt names the pixel format), f16s, f16s_lut, grid, rank, band, pix_band."""
    p64 = round_up(p, 64)
    ks, ksc = -(-nr // 16), -(-nc // 16)
    if form == "f32":
        return p64 // 2 + 1, 0, 316
    if form == "pix_f32":
        return p64 // 2 + 1, 0, 316 + 104 * PIX_EXPONENT_ROUNDINGS[fmt]
    if form == "f16s":
        return 12 * (p64 // 64), 3, 120
    if form == "f16s_lut":
        return 12 * (p64 // 64), 3, 36
    if form == "grid":
        return 3 * ks + 3 * ksc, 6, 23
    if form == "rank":
        return 3 * ks + 3 * (R // 16) + 3 * ksc, 9, 24
    if form == "band":
        return 3 * nr * ksc, 3, 24
    if form == "pix_band":
        return 3 * nr * ksc, 3, 130
    raise ValueError(form)


def gamma(form, p, **kw):
    K, s, c = counts(form, p, **kw)
    return (K + c) * U + s * V


def psi64(phi_A, pinv, s):
    """Psi = s (phi_A pinv) exactly (the products of two f32 values are exact in f64; the third factor rounds at 2^-53)."""
    return float(np.float32(s)) * (phi_A.astype(np.float64) * pinv.astype(np.float64)[None, :])


def psi32(phi_A, pinv, s):
    """Psi as k_make_psi rounds it: scale * (phiA * pinv), f32."""
    return (np.float32(s) * (phi_A.astype(np.float32) * pinv.astype(np.float32)[None, :])).astype(np.float32)


class Reference:
    """What the bound needs of one (guide, sample set, Psi), for the non-sample pixels of the image rows [row0, row1) in raster order:
    phi = K_B^T Psi, kabs = K_B^T |Psi|, ksp = K_sp^T |Psi| (the spatial factor alone), rowsum[x] = sum_i K(x, s_i); pixels: their
    raster indices; first: the sample-first row of the first of them."""


def reference(img, idx, Psi, h_loc, h_val, kern=u16_ref.kernel, rows=None, chunk_rows=16):
    h, w = img.shape[:2]
    idx = np.asarray(idx, dtype=np.int64)
    p = idx.size
    row0, row1 = (0, h) if rows is None else rows
    mask = np.zeros(h * w, dtype=bool)
    mask[idx] = True
    aP = np.abs(Psi)
    flat = np.zeros((h, w))                                         # (the spatial factor alone: the kernel of a constant image)
    out = Reference()
    parts = dict(phi=[], kabs=[], ksp=[], rowsum=[], pixels=[])
    for r0 in range(row0, row1, chunk_rows):
        px = np.arange(r0 * w, min(row1, r0 + chunk_rows) * w, dtype=np.int64)
        px = px[~mask[px]]
        if not px.size:
            continue
        K = kern(img, px, idx, h_loc, h_val)                       # [pixels, p]
        Ksp = u16_ref.kernel(flat, px, idx, h_loc, 1.0)
        parts["phi"].append(K @ Psi)
        parts["kabs"].append(K @ aP)
        parts["ksp"].append(Ksp @ aP)
        parts["rowsum"].append(K.sum(axis=1))
        parts["pixels"].append(px)
    for k, v in parts.items():
        setattr(out, k, np.concatenate(v))
    out.first = p + int(row0 * w - np.count_nonzero(idx < row0 * w))
    out.p = p
    return out


def bound(form, g, ref, Psi, cols=None):
    """gamma (K_B^T |Psi|) + a for the pixels of `ref` and the columns `cols` (a slice; None: all) of Psi (float64 [p, ld])."""
    cols = slice(None) if cols is None else cols
    aP = np.abs(Psi[:, cols])
    p = aP.shape[0]
    colmax, col1 = aP.max(axis=0), aP.sum(axis=0)
    if form in ("f32", "pix_f32"):
        return g * ref.kabs[:, cols] + 2.0 ** -126 * col1[None, :] + p * 2.0 ** -148 * (col1 > 0)[None, :]
    if form in ("f16s", "f16s_lut"):
        return g * ref.kabs[:, cols] + 2.0 ** -40 * col1[None, :] + 2.0 ** -38 * ref.rowsum[:, None] * colmax[None, :]
    if form in ("grid", "band", "pix_band"):
        return g * ref.kabs[:, cols] + p * 2.0 ** -36 * colmax[None, :]
    if form == "rank":
        return g * ref.ksp[:, cols] + p * 2.0 ** -25 * colmax[None, :] + 2.0 ** -30 * ref.ksp[:, cols]
    raise ValueError(form)


def check(Phi_B, Phi_ref, B):
    """(worst ratio |Phi - Phi_ref| / B where B > 0, every element within the bound and exactly zero where B = 0)."""
    err = np.abs(Phi_B.astype(np.float64) - Phi_ref)
    pos = B > 0
    ratio = float((err[pos] / B[pos]).max()) if pos.any() else 0.0
    return ratio, bool((err <= B).all() and not Phi_B[~pos].any())


# ---- the test block -------------------------------------------------------------------------------------------------------------------

FULL_LD = 256
COL_ZERO, COL_EVEN_ZERO, COL_UNIT0 = 1, 2, 3


def unit_samples(p):
    """The samples of the unit-vector columns (columns COL_UNIT0 ..): 0, 63, 64, p // 2, p - 1, as far as they exist and are distinct:
    the grid's corners, the chunk boundary, the middle, the ragged last chunk."""
    out = []
    for i in (0, 63, 64, p // 2, p - 1):
        if 0 <= i < p and i not in out:
            out.append(i)
    return out


def _full_block(p, seed):
    rng = np.random.default_rng(seed)
    m = FULL_LD - 5
    e = np.round(np.linspace(-30, 30, m)).astype(int)
    rng.shuffle(e)
    phi_A = np.zeros((p, FULL_LD), dtype=np.float32)
    phi_A[:, :m] = (rng.normal(size=(p, m)) * 2.0 ** e[None, :]).astype(np.float32)
    phi_A[:, COL_ZERO] = 0.0
    phi_A[0::2, COL_EVEN_ZERO] = 0.0
    for k, i in enumerate(unit_samples(p)):
        phi_A[:, COL_UNIT0 + k] = 0.0
        phi_A[i, COL_UNIT0 + k] = 1.0
    pinv = np.zeros(FULL_LD, dtype=np.float32)
    pinv[:m] = rng.uniform(0.5, 2.0, size=m).astype(np.float32)
    pinv[0:m:2] = np.ldexp(np.float32(1), rng.integers(-3, 4, size=len(range(0, m, 2)))).astype(np.float32)
    return phi_A, pinv


_BLOCKS = {}


def make_block(p, ld, m, seed):
    """(phi_A float32 [p, ld], pinv float32 [m]): the leading columns of one block of 256 columns per (p, seed), so that a shape's
    reference is computed once at 256 columns and serves every narrower ld. Normal columns scaled by 2^e, e spread over -30 .. +30 in
    shuffled order; column 1 all zero; column 2 zero on the even samples; columns 3 .. unit vectors at unit_samples(p): each reads one
    row of K_B entry by entry at every pixel; pinv: powers of two (2^-3 .. 2^3) on the even columns, values in (0.5, 2) on the odd ones;
    the columns from m on are zero."""
    assert COL_UNIT0 + 5 <= m <= ld <= FULL_LD and m <= FULL_LD - 5
    if (p, seed) not in _BLOCKS:
        _BLOCKS[(p, seed)] = _full_block(p, seed)
    phi_A, pinv = _BLOCKS[(p, seed)]
    out = phi_A[:, :ld].copy()
    out[:, m:] = 0.0
    return out, pinv[:m].copy()


# ---- numpy emulation of the direct split-f16 kernel (k_make_psi's Psi, launch_nystroem_f16s' scales, k_psi_split_f16, k_nystroem_f16s) --

def _split(v32):
    hi = v32.astype(np.float16)
    lo = (v32 - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


DEFECTS = ("drop_lo_hi", "drop_last_chunk", "column_off_by_one", "band_row_short", "rounded_inverse_scale")


def emulate_direct_f16s(K, Psi, defect=None, grid=None, width=None, pixels=None, sample=None, column=None):
    """Phi_B = K Psi as the kernel computes it. K: float64 [pixels, p], the exact entries (rounded to f32 once as K' = 2^15 K: the
    generation's own roundings are not modelled); Psi: float32 [p, ld] (psi32). Column scales 2^e with |Psi| 2^e in [2^13, 2^14) and
    the exact inverse 2^(-e - 15) (launch_nystroem_f16s), hi / lo splits of K' and of the scaled Psi, per 64-sample chunk four steps
    of 16 samples with three products each (hi hi, hi lo, lo hi), one MFMA = the exact sum of its 16 products added to the f32
    accumulator with one rounding, chunks in ascending order.
    defect: one of DEFECTS --
      drop_lo_hi             the K-lo x Psi-hi product left out
      drop_last_chunk        the last (on most shapes ragged) 64-sample chunk left out
      column_off_by_one      the entries of sample `sample` taken at the next pixel of the list (a column index off by one)
      band_row_short         per pixel, the grid row of samples farthest from the pixel's image row dropped (a band one row too short);
                             grid = (nr, nc, sample image rows [p]), width, pixels (raster indices) say which
      rounded_inverse_scale  on column `column` the inverse scale's exponent from round(log2(max)) instead of the exact floor: where
                             the two differ the column comes back one binade off"""
    npx, p = K.shape
    ld = Psi.shape[1]
    assert defect is None or defect in DEFECTS
    p64 = round_up(p, 64)
    mx = np.abs(Psi).max(axis=0)
    ex = np.zeros(ld, dtype=int)
    ok = (mx > 0) & np.isfinite(mx)
    ex[ok] = 14 - np.frexp(mx[ok])[1]                       # frexp: mx = f 2^e, f in [0.5, 1)
    ex = np.clip(ex, -100, 100)
    scale = np.ldexp(np.float32(1), ex).astype(np.float32)
    inv_ex = -ex - 15
    if defect == "rounded_inverse_scale":
        assert ok[column]
        inv_ex = inv_ex.copy()
        inv_ex[column] = -(13 - int(np.rint(np.log2(float(mx[column]))))) - 15
    inv = np.ldexp(np.float32(1), inv_ex).astype(np.float32)
    Pp = np.zeros((p64, ld), dtype=np.float32)
    Pp[:p] = Psi * scale[None, :]
    bh, bl = _split(Pp)
    K = K.copy()
    if defect == "column_off_by_one":
        K[:-1, sample] = K[1:, sample]
    if defect == "band_row_short":
        nr, nc, srow = grid
        prow = np.asarray(pixels) // width
        grows = np.unique(srow)
        far = grows[np.abs(prow[:, None] - grows[None, :]).argmax(axis=1)]      # [pixels]: the farthest grid row's image row
        K[srow[None, :] == far[:, None]] = 0.0
    Kp = np.zeros((npx, p64), dtype=np.float32)
    Kp[:, :p] = (K * 32768.0).astype(np.float32)
    ah, al = _split(Kp)
    f8 = np.float64
    nchunks = p64 // 64
    if defect == "drop_last_chunk":
        nchunks -= 1
    acc = np.zeros((npx, ld), dtype=np.float32)
    for ch in range(nchunks):
        for t in range(4):
            k = slice(ch * 64 + 16 * t, ch * 64 + 16 * t + 16)
            prods = [(ah, bh), (ah, bl)] + ([] if defect == "drop_lo_hi" else [(al, bh)])
            for a, b in prods:
                acc = (acc.astype(f8) + a[:, k].astype(f8) @ b[k, :].astype(f8)).astype(np.float32)
    return acc * inv[None, :]
