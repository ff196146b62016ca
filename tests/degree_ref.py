"""The float64 reference and the error bound of the degree stage D_A = rowsum [K_A K_B] (glf_Degree_ex) per form, the grid shapes of the
tests with the launch plan the host derives for each, and a numpy emulation of the grid-factored form. Shared by
tests/test_degree_bound.py (CPU) and tests/test_gpu_degree.py. U, V and the model of an MFMA instruction (one link of the f32 chain
per instruction) are tests/operator_ref.py's.

Reference, float64, over the image rows [row0, row1), K from the kernel's definition (u16_ref.kernel / rgb_ref.kernel; NLM: the oracle):
  D_ref[i] = sum K(s_i, px)   Uy_ref[i] = sum K(s_i, px) y[px]   Us_ref[i] = sum K(s_i, px) s[px]   Uabs[i] = sum K(s_i, px) |s[px]|
Bound, per sample:  |D - D_ref| <= gamma D_ref + a,  |Uy - Uy_ref| <= gamma Uy_ref + 255 a,  |Us - Us_ref| <= gamma Uabs + max|s| a,
gamma = (K + c) u + s v,  u = 2^-24, v = 2^-22.

K counts the links of the longest f32 chain a term runs through, c the roundings a term carries before it enters the chain, s the
split-f16 operand roundings (v each). npix = (row1 - row0) width. Line numbers as of this commit (csrc/).

form       K                        s  c          where
direct     12                       0  39         k_degree / k_degree_win, degree_chunk_lut (affinity.hip:170-225): a strip's row is one
                                                  product and three fmas (:209-212), the strip accumulator one fma per row over the 8
                                                  rows of a half (:213), f64 from :216 on: 4 + 8. c: P correctly rounded from f64 (1,
                                                  :253) of an exponent whose s_val is an f32 (make_coef, ctx.hip:487): t_P ln 2 u; Er
                                                  and Ec (:181, :201) are v_exp_f32 (1 ulp = 2 u each) of -(d^2 s_loc), d^2 exact, the
                                                  product rounded and s_loc an f32: 2 t_r ln 2 u and 2 t_c ln 2 u. Together at most
                                                  2 t ln 2 u on an entry 2^-t: 34 u for t <= 24; beyond, the entry is below 2^-24 and
                                                  moves by at most 2 t 2^-t ln 2 u < 2^-43 absolutely (the floor). 34 + 1 + 2 + 2.
grid       min(w, 2 r - 1) + 96     3  20 (21)    k_dgrid_hist (affinity_grid.inc:88-94): a bin of Wt is a chain of f32 additions in
                                                  ascending column order, one per pixel of that value within reach of the column -- at
                                                  most min(width, 2 radius - 1), radius the first exact zero of the f32 table (no zero
                                                  in the table: width); weighted (:82-85, one fmaf per pixel): one more rounding per
                                                  term, c = 21. k_dgrid_zmfma (:240-242): 3 MFMAs per k-step, DGZ_CHUNK / 16 = 32
                                                  k-steps per f32 chunk sum; the scales (:220, :264) are powers of two; f64 over chunks
                                                  and values (k_dgrid_final_parts, :296-301). s: the split of 2^15 Er (k_dgrid_erfrag,
                                                  :138-141), of 2^wsh Wt (:219-230), and lo x lo. c: the tables P, Er, Ec are rounded
                                                  once from f64 (grid_common.inc:188-189; 3) of exponents whose s is an f32: t ln 2 u,
                                                  17 u for t <= 24, below 2^-44 absolutely beyond (operator_ref's entries).
pix        64                       0  2 + 104 (3 + n)   k_degree_entrywise<G> (entrywise.hip:91-103): acc += v_exp_f32(..) over the 64
                                                  pixels of a tile row, f64 from :103. The exponent fmaf(u, s_val, fmaf(dc, dc, qr) *
                                                  s_loc) (:101) carries the coefficients' rounding, the product's and the fmaf's (3) and
                                                  dist2's n = nystroem_ref.PIX_EXPONENT_ROUNDINGS[format], each amplified by t ln 2 <=
                                                  150 ln 2 < 104 (t > 150: the entry is below 2^-150, the floor).
nlm        64                       0  nlm_c(h_val)   k_nlm_degree (nlm.hip:138-140): acc += v_exp_f32(-(d s_val)) over a tile of 64 pixels.
                                                  d = sum_k (f_k - g_k)^2 (nlm_dist, :98-113): features f = G_k x pixel (G an f32, the
                                                  product rounded: 2 u |f|), the difference rounded (u), 49 fmas in two chains and two
                                                  adds (27 links): with sum_k G_k^2 < 0.056 (sigma 1.2) the differences carry an absolute
                                                  error of at most 4 u 255 sqrt(0.056) < 242 u in the 2-norm, so the exponent tau =
                                                  s_val d moves by at most 2 sqrt(tau s_val) 242 u + (27 + 2) u tau (s_val's rounding, the
                                                  product's). nlm_c = ceil(ln 2 (484 sqrt(24 s_val) + 29 x 24)) + 2 for tau <= 24; beyond,
                                                  the entry is below 2^-24: the same expression at tau = 150 times 2^-24 u, the floor.

a, the parts the forms drop by design:
direct     npix 2^-43 (entries beyond t = 24, above) + npix 2^-125 (a factor or a product below the f32 normal range)
grid       npix 2^-44 (entries beyond t = 24) + the pair floors: 2^15 Er below 2^-25 is a zero (hi, lo) pair, and a lo half below the
           f16 normal range is exact to 2^-25 only -- 2^-40 of Er, against at most sum_r sum_v Wt <= nrows wmax per sample (P <= 1,
           wmax = 1 + 2 sum_d Ec(d) the table's mass the host sizes the scale by, :349-353): 2^-40 nrows wmax; 2^wsh Wt likewise,
           2^-25-wsh <= 2^-38 wmax of Wt, against sum_r Er <= min(nrows, wmax_r) and sum_v P(|v_i - v|) <= pmass = 1 + 2 sum_e P(e):
           2^-38 wmax min(nrows, emass) pmass. Weighted: both times max |s| (the host's wmax carries it, :354).
pix, nlm   npix 2^-125; nlm: + npix 2^-24 u (the expression above at tau = 150)
These numbers are derived from the code, not measured; profiles/degree_error.json records how far below them the kernels stay."""
import bisect
import math

import numpy as np

import u16_ref
from nystroem_ref import PIX_EXPONENT_ROUNDINGS
from operator_ref import U, V, round_up

LOG2E = 1.4426950408889634
DGZ_CHUNK, DGZ_MG, ZWIN = 512, 5, 4
FIVES, TEN, WINDOW = 0, 1, 2                     # glf_degree_info.shape
DENSE, GRID, WINDOWED, ENTRYWISE, NLM = 0, 1, 2, 5, 6   # glf_degree_info.path
H_VAL = 30.0


def s_f32(h):
    """make_coef: log2(e) / h^2 rounded to f32."""
    return np.float32(LOG2E / (float(h) * float(h)))


def etab32(h_loc, n):
    """The spatial factor table as the host builds it: exp2(-s_loc d^2) correctly rounded from f64, s_loc an f32."""
    d = np.arange(n, dtype=np.float64)
    return np.exp2(-float(s_f32(h_loc)) * d * d).astype(np.float32)


def ptab32(h_val):
    e = np.arange(256, dtype=np.float64)
    return np.exp2(-float(s_f32(h_val)) * e * e).astype(np.float32)


def zero_radius(h_loc, maxdim):
    """First distance at which the f32 spatial factor is exactly 0 (GridTables::build); maxdim where there is none."""
    z = np.nonzero(etab32(h_loc, maxdim) == 0)[0]
    return int(z[0]) if z.size else maxdim


def wmax_of(h_loc, width):
    """The table mass the host sizes the f16 scale of Wt by (affinity_grid.inc:349-353)."""
    d = np.arange(1, width, dtype=np.float64)
    return 1.0 + 2.0 * float(np.exp2(-float(s_f32(h_loc)) * d * d).sum())


def grid_plan(w, h, rows, cols, h_loc, row0=0, row1=None, zmfma_groups=False):
    """What degree_rows_grid decides for a sample grid (affinity_grid.inc:359-379): dict(nr, nc, ncp, radius, shape, chunks, mgroups,
    mtiles, mt0 (window: the first m-tile of every chunk))."""
    row1 = h if row1 is None else row1
    rows, cols = [int(r) for r in rows], [int(c) for c in cols]
    nr, nc = len(rows), len(cols)
    maxdim = max(w, h)
    radius = zero_radius(h_loc, maxdim)
    nrows = row1 - row0
    mtiles, nchunks = -(-nr // 32), -(-nrows // DGZ_CHUNK)
    window, mt0 = radius < maxdim and not zmfma_groups, []
    for c in range(nchunks):
        if not window:
            break
        r_lo, r_hi = row0 + c * DGZ_CHUNK - (radius - 1), row0 + (c + 1) * DGZ_CHUNK - 1 + (radius - 1)
        a_lo, a_hi = bisect.bisect_left(rows, r_lo), bisect.bisect_right(rows, r_hi) - 1
        mt0.append(a_lo // 32 if a_hi >= a_lo else 0)
        if a_hi >= a_lo and a_hi // 32 - a_lo // 32 + 1 > ZWIN:
            window = False
    one = not window and DGZ_MG < mtiles <= 2 * DGZ_MG and not zmfma_groups
    mg = ZWIN if window else 2 * DGZ_MG if one else DGZ_MG
    return dict(nr=nr, nc=nc, ncp=round_up(nc, 4), radius=radius, shape=WINDOW if window else TEN if one else FIVES, chunks=nchunks,
                mgroups=1 if window else -(-mtiles // mg), mtiles=mtiles, mt0=mt0 if window else None)


# The grid shapes of tests/test_gpu_degree.py (8-bit grey, DEG_PATH=grid): name -> (w, h, grid rows, grid columns, h_loc); "sampling":
# the rows and columns of glf.Sampling(w, h, 20), filled in by the tests (4 x 6).
def _shapes():
    ev = lambda n, step=1, first=0: list(range(first, first + n * step, step))   # noqa: E731
    return {
        "fives":          (53, 37, None, None, 40.0),                            # glf.Sampling(53, 37, 20): 4 x 6
        "ten":            (12, 400, ev(200, 2), [1, 5, 10], 40.0),
        "three_groups":   (12, 700, ev(350, 2), [1, 5, 10], 80.0),
        "window_1":       (96, 80, ev(8, 10, 3), ev(10, 9, 5), 5.0),
        "window_3":       (16, 1100, ev(184, 6), [1, 6, 10, 15], 5.0),
        "window_refused": (16, 1100, ev(275, 4), [1, 6, 10, 15], 5.0),
        "wide_5":         (150, 24, [5, 17], ev(70, 2, 3), 5.0),
        "wide_40":        (150, 24, [5, 17], ev(70, 2, 3), 40.0),
    }


SHAPES = _shapes()
FIVES_GRID = ([4, 13, 22, 31], [4, 13, 22, 31, 40, 49])   # what glf.Sampling(53, 37, 20) realises (asserted by the tests)
# name -> the realised (p, nr, nc, radius, shape, chunks, mgroups) over all rows; test_degree_bound.py derives each from grid_plan
TABLE = {
    "fives":          (24, 4, 6, 53, FIVES, 1, 1),
    "ten":            (600, 200, 3, 400, TEN, 1, 1),
    "three_groups":   (1050, 350, 3, 700, FIVES, 2, 3),
    "window_1":       (80, 8, 10, 51, WINDOW, 1, 1),
    "window_3":       (736, 184, 4, 51, WINDOW, 3, 1),
    "window_refused": (1100, 275, 4, 51, TEN, 3, 1),
    "wide_5":         (140, 2, 70, 51, WINDOW, 1, 1),
    "wide_40":        (140, 2, 70, 150, FIVES, 1, 1),
}


def shape(name):
    """(w, h, rows, cols, h_loc, idx uint32 [p]) of a grid shape."""
    w, h, rows, cols, h_loc = SHAPES[name]
    if rows is None:
        rows, cols = FIVES_GRID
    idx = (np.asarray(rows, dtype=np.int64)[:, None] * w + np.asarray(cols, dtype=np.int64)[None, :]).reshape(-1).astype(np.uint32)
    return w, h, list(rows), list(cols), h_loc, idx


# ---- the bound ------------------------------------------------------------------------------------------------------------------------

def nlm_c(h_val, tau=24.0):
    s_val = LOG2E / (float(h_val) ** 2)
    return int(math.ceil(math.log(2.0) * (484.0 * math.sqrt(tau * s_val) + 29.0 * tau))) + 2


def counts(form, width=0, radius=0, weighted=False, fmt=None, h_val=None):
    """(K, s, c) of the table above. form: direct, grid, pix (fmt names the pixel format), nlm."""
    if form == "direct":
        return 12, 0, 39
    if form == "grid":
        return min(width, 2 * radius - 1) + 96, 3, 21 if weighted else 20
    if form == "pix":
        return 64, 0, 2 + 104 * (3 + PIX_EXPONENT_ROUNDINGS[fmt])
    if form == "nlm":
        return 64, 0, nlm_c(h_val)
    raise ValueError(form)


def gamma(form, **kw):
    K, s, c = counts(form, **kw)
    return (K + c) * U + s * V


def floor(form, width, nrows, h_loc=None, h_val=None):
    """a of the table above for D (Uy: times 255; Us: times max |s|)."""
    npix = float(width) * nrows
    if form == "direct":
        return npix * (2.0 ** -43 + 2.0 ** -125)
    if form == "grid":
        wm = wmax_of(h_loc, width)
        emass = wmax_of(h_loc, 1 << 14)
        e = np.arange(1, 256, dtype=np.float64)
        pmass = 1.0 + 2.0 * float(np.exp2(-float(s_f32(h_val)) * e * e).sum())
        return npix * 2.0 ** -44 + 2.0 ** -40 * nrows * wm + 2.0 ** -38 * wm * min(float(nrows), emass) * pmass
    if form == "pix":
        return npix * 2.0 ** -125
    if form == "nlm":
        return npix * (2.0 ** -125 + nlm_c(h_val, 150.0) * 2.0 ** -24 * U)
    raise ValueError(form)


class Reference:
    """D, Uy, Us, Uabs (float64 [p]) of one (guide, sample set, row range, plane); pairs: the (sample, pixel) pairs whose entry is at
    least 2^-126; smax = max |s| over the rows."""


def reference(img, idx, h_loc, h_val, rows=None, kern=u16_ref.kernel, plane=None, chunk_rows=32):
    h, w = img.shape[:2]
    idx = np.asarray(idx, dtype=np.int64)
    row0, row1 = (0, h) if rows is None else rows
    out = Reference()
    out.D, out.Uy, out.Us, out.Uabs, out.pairs = np.zeros(idx.size), np.zeros(idx.size), np.zeros(idx.size), np.zeros(idx.size), 0
    y = img.reshape(-1).astype(np.float64) if img.ndim == 2 else None
    s = None if plane is None else np.asarray(plane, dtype=np.float32).reshape(-1).astype(np.float64)
    for r0 in range(row0, row1, chunk_rows):
        px = np.arange(r0 * w, min(row1, r0 + chunk_rows) * w, dtype=np.int64)
        K = kern(img, idx, px, h_loc, h_val)                       # [p, pixels]
        out.D += K.sum(axis=1)
        out.pairs += int(np.count_nonzero(K >= 2.0 ** -126))
        if y is not None:
            out.Uy += K @ y[px]
        if s is not None:
            out.Us += K @ s[px]
            out.Uabs += K @ np.abs(s[px])
    out.smax = 0.0 if s is None else float(np.abs(s[row0 * w:row1 * w]).max())
    out.rows, out.width = (row0, row1), w
    return out


def bounds(form, ref, h_loc=None, h_val=None, **kw):
    """(gamma, B_D, B_Uy, B_Us) for the samples of `ref`; kw: counts' (width / radius / fmt). B_Us: the weighted form's gamma."""
    nrows = ref.rows[1] - ref.rows[0]
    a = floor(form, ref.width, nrows, h_loc=h_loc, h_val=h_val)
    g = gamma(form, h_val=h_val, **kw) if form == "nlm" else gamma(form, **kw)
    gw = gamma(form, weighted=True, **kw) if form == "grid" else g
    return g, g * ref.D + a, g * ref.Uy + 255.0 * a, gw * ref.Uabs + ref.smax * a


def check(x, x_ref, B):
    """(worst |x - x_ref| / B, every sample within the bound and finite)."""
    err = np.abs(np.asarray(x, dtype=np.float64) - x_ref)
    ok = bool(np.isfinite(x).all() and (err <= B).all())
    return float((err / B).max()) if np.isfinite(err).all() else float("inf"), ok


# ---- guides ---------------------------------------------------------------------------------------------------------------------------

SPARSE_H_VAL = 0.08    # P(1) = exp(-1 / 0.0064) < 2^-225: below every floor, a pixel counts only where its value is the sample's


def sparse_guide(w, h, seed):
    """Sparse support: with SPARSE_H_VAL a sample sees only the pixels of its own value, and the values are a fixed permutation of
    0 .. 255 walked with a stride coprime to 256 along the raster, so the pixels of one value are 256 raster steps apart: a handful
    within a sample's reach, each of which moves D by far more than the bound."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(256)
    k = np.arange(w * h, dtype=np.int64)
    return perm[(k * 37 + (k // 256) * 11) % 256].astype(np.uint8).reshape(h, w)


def signed_plane(w, h, seed):
    """A signed float plane with cancellation: alternating signs along both axes under a slow envelope, values with a lo half."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:h, 0:w]
    s = np.where((r + c) % 2 == 0, 1.0, -1.0) * (0.5 + 0.25 * np.sin(r / 7.0)) + 0.01 * rng.normal(size=(h, w))
    return s.astype(np.float32)


# ---- numpy emulation of the grid-factored form ------------------------------------------------------------------------------------------

DEFECTS = ("drop_lo_hi", "chunk_short", "reach_short", "padding_column", "neighbour_weight")


def _split(v32):
    hi = v32.astype(np.float16)
    lo = (v32 - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def emulate_grid(img, rows, cols, h_loc, h_val, row0=0, row1=None, plane=None, defect=None):
    """(D or U_s, Uy) as k_dgrid_hist, k_dgrid_erfrag, k_dgrid_zmfma and k_dgrid_final_parts compute them over the image rows [row0,
    row1): the f32 histogram in ascending column order (weighted: one fma per pixel), the host's power-of-two scale from wmax, the (hi,
    lo) splits of 2^15 Er and 2^wsh Wt, three products per 16-row k-step with one f32 rounding each, one f32 sum per chunk of 512 rows,
    f64 over the chunks c_lo .. c_hi of a grid row's reach and over the values. The tables are the host's (correctly rounded f32).
    defect: one of DEFECTS --
      drop_lo_hi        the Er-lo x Wt-hi product left out
      chunk_short       c_hi from the grid row itself instead of the end of its reach: a grid row within the radius before a chunk
                        boundary loses the next chunk
      reach_short       the reach of a grid row one image row short where it still matters: the rows at the largest distance with
                        Er >= 2^-10 dropped. (The kernels' own radius is the f32 table's first exact zero: the row one short of it weighs
                        less than 2^-126 and no bound can see it -- test_degree_bound.py shows that variant too, as `zero_radius_short`)
      padding_column    the last grid column read at the padding column ncp - 1 (applies where nc is no multiple of 4)
      neighbour_weight  weighted form: a pixel's weight taken at the next column"""
    assert defect is None or defect in DEFECTS + ("zero_radius_short",)
    h, w = img.shape
    row1 = h if row1 is None else row1
    nrows, nr, nc = row1 - row0, len(rows), len(cols)
    ncp, maxdim = round_up(nc, 4), max(w, h)
    et, pt = etab32(h_loc, maxdim), ptab32(h_val)
    radius = zero_radius(h_loc, maxdim)
    et_r = et.copy()
    if defect == "reach_short":
        et_r[int(np.nonzero(et >= 2.0 ** -10)[0][-1])] = 0.0
    if defect == "zero_radius_short" and radius < maxdim:
        et_r[radius - 1] = 0.0
    # 1. Wt[r][v][b], f32, ascending columns (pixels out of a column's reach add the table's exact zero)
    ne = min(maxdim, radius + 1)
    C = np.asarray(cols, dtype=np.int64)
    Wt = np.zeros((nrows, 256, ncp), dtype=np.float32)
    sub = img[row0:row1]
    rr = np.arange(nrows)
    wp = None if plane is None else np.asarray(plane, dtype=np.float32)[row0:row1]
    for c in range(w):
        e = np.zeros(ncp, dtype=np.float32)
        e[:nc] = et[np.minimum(np.abs(c - C), ne - 1)]
        v = sub[:, c].astype(np.int64)
        if wp is None:
            Wt[rr, v, :] = Wt[rr, v, :] + e[None, :]
        else:
            wc = wp[:, min(c + 1, w - 1)] if defect == "neighbour_weight" else wp[:, c]
            Wt[rr, v, :] = (Wt[rr, v, :].astype(np.float64) + wc.astype(np.float64)[:, None] * e.astype(np.float64)[None, :]).astype(np.float32)
    # 2. the scale
    wmax = wmax_of(h_loc, w)
    if wp is not None:
        wabs = float(np.abs(wp).max())
        wmax *= wabs if wabs > 0 else 1.0
    wexp = math.frexp(wmax)[1]
    wsh = 14 - wexp
    # 3. splits
    R = np.asarray(rows, dtype=np.int64)
    Er = np.float32(32768.0) * et_r[np.abs((row0 + np.arange(nrows))[None, :] - R[:, None])]      # [nr, nrows]
    ah, al = _split(Er.astype(np.float32))
    bh, bl = _split((Wt.reshape(nrows, 256 * ncp) * np.float32(2.0 ** wsh)).astype(np.float32))
    f8 = np.float64
    nchunks = -(-nrows // DGZ_CHUNK)
    Z = np.zeros((nchunks, nr, 256 * ncp), dtype=np.float32)
    outscale = np.float32(2.0 ** (-15 - wsh))
    for ch in range(nchunks):
        acc = np.zeros((nr, 256 * ncp), dtype=np.float32)
        for k0 in range(ch * DGZ_CHUNK, min(nrows, (ch + 1) * DGZ_CHUNK), 16):
            k = slice(k0, min(k0 + 16, nrows))
            for a, b in [(ah, bh), (ah, bl)] + ([] if defect == "drop_lo_hi" else [(al, bh)]):
                acc = (acc.astype(f8) + a[:, k].astype(f8) @ b[k, :].astype(f8)).astype(np.float32)
        Z[ch] = acc * outscale
    # 4. f64 over the chunks of each grid row's reach and over the values
    rad = radius if radius < maxdim else 1 << 28
    D, Uy = np.zeros(nr * nc), np.zeros(nr * nc)
    vals = np.arange(256, dtype=np.float64)
    for a in range(nr):
        ra = int(R[a]) - row0
        hi = ra + rad - 1
        c_lo = max(0, int(math.trunc((ra - rad + 1) / DGZ_CHUNK)))
        c_hi = -1 if hi < 0 else min(nchunks - 1, hi // DGZ_CHUNK)
        if defect == "chunk_short":
            c_hi = -1 if hi < 0 else min(nchunks - 1, max(ra, 0) // DGZ_CHUNK)
        zs = Z[c_lo:c_hi + 1, a].astype(f8).sum(axis=0).reshape(256, ncp) if c_hi >= c_lo else np.zeros((256, ncp))
        for b in range(nc):
            sv = int(img[int(R[a]), int(C[b])])
            col = ncp - 1 if (defect == "padding_column" and b == nc - 1) else b
            P = pt[np.abs(sv - np.arange(256))].astype(f8)
            D[a * nc + b] = float((P * zs[:, col]).sum())
            Uy[a * nc + b] = float((vals * P * zs[:, col]).sum())
    return D, Uy


def emulate_direct_strips(img, idx, h_loc, h_val, pad_weight=0.0):
    """A small model of degree_chunk_lut's strips over all rows: D[i] = sum_r Er sum_c Ec P(|v_i - img[r][c]|) in float64 with the f32
    tables, the row padded to a multiple of 4 columns with pixels of value 0 (the staged tile's padding, affinity.hip:192) whose Ec is
    `pad_weight`: 0 as the kernel has it (:201), 1 for the defect."""
    h, w = img.shape
    idx = np.asarray(idx, dtype=np.int64)
    et, pt = etab32(h_loc, max(w, h)).astype(np.float64), ptab32(h_val).astype(np.float64)
    sr, sc, sv = idx // w, idx % w, img.reshape(-1)[idx].astype(np.int64)
    npad = round_up(w, 4) - w
    D = np.zeros(idx.size)
    for r in range(h):
        Er = et[np.abs(sr - r)]
        Ec = et[np.abs(sc[:, None] - np.arange(w)[None, :])]
        P = pt[np.abs(sv[:, None] - img[r].astype(np.int64)[None, :])]
        D += Er * ((Ec * P).sum(axis=1) + npad * pad_weight * pt[np.abs(sv - 0)])
    return D
