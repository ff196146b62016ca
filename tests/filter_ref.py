"""The float64 reference and the error bounds of the filter stage (glf_Filter_ex) kernel by kernel, the inputs and shapes of its tests,
and a numpy emulation of k_phi_t_y, k_apply_filter (and the panel form) in their operation order. Shared by tests/test_filter_bound.py
(CPU) and tests/test_gpu_filter.py. U and V are tests/operator_ref.py's; u = U = 2^-24, e = 2^-53, gamma(n, u) = n u / (1 - n u).

Each kernel is held against float64 of its OWN inputs: the projection against Phi^T x of the f32 bits of Phi, the apply kernels against
gain Phi w - ysub x with w = f(lam) c formed in float64 from the c the call itself reports, so one kernel's error is not charged to the
next. Line numbers as of this commit (csrc/).

Projection, componentwise |c_j - c_ref_j| <= gamma_j sum_x |Phi_xj x_x|:
kernel               f32 links  f64 links                        where
k_phi_t_y            32         33 + nrl + ceil(nblk / 256) + 8  filter.hip:35 one fmaf per pixel (y is exact in f32), the chain cut at
                                                                 32 (:36-40); f64 over a thread's chains (:37, :42: at most 1024 / 32
                                                                 + 1), the nrl = 256 / ld row lanes in LDS (:47), then k_cols_sum: a
                                                                 thread's rows (:58, ceil(nblk / 256) of them) and the 8-level tree
                                                                 (:61-64)
k_phi_t_signals      0          1024 / nrl + nrl + ceil(nblk / 256) + 8
                                                                 filter.hip:289 an f64 fma per pixel and plane (f32 x f32 is exact in
                                                                 f64), one chain per thread over its 1024 / nrl rows; LDS :297; k_cols_sum
k_phi_t_pix_signals  0          the same                         entrywise.hip:260-263, the channels read from the image (exact)
k_phi_gram           64         ceil(tiles / nblk) + ceil(nblk / 256) + 8
                                                                 filter.hip:153 chains of 64 f32 fmas over a tile of 64 pixels, f64 across
                                                                 the tiles of a workgroup (:154; tiles = ceil(npix / 64), nblk = min(512,
                                                                 tiles), :169), then k_cols_sum; against sum_x |Phi_xi Phi_xj|

Apply, per pixel |corr - corr_ref| <= gamma(K, u) gain sum_j |Phi_xj w_j| + u |corr_ref| (+ the sharpening weights' f64 slack):
kernel                        K                         where
k_apply_filter<LD>            7 + log2(LD / 4)          w rounded to f32 on the host (filter_rule.hpp:57; 1), the product (1) and the three
k_apply_filter_signals<LD>                              in-lane adds (filter.hip:193; a term passes through at most 3), log2(LD / 4) shuffle
                                                        adds (:195), gain * s (:200; 1), and one more for the subtraction's share of the
                                                        dot product's error; the subtraction itself is the u |corr_ref| term (ysub is 0
                                                        or 1, so ysub * y is exact). hipcc may contract products and adds into fmas: that
                                                        removes roundings, never adds one, so the bound holds either way. The planes'
                                                        out = v + c adds one rounding of the stored value: u |v + corr_ref|.
k_filter_accum / _finish      13 + (panels - 1)         the same dot product at LD = 256 (filter.hip:446-448: 1 + 1 + 3 + 6), one f32 add
                                                        per further panel (:449), gain * acc (:460), the subtraction's share
k_apply_filter_pix<LD, G>     f32: 1; f64: 6 + log2(LD / 4)
k_apply_filter_pix_signals                              entrywise.hip:190-195: only the rounding of w to f32 is an f32 rounding; the
                                                        products are exact in f64, three adds, the shuffle adds, gain * s and the
                                                        subtraction are f64 roundings: u gain sum |Phi w| + gamma(6 + log2(LD / 4), e)
                                                        gain sum |Phi w| + e |corr_ref|. The stored float (zf, an f32 output, a plane)
                                                        adds e |x + corr| for the sum and u |x + corr| for its rounding.

The c epilogue of the Nystroem forms (the whole path's c = Phi^T y for an 8-bit grey guide: rq.d_c), against Phi_cap^T y of the captured
Phi, componentwise |c_j - c_ref_j| <= gamma_j sum_x |Phi_xj y_x|. Every form accumulates csum = fmaf(v, y, csum) in f32 per lane with v
the value it stores into Phi, then goes to f64:
form                      f32 links            where
direct f32                16 PB + 1            nystroem.hip:216-234 one fmaf per accumulator register over PB blocks of 16, one shuffle add
                                               of the two halves (:242); PB = 2 up to ld 128, 1 at ld 256 (nys_dispatch_ld, :852-855)
direct split-f16, LUT     16 PB + 1            nystroem.hip:722-734, PB = 2 up to ld 64, 1 above
grid                      width                nystroem_grid.inc:890: a lane adds one fmaf per pixel of its half of the chunks its wave
                                               takes from one image row; never more than the row has pixels
rank                      4 + 5                nystroem_rank.inc:622-625 one fmaf per chunk of the wave (RANK_CPW = 4, :29), then five
                                               shuffle adds over the 32 pixels of the half (:637)
band                      16 PB + 1            nystroem_band.inc:702-706, :716; BAND_PB = 2, one tile per wave
f64 links, all forms: at most 16 in the kernel (one per wave's partial: nystroem.hip:248, nystroem_grid.inc:965, nystroem_rank.inc:644,
nystroem_band.inc:722), sum_rows (nystroem.hip:254-281: 1024 / nrl + nrl in k_rows_sum_lvl1, one per 1024 partial rows and the
accumulated value in k_rows_sum_lvl2; no more partial rows than pixels), and the sample rows' share (k_scatter_sample_rows, :909-936:
exact products, 512 / nrl + nrl adds, one per 512 samples and the accumulated value).

Outputs. Grey: zf = fl32(fl32(y) + corr) and out = clamp(y + floor(corr), 0, 255), NaN -> 0, exactly, from the call's own d_corr
(glf_internal.hpp:290-296). 16 bits: the same rule on the f64 correction (:298-305); 8-bit colour: the f64 correction rounded to f32
first (:402), so its window of doubt around an integer is wider by u |corr|. Where corr_ref is within the bound of an integer either
neighbour is accepted; AMBIGUOUS_CAP caps the share of such pixels per case.

These numbers are derived from the code, not measured; profiles/filter_error.json records how far below them the kernels stay."""
import math

import numpy as np

from operator_ref import U, V  # noqa: F401  (V: the split-f16 unit of the whole-path leg)

E = 2.0 ** -53
REFERENCE, POC, SMOOTH, SHARPEN = 0, 1, 2, 3
FORMATS = ("u8", "rgb8", "u16", "f32", "rgbf32")
CHANNELS = {"u8": 1, "rgb8": 3, "u16": 1, "f32": 1, "rgbf32": 3}
AMBIGUOUS_CAP = 0.01
MAX_BLOCKS = 8192
# glf_filter_info.kernels
(FK_PHI_T_Y, FK_PHI_T_SIGNALS, FK_PHI_T_PIX_SIGNALS, FK_PHI_GRAM, FK_APPLY, FK_APPLY_SIGNALS, FK_APPLY_PIX, FK_APPLY_PIX_SIGNALS, FK_PLANES,
 FK_ACCUM, FK_FINISH) = (1 << i for i in range(11))

# (width, height, ld, m): the smallest shapes at which each path differs
TINY = [(53, 37, ld, m) for ld in (32, 64, 128, 256) for m in (ld, ld - 12)]
STRIDE = [(523, 503, 32, 32), (367, 359, 64, 64), (257, 257, 128, 128), (181, 183, 256, 256)]  # just above 8192 x pixels per block pass
WIDE = [(53, 37, 512, 300), (181, 183, 512, 300)]                                                # two panels, the second with 44 columns


def gamma(n, u):
    return n * u / (1.0 - n * u)


def _join(a, b):
    return a + b + a * b


def ppb(ld):
    return 256 // (min(ld, 256) // 4)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def image(w, h, seed=1):
    """127.5 + 100 sin(x / 17) cos(y / 23) plus noise, clipped: uint8 [h, w]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    v = 127.5 + 100.0 * np.sin(x / 17.0) * np.cos(y / 23.0) + rng.normal(0.0, 12.0, (h, w))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def guide(fmt, w, h, seed=1):
    """The guide of a format: the grey image; for the others tests/pix_cases.py's, the integer ones with two 4 x 4 patches at the ends
    of their range (16 bits reach 0 and 65535), the float ones times 100 (negative and large values)."""
    if fmt == "u8":
        return image(w, h, seed)
    import pix_cases
    g = pix_cases.pix_case(fmt, w, h, seed)[0].copy()
    if fmt in ("rgb8", "u16"):
        g[3:7, 3:7] = np.iinfo(g.dtype).max
        g[h - 7:h - 3, w - 7:w - 3] = 0
        return g
    return (g * np.float32(100.0)).astype(np.float32)


def planes(nsig, w, h, seed=7):
    """Zero-mean float planes [nsig, h, w]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for k in range(nsig):
        v = 40.0 * np.sin(x / (11.0 + 3 * k)) * np.cos(y / (13.0 + 2 * k)) + rng.normal(0.0, 5.0, (h, w))
        out.append(v - v.mean())
    return np.stack(out).astype(np.float32)


def make_phi(w, h, m, ld, seed=5, pad=0.0):
    """The float32 rounding of a QR-orthonormalised N x m matrix -- a constant column, three low-frequency columns matched to the
    image, Gaussian columns -- as float32 [N, ld], the padded columns holding `pad`."""
    N = w * h
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    cols = [np.ones(N), (np.sin(x / 17.0) * np.cos(y / 23.0)).ravel(), np.sin(x / 17.0).ravel(), np.cos(y / 23.0).ravel()][:m]
    A = np.empty((N, m))
    A[:, :len(cols)] = np.stack(cols, axis=1)
    A[:, len(cols):] = rng.normal(0.0, 1.0, (N, m - len(cols)))
    Q, R = np.linalg.qr(A)
    Q *= np.sign(np.diag(R))[None, :]
    out = np.full((N, ld), pad, dtype=np.float32)
    out[:, :m] = Q.astype(np.float32)
    return out


def lam_ramp(m):
    return (np.arange(m, dtype=np.float64) + 1.0) / (m + 1.0)


# ---- the filter rule (csrc/filter_rule.hpp) ---------------------------------------------------------------------------------------
def filter_gain(mode, gain):
    return float(np.float32(gain)) if mode == REFERENCE else 1.0


def filter_ysub(mode):
    return 1.0 if mode >= SMOOTH else 0.0


def weights(mode, lam, c, filter_pow=1, beta=1.5, G=None):
    """(w in float64, dw): filter_weights_row before its rounding to f32, and a bound on what the host's own f64 evaluation may
    differ from this one by (sums in another order; pow against a product)."""
    lam = np.asarray(lam, dtype=np.float64)
    m = lam.size
    c = np.asarray(c, dtype=np.float64)[:m]
    if mode == SHARPEN:
        L = 1.0 - lam
        Ga = np.abs(G[:m, :m])
        t = L * c
        u = L * (G[:m, :m] @ t)
        v = L * (G[:m, :m] @ u)
        du = (m + 2) * 2 * E * np.abs(L) * (Ga @ np.abs(t))
        dv = (m + 2) * 2 * E * np.abs(L) * (Ga @ np.abs(u)) + np.abs(L) * (Ga @ du)
        out = (1.0 + beta) * u - beta * v
        return out, (1.0 + beta) * du + beta * dv + 6 * E * ((1.0 + beta) * np.abs(u) + beta * np.abs(v))
    if mode == POC:
        f = -(lam + 5.0)
    elif mode == SMOOTH:
        f = 1.0 - lam
    else:
        f = lam ** (filter_pow if filter_pow > 0 else 1)
    out = f * c
    return out, 4 * E * np.abs(out)


# ---- projection --------------------------------------------------------------------------------------------------------------------
def proj_counts(kernel, ld, npix):
    """(f32 links, f64 links) of a projection kernel over npix pixels."""
    nrl, nblk = 256 // ld, -(-npix // 1024)
    cols_sum = -(-nblk // 256) + 8
    if kernel == "phi_t_y":
        return 32, 33 + nrl + cols_sum
    if kernel in ("phi_t_signals", "phi_t_pix_signals"):
        return 0, 1024 // nrl + nrl + cols_sum
    if kernel == "phi_gram":
        tiles = -(-npix // 64)
        nb = max(1, min(512, tiles))
        return 64, -(-tiles // nb) + -(-nb // 256) + 8
    raise KeyError(kernel)


def proj_gamma(kernel, ld, npix):
    k32, k64 = proj_counts(kernel, ld, npix)
    return _join(gamma(k32, U), gamma(k64, E))


def nystroem_c_counts(form, ld, width, N, p):
    """(f32 links, f64 links) of a Nystroem form's c epilogue, sum_rows and the sample rows' share (the table above)."""
    nrl = 256 // ld
    k64 = 16 + (1024 // nrl + nrl) + (N // 1024 + 2) + (512 // nrl + nrl) + (p // 512 + 2)
    k32 = {"direct_f32": 16 * (2 if ld <= 128 else 1) + 1, "direct_f16s": 16 * (2 if ld <= 64 else 1) + 1,
           "lut": 16 * (2 if ld <= 64 else 1) + 1, "grid": width, "rank": 4 + 5, "band": 16 * 2 + 1}[form]
    return k32, k64


def nystroem_c_gamma(form, ld, width, N, p):
    k32, k64 = nystroem_c_counts(form, ld, width, N, p)
    return _join(gamma(k32, U), gamma(k64, E))


def proj_ref(phi, x, pix0, pix1):
    """(c_ref, sum_x |Phi_xj x_x|) over the pixels [pix0, pix1): phi float32 [N, cols], x [N] (exact values)."""
    P = phi[pix0:pix1].astype(np.float64)
    xv = np.asarray(x, dtype=np.float64).ravel()[pix0:pix1]
    return P.T @ xv, np.abs(P).T @ np.abs(xv)


def gram_ref(phi, m):
    P = phi[:, :m].astype(np.float64)
    return P.T @ P, np.abs(P).T @ np.abs(P)


# ---- apply -------------------------------------------------------------------------------------------------------------------------
def apply_K(ld, panels=0):
    """The f32 roundings a term of the grey kernels' dot product carries (the table above)."""
    if panels:
        return 13 + (panels - 1)
    return 7 + int(math.log2(ld // 4))


def apply_ref(phi, m, w64, dw, gain, ysub, x, pix0, pix1, ld, f64_kernel=False, panels=0):
    """(corr_ref, bound) per pixel of [pix0, pix1): corr_ref = gain Phi w - ysub x in float64, and the derived bound of the kernel."""
    P = phi[pix0:pix1, :m].astype(np.float64)
    xv = np.asarray(x, dtype=np.float64).ravel()[pix0:pix1]
    corr = gain * (P @ w64) - ysub * xv
    A = gain * (np.abs(P) @ np.abs(w64))
    slack = gain * (np.abs(P) @ dw)
    if f64_kernel:
        g = _join(U, gamma(6 + int(math.log2(ld // 4)), E))
        return corr, g * A + E * np.abs(corr) + slack
    return corr, gamma(apply_K(ld, panels), U) * A + U * np.abs(corr) + slack


def stored_f32_slack(v):
    """The stored float x + corr: the f64 (or f32) sum and its rounding to f32."""
    return (U + 2 * E) * np.abs(v)


# ---- the output rules --------------------------------------------------------------------------------------------------------------
def out_rule(x, c, top):
    """clamp(x + floor(c), 0, top), NaN -> 0: filter_output (top 255, c an f32) and filter_output_u16 (top 65535, c an f64)."""
    c = np.asarray(c)
    with np.errstate(invalid="ignore"):
        fc = np.floor(np.clip(np.where(np.isnan(c), 0.0, c).astype(np.float64), -1.0e6, 1.0e6))
    z = np.asarray(x, dtype=np.int64) + fc.astype(np.int64)
    z = np.clip(z, 0, top)
    return np.where(np.isnan(c), 0, z)


def zf_rule(y, c32):
    """fl32(fl32(y) + corr), the grey kernels' float z."""
    return (np.asarray(y).astype(np.float32) + np.asarray(c32, dtype=np.float32)).astype(np.float32)


def ambiguous(corr_ref, bound):
    """Pixels whose reference correction is within its bound of an integer: floor may fall either way."""
    return np.abs(corr_ref - np.rint(corr_ref)) <= bound


def check_int_output(out, x, corr_ref, bound, top):
    """(ok, ambiguous share): out equals the rule on corr_ref wherever that is farther from an integer than its bound, one of the two
    neighbours' results elsewhere."""
    amb = ambiguous(corr_ref, bound)
    lo, hi = out_rule(x, corr_ref - bound, top), out_rule(x, corr_ref + bound, top)
    out = np.asarray(out, dtype=np.int64)
    ok = np.where(amb, (out == lo) | (out == hi), out == out_rule(x, corr_ref, top))
    return bool(ok.all()), float(amb.mean())


# ---- emulation -----------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf through float64: the product of two f32 is exact there; the sum is rounded to f64 and then to f32 (a double rounding that
    differs from fmaf's single one only on a near-tie: below anything these tests resolve)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _cols_sum(part):
    """k_cols_sum: 256 threads stride the rows, then the LDS tree."""
    nrows = part.shape[0]
    pad = -(-nrows // 256) * 256
    p = np.zeros((pad,) + part.shape[1:])
    p[:nrows] = part
    p = p.reshape(pad // 256, 256, *part.shape[1:])
    sh = np.zeros((256,) + part.shape[1:])
    for r in range(p.shape[0]):
        sh = sh + p[r]
    o = 128
    while o > 0:
        sh[:o] = sh[:o] + sh[o:2 * o]
        o >>= 1
    return sh[0]


def emu_phi_t_y(phi, img, pix0, pix1, defect=None):
    """k_phi_t_y + k_cols_sum over the pixels [pix0, pix1): phi float32 [N, ld], img uint8. defect "drop_last_block": the last, partial
    1024-block is not summed."""
    ld = phi.shape[1]
    nrl = 256 // ld
    npix = pix1 - pix0
    nblk = -(-npix // 1024)
    if defect == "drop_last_block" and npix % 1024:
        nblk, npix = nblk - 1, (nblk - 1) * 1024
    if nblk == 0:
        return np.zeros(ld)
    P = np.zeros((nblk * 1024, ld), dtype=np.float32)
    Y = np.zeros(nblk * 1024, dtype=np.float32)
    P[:npix] = phi[pix0:pix0 + npix]
    Y[:npix] = np.asarray(img).ravel()[pix0:pix0 + npix].astype(np.float32)
    per = 1024 // nrl                     # rows per thread: r = rl + k nrl
    nch = -(-per // 32)
    P = P.reshape(nblk, per, nrl, ld)
    Y = Y.reshape(nblk, per, nrl, 1)
    s = np.zeros((nblk, nrl, ld))
    for ch in range(nch):
        acc = np.zeros((nblk, nrl, ld), dtype=np.float32)
        for k in range(ch * 32, min(per, ch * 32 + 32)):
            acc = _fma32(P[:, k], np.broadcast_to(Y[:, k], acc.shape), acc)
        s = s + acc.astype(np.float64)
    t = np.zeros((nblk, ld))
    for r in range(nrl):
        t = t + s[:, r]
    return _cols_sum(t)


def emu_dot(P, w, contract=False, short_tree=False):
    """The dot product of k_apply_filter: float4 lanes, the xor tree. P float32 [npix, LD], w float32 [LD]."""
    npix, LD = P.shape
    lpp = LD // 4
    F = P.reshape(npix, lpp, 4)
    W = np.asarray(w, dtype=np.float32).reshape(1, lpp, 4)
    if contract:
        s = (F[..., 0] * W[..., 0]).astype(np.float32)
        for k in (1, 2, 3):
            s = _fma32(F[..., k], np.broadcast_to(W[..., k], s.shape), s)
    else:
        pr = (F * W).astype(np.float32)
        s = ((pr[..., 0] + pr[..., 1]).astype(np.float32) + pr[..., 2]).astype(np.float32)
        s = (s + pr[..., 3]).astype(np.float32)
    lane = np.arange(lpp)
    o = lpp // 2
    while o > (1 if short_tree else 0):
        s = (s + s[:, lane ^ o]).astype(np.float32)
        o >>= 1
    return s[:, 0]


def emu_apply(phi, w, x, gain, ysub, pix0, pix1, contract=False, defect=None):
    """k_apply_filter / k_apply_filter_signals over [pix0, pix1): the f32 correction per pixel of the range (NaN where the defect
    "no_stride" leaves a pixel unwritten). defect "short_tree": the shuffle tree one level short."""
    P = phi[pix0:pix1]
    s = emu_dot(P, w, contract, short_tree=defect == "short_tree")
    xv = np.asarray(x).ravel()[pix0:pix1].astype(np.float32)
    g, ys = np.float32(gain), np.float32(ysub)
    if contract:
        c = _fma32(np.broadcast_to(g, s.shape), s, -(ys * xv))
    else:
        c = ((g * s).astype(np.float32) - (ys * xv).astype(np.float32)).astype(np.float32)
    if defect == "no_stride":
        c = c.copy()
        c[MAX_BLOCKS * ppb(phi.shape[1]):] = np.nan
    return c


def emu_panels(phi, m, w_panels, x, gain, ysub, pix0, pix1, stuck_first=False):
    """k_filter_accum over the 256-column panels and k_filter_finish: w_panels a list of float32 [256] per panel."""
    acc = None
    for q, w in enumerate(w_panels):
        s = emu_dot(np.ascontiguousarray(phi[pix0:pix1, q * 256:(q + 1) * 256]), w)
        acc = s if (acc is None or stuck_first) else (acc + s).astype(np.float32)
    xv = np.asarray(x).ravel()[pix0:pix1].astype(np.float32)
    return ((np.float32(gain) * acc).astype(np.float32) - (np.float32(ysub) * xv).astype(np.float32)).astype(np.float32)


def panel_weights(mode, lam, c, m, filter_pow=1, lam_from_first=False):
    """The panels' f32 weights [256] each, the padded columns zero. lam_from_first: the seeded defect (every panel takes the first
    panel's eigenvalues)."""
    out = []
    for q in range(-(-m // 256)):
        mq = min(256, m - q * 256)
        lq = lam[:mq] if lam_from_first else lam[q * 256:q * 256 + mq]
        w64, _ = weights(mode, lq, c[q * 256:q * 256 + mq], filter_pow)
        w = np.zeros(256, dtype=np.float32)
        w[:mq] = w64.astype(np.float32)
        out.append(w)
    return out


def dump_record(path, rec):
    """The error record as JSON with one row per line: [kernel, case, gamma, worst error over bound, worst of]."""
    import json
    rows = [r if isinstance(r, list) else [r["kernel"], r["case"], float("%.4g" % r["gamma"]), round(r["worst_error_over_bound"], 4), r["worst_of"]]
            for r in rec["rows"]]
    head = {k: v for k, v in rec.items() if k != "rows"}
    head["columns"] = "kernel, case, gamma, worst_error_over_bound, worst_of"
    with open(path, "w") as f:
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "rows": [\n' + ",\n".join("  " + json.dumps(r) for r in rows) + "\n ]\n}\n")


def check(x, ref, bound):
    """(largest |x - ref| / bound, all within)."""
    err = np.abs(np.asarray(x, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    worst = float(np.nanmax(ratio)) if ratio.size else 0.0
    return worst, bool((err <= bound).all())
