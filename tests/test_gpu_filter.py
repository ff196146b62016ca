"""The filter stage kernel by kernel, through glf_Filter_ex (the stage call on a given Phi, with the whole path's functions, a row
range, planes, a projection handed in, and a report of what ran), each kernel against float64 of its own inputs with a bound derived
from its arithmetic. Needs an MI355X: -m gpu.

Reference, bounds and inputs: tests/filter_ref.py (its docstring holds the counts with the code each comes from; tests/test_filter_bound.py
holds an emulation to them on the CPU and seeds the defects). Every call writes into sentinel-filled buffers, every pixel is compared,
pixels outside the row range must keep the sentinel, and glf_filter_info is compared with the plan: a test that ran another kernel
than it names fails. The grey outputs are held exactly to their rule from the call's own d_corr; the integer outputs of the pixel
formats wherever the reference correction is farther from an integer than its bound.

The stage call projects with k_phi_t_y; the whole path takes c from the Nystroem extension's epilogue instead. The last test closes that
gap: one captured whole-path run per Nystroem form, its c against float64 Phi_cap^T y, its corr and out as above.

What these tests cannot see: multi-rank collectives, the fused forms (tests/test_gpu_band_*.py), and errors below the derived bounds.

Set GLF_FILTER_ERROR_JSON to a path to have gamma and the largest observed |error| / bound per kernel and case written there (a
record: the asserted bound is the derived one)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import filter_ref as fr  # noqa: E402
import nystroem_ref as nref  # noqa: E402

SENTINEL = -12345.5
INT_SENTINEL = {"u8": 165, "rgb8": 165, "u16": 42405}
PIX = {"u8": glf.PIX_U8, "rgb8": glf.PIX_RGB8, "u16": glf.PIX_U16, "f32": glf.PIX_F32, "rgbf32": glf.PIX_RGBF32}
OUT_DTYPE = {"u8": np.uint8, "rgb8": np.uint8, "u16": np.uint16, "f32": np.float32, "rgbf32": np.float32}
TOP = {"u8": 255, "rgb8": 255, "u16": 65535}
_RECORD, _INPUTS, _MATS = {}, {}, {}
ID = lambda s: "%dx%d-ld%d-m%d" % s  # noqa: E731


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = glf.Context(0)
    yield c
    c.destroy(*_MATS.values())
    _MATS.clear()
    c.close()


@pytest.fixture(scope="module", autouse=True)
def _error_record():
    yield
    path = os.environ.get("GLF_FILTER_ERROR_JSON")
    if path and _RECORD:
        agg = {}
        for (kernel, case, what), (ratio, g) in sorted(_RECORD.items()):
            a = agg.setdefault((kernel, case), dict(kernel=kernel, case=case, gamma=g, worst_error_over_bound=-1.0, worst_of=None))
            if ratio > a["worst_error_over_bound"]:
                a["worst_error_over_bound"], a["worst_of"] = ratio, what
        what = ("gamma (derived, asserted) and the largest observed |error| / bound per kernel and case of tests/test_gpu_filter.py on an "
                "MI355X (GLF_FILTER_ERROR_JSON=<this file> python -m pytest tests/test_gpu_filter.py -m gpu). A record only.")
        fr.dump_record(path, dict(what=what, rows=[agg[k] for k in sorted(agg)]))


def _inputs(shape, pad=0.0):
    """(phi float32 [N, ld], lam): computed once per shape and left unchanged."""
    key = shape + (pad,)
    if key not in _INPUTS:
        w, h, ld, m = shape
        phi = fr.make_phi(w, h, m, ld, pad=pad)
        phi.setflags(write=False)
        _INPUTS[key] = (phi, fr.lam_ramp(m))
    return _INPUTS[key]


def _mat(ctx, phi, m, key=None):
    """phi float32 [N, ld] as a dense raster-order glf_mat of m columns, its padded columns as given."""
    if key is not None and key in _MATS:
        return _MATS[key]
    mat = glf.Mat()
    N, ld = phi.shape
    ctx._check(glf._lib.glf_mat_create_dense(ctx._ctx, C.byref(mat), C.c_int64(N), C.c_int64(m), C.c_int64(ld)))
    a = np.ascontiguousarray(phi)
    ctx._check(glf._lib.glf_memcpy_h2d(ctx._ctx, C.c_void_p(mat.data), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes)))
    mat.row_order = glf.ROWS_RASTER
    if key is not None:
        _MATS[key] = mat
    return mat


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _plan(fmt, ld, m, npix, nsig, mode, given_c):
    """glf_filter_info as the host must fill it."""
    wide = ld > 256
    if wide:
        k = fr.FK_ACCUM | fr.FK_FINISH | (0 if given_c else fr.FK_PHI_T_Y)
    elif fmt == "u8":
        k = fr.FK_APPLY | (0 if given_c else fr.FK_PHI_T_Y)
        if nsig:
            k |= fr.FK_APPLY_SIGNALS | (0 if given_c else fr.FK_PHI_T_SIGNALS)
    elif nsig:
        k = fr.FK_APPLY_PIX_SIGNALS | (0 if given_c else fr.FK_PHI_T_PIX_SIGNALS)
    else:
        k = fr.FK_PLANES | fr.FK_APPLY_PIX | (0 if given_c else fr.FK_PHI_T_SIGNALS)
    if mode == fr.SHARPEN:
        k |= fr.FK_PHI_GRAM
    p = fr.ppb(ld)
    blocks = min(fr.MAX_BLOCKS, -(-npix // p))
    return dict(kernels=k, ld=min(ld, 256), panels=-(-m // 256) if wide else 0, proj_blocks=0 if given_c else -(-npix // 1024),
                apply_blocks=blocks, grid_strided=int(blocks * p < npix))


def _run(ctx, fmt, shape, mode=fr.REFERENCE, filter_pow=1, gain=3.0, rows=None, sig=None, c_in=None, pad=0.0, phi=None, img=None,
         want_corr=None):
    """One stage call into sentinel-filled buffers; the outputs on the host, with the info and the inputs."""
    w, h, ld, m = shape
    N, nch = w * h, fr.CHANNELS[fmt]
    phi_np, lam = _inputs(shape, pad)
    key = shape + (pad,)
    if phi is not None:
        phi_np, key = phi, None
    mat = _mat(ctx, phi_np, m, key)
    img = fr.guide(fmt, w, h) if img is None else img
    nsig = 0 if sig is None else sig.shape[0]
    r0, r1 = (0, h) if rows is None else rows
    pix0, pix1 = r0 * w, r1 * w
    if fmt in INT_SENTINEL:
        out0 = np.full((h, w, nch) if nch == 3 else (h, w), INT_SENTINEL[fmt], dtype=OUT_DTYPE[fmt])
    else:
        out0 = np.full((h, w, nch) if nch == 3 else (h, w), SENTINEL, dtype=np.float32)
    d_out, d_zf = _dev(ctx, out0), _dev(ctx, np.full((nch, h, w), SENTINEL, dtype=np.float32))
    want_corr = (fmt == "u8" and ld <= 256) if want_corr is None else want_corr
    d_corr = _dev(ctx, np.full(pix1 - pix0, SENTINEL, dtype=np.float32)) if want_corr else None
    d_sig = None if sig is None else _dev(ctx, sig)
    d_sig_out = None if sig is None else _dev(ctx, np.full(sig.shape, SENTINEL, dtype=np.float32))
    c_out = np.full((nch + nsig, m), SENTINEL)
    gram = np.full((m, m), SENTINEL)
    try:
        info = ctx.Filter_ex(PIX[fmt], _dev(ctx, img), mat, lam, filter_mode=mode, filter_pow=filter_pow, gain=gain, rows=rows, sig=d_sig,
                             sig_out=d_sig_out, c_in=c_in, c_out=c_out, gram_out=gram, out=d_out, zf=d_zf, corr=d_corr)
    finally:
        if key is None:
            ctx.destroy(mat)
    res = dict(fmt=fmt, shape=shape, mode=mode, filter_pow=filter_pow, gain=gain, img=img, phi=phi_np, lam=lam, sig=sig, pix=(pix0, pix1),
               out=d_out.cpu().numpy(), zf=d_zf.cpu().numpy(), corr=None if d_corr is None else d_corr.cpu().numpy(),
               sig_out=None if sig is None else d_sig_out.cpu().numpy(), c=c_out, gram=gram, info=info, given_c=c_in is not None)
    plan = _plan(fmt, ld, m, pix1 - pix0, nsig, mode, c_in is not None)
    assert {k: info[k] for k in plan} == plan, (info, plan)
    assert (info["pix0"], info["pix1"]) == (pix0, pix1)
    # pixels outside the row range keep the sentinel
    o = res["out"].reshape(N, nch)
    assert (o[:pix0] == out0.reshape(N, nch)[:pix0]).all() and (o[pix1:] == out0.reshape(N, nch)[pix1:]).all()
    z = res["zf"].reshape(nch, N)
    assert (z[:, :pix0] == SENTINEL).all() and (z[:, pix1:] == SENTINEL).all() and not (z[:, pix0:pix1] == SENTINEL).any()
    if sig is not None:
        s = res["sig_out"].reshape(nsig, N)
        assert (s[:, :pix0] == SENTINEL).all() and (s[:, pix1:] == SENTINEL).all() and not (s[:, pix0:pix1] == SENTINEL).any()
    assert not (c_out == SENTINEL).any()
    assert (gram == SENTINEL).all() == (mode != fr.SHARPEN)
    return res


def _within(kernel, case, what, x, ref, bound, g):
    ratio, ok = fr.check(x, ref, bound)
    _RECORD[(kernel, case, what)] = (ratio, g)
    print("%s %s %s: gamma 2^%.2f, worst error / bound %.4f" % (kernel, case, what, np.log2(g), ratio))
    assert ok, (kernel, case, what, ratio)
    return ratio


def _verify(res, case, vacuity=True):
    """Every kernel of one call against float64 of its own inputs, and the outputs against their rules."""
    fmt, (w, h, ld, m), mode = res["fmt"], res["shape"], res["mode"]
    N, nch = w * h, fr.CHANNELS[fmt]
    pix0, pix1 = res["pix"]
    npix = pix1 - pix0
    phi, lam, sig = res["phi"], res["lam"], res["sig"]
    nsig = 0 if sig is None else sig.shape[0]
    gain, ysub = fr.filter_gain(mode, res["gain"]), fr.filter_ysub(mode)
    wide = ld > 256
    chans = res["img"].reshape(N, nch).T                     # [nch][N], exact values
    xs = [chans[k] for k in range(nch)] + [sig[k].ravel() for k in range(nsig)]
    if fmt == "u8":
        pk = ["phi_t_y"] + ["phi_t_signals"] * nsig
    else:
        pk = ["phi_t_pix_signals" if nsig else "phi_t_signals"] * (nch + nsig)
    G = None
    if mode == fr.SHARPEN:
        G_ref, G_abs = fr.gram_ref(phi, m)
        gg = fr.proj_gamma("phi_gram", ld, npix)
        _within("k_phi_gram", case, "G", res["gram"], G_ref, gg * G_abs, gg)
        G = res["gram"]
    for r, x in enumerate(xs):
        what = "c[%d]" % r
        # ---- projection
        if not res["given_c"]:
            c_ref, c_abs = fr.proj_ref(phi, x, pix0, pix1)
            g = fr.proj_gamma(pk[r], min(ld, 256), npix)
            _within("k_" + pk[r], case, what, res["c"][r], c_ref[:m], g * c_abs[:m], g)
        # ---- apply, from the call's own c
        if wide:
            w64 = np.concatenate([fr.weights(mode, lam[q:q + 256], res["c"][r][q:q + 256], res["filter_pow"])[0] for q in range(0, m, 256)])
            dw = 4 * fr.E * np.abs(w64)
        else:
            w64, dw = fr.weights(mode, lam, res["c"][r], res["filter_pow"], G=G)
        grey_kernel = fmt == "u8"
        corr_ref, bound = fr.apply_ref(phi, m, w64, dw, gain, ysub, x, pix0, pix1, min(ld, 256), f64_kernel=not grey_kernel,
                                       panels=-(-m // 256) if wide else 0)
        xr = np.asarray(x, dtype=np.float64)[pix0:pix1]
        gk = fr.gamma(fr.apply_K(min(ld, 256), -(-m // 256) if wide else 0), fr.U) if grey_kernel else fr.U
        if r >= nch:                                          # a plane: out = v + corr, stored as a float
            kern = "k_apply_filter_signals" if grey_kernel else "k_apply_filter_pix_signals"
            ref = xr + corr_ref
            _within(kern, case, "plane[%d]" % (r - nch), res["sig_out"].reshape(nsig, N)[r - nch, pix0:pix1], ref,
                    bound + fr.stored_f32_slack(ref), gk)
            continue
        if grey_kernel:
            zf, out = res["zf"].reshape(N)[pix0:pix1], res["out"].reshape(N)[pix0:pix1]
            y = res["img"].reshape(N)[pix0:pix1]
            if wide:                                          # no d_corr: the float z resolves the correction to ulp(z)
                ref = xr + corr_ref
                _within("k_filter_accum", case, "zf", zf, ref, bound + fr.stored_f32_slack(ref), gk)
                ok, share = fr.check_int_output(out, y, corr_ref, bound, 255)
                assert ok and share < fr.AMBIGUOUS_CAP, share
                corr = corr_ref
            else:
                corr = res["corr"]
                _within("k_apply_filter", case, "corr", corr, corr_ref, bound, gk)
                assert (zf.view(np.uint32) == fr.zf_rule(y, corr).view(np.uint32)).all()          # bit for bit
                assert (out.astype(np.int64) == fr.out_rule(y, corr, 255)).all()                  # exactly, every pixel
            if vacuity and mode == fr.REFERENCE:
                moved, clamped = (out != y).mean(), int((out == 255).sum())
                print("%s: moved %.3f, at 255: %d, negative corrections %.3f" % (case, moved, clamped, (corr < 0).mean()))
                assert moved > 0.8 and clamped >= 3
                # floor against truncation shows at negative fractional corrections: the full-width cases hold them (with fewer
                # columns the constant column's lam = 1 / (m + 1) lifts every correction above zero)
                assert m < ld or ((corr < 0) & (corr != np.floor(corr))).any()
            continue
        kern = "k_apply_filter_pix_signals" if nsig else "k_apply_filter_pix"
        ref = xr + corr_ref
        zf = res["zf"].reshape(nch, N)[r, pix0:pix1]
        _within(kern, case, "zf[%d]" % r, zf, ref, bound + fr.stored_f32_slack(ref), gk)
        out = res["out"].reshape(N, nch)[pix0:pix1, r]
        if fmt in TOP:
            b = bound + (fr.U * np.abs(corr_ref) if fmt == "rgb8" else 0.0)    # rgb8: the f64 correction is rounded to f32 before the floor
            ok, share = fr.check_int_output(out, xr, corr_ref, b, TOP[fmt])
            print("%s %s[%d]: ambiguous share %.2e" % (case, fmt, r, share))
            assert ok and share < fr.AMBIGUOUS_CAP
            if vacuity and mode == fr.REFERENCE:
                assert (out != xr).mean() > 0.8 and (out == TOP[fmt]).any() and (out == 0).any()
        else:
            _within(kern, case, "out[%d]" % r, out, ref, bound + fr.stored_f32_slack(ref), gk)
            if vacuity and mode == fr.REFERENCE:
                assert np.median(np.abs(corr_ref) / np.maximum(bound, 1e-300)) > 1e4 and (xr < 0).any() and np.abs(xr).max() > 1000


# ---- grey guide --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", fr.TINY, ids=ID)
def test_tiny_grey_guide_every_width(ctx, shape):
    res = _run(ctx, "u8", shape)
    _verify(res, "tiny-" + ID(shape))
    if shape[3] < shape[2]:       # a finite sentinel in Phi's padded columns changes no bit against zero padding
        pad = _run(ctx, "u8", shape, pad=0.37)
        for k in ("out", "zf", "corr"):
            assert (res[k].view(np.uint8) == pad[k].view(np.uint8)).all(), k
        assert (res["c"].view(np.uint64) == pad["c"].view(np.uint64)).all()


@pytest.mark.parametrize("mode,filter_pow", [(fr.REFERENCE, 2), (fr.POC, 1), (fr.SMOOTH, 1), (fr.SHARPEN, 1)],
                         ids=["reference-pow2", "poc", "smooth", "sharpen"])
@pytest.mark.parametrize("shape", [fr.TINY[0], fr.TINY[7]], ids=ID)
def test_tiny_grey_guide_every_mode(ctx, shape, mode, filter_pow):
    res = _run(ctx, "u8", shape, mode=mode, filter_pow=filter_pow)
    _verify(res, "tiny-%s-mode%d-pow%d" % (ID(shape), mode, filter_pow), vacuity=False)
    if mode == fr.POC:            # drives every 8-bit output to 0: its corr and zf are what the case checks
        assert (res["out"] == 0).all() and (res["corr"] < -100).all()
    else:
        assert np.unique(res["out"]).size > 16


@pytest.mark.parametrize("shape", fr.STRIDE, ids=ID)
def test_grid_stride_pass_of_the_grey_kernels(ctx, shape):
    res = _run(ctx, "u8", shape)
    assert res["info"]["grid_strided"] == 1 and res["info"]["apply_blocks"] == fr.MAX_BLOCKS
    _verify(res, "stride-" + ID(shape))


@pytest.mark.parametrize("mode", [fr.SMOOTH, fr.SHARPEN], ids=["smooth", "sharpen"])
def test_smoothing_modes_at_a_stride_shape(ctx, mode):
    """The cancellation in Phi w is where the grey kernel's f32 dot is weakest: the record says how close it comes to its bound."""
    shape = fr.STRIDE[2]
    res = _run(ctx, "u8", shape, mode=mode)
    _verify(res, "stride-%s-mode%d" % (ID(shape), mode), vacuity=False)
    assert np.unique(res["out"]).size > 16


@pytest.mark.parametrize("shape", [fr.TINY[0], fr.STRIDE[1]], ids=ID)
def test_row_ranges_with_a_given_projection(ctx, shape):
    w, h, ld, m = shape
    full = _run(ctx, "u8", shape)
    inner = (20, 30) if h < 100 else (101, 230)
    assert (inner[0] * w) % 1024 != 0
    parts = np.zeros(m)
    for rows in ((0, 1), (h - 1, h), inner):
        res = _run(ctx, "u8", shape, rows=rows, c_in=np.ascontiguousarray(full["c"]))
        assert (res["c"].view(np.uint64) == full["c"].view(np.uint64)).all()
        _verify(res, "rows-%s-%d-%d" % ((ID(shape),) + rows), vacuity=False)
        p0, p1 = res["pix"]
        for k in ("out", "zf"):   # the same weights: the range's pixels carry the full call's bits
            assert (res[k].reshape(-1)[p0:p1] == full[k].reshape(-1)[p0:p1]).all()
        assert (res["corr"] == full["corr"][p0:p1]).all()
    # the projections of three disjoint ranges, summed on the host, match the full one within the bound
    cuts = (0, inner[0], inner[1], h)
    for a, b in zip(cuts[:-1], cuts[1:]):
        res = _run(ctx, "u8", shape, rows=(a, b))
        _verify(res, "rows-own-c-%s-%d-%d" % (ID(shape), a, b), vacuity=False)
        parts = parts + res["c"][0]
    c_ref, c_abs = fr.proj_ref(full["phi"], full["img"].ravel(), 0, w * h)
    g = fr.proj_gamma("phi_t_y", ld, w * h)
    _within("k_phi_t_y", "rows-sum-" + ID(shape), "c", parts, c_ref[:m], (g + 4 * fr.E) * c_abs[:m], g)


@pytest.mark.parametrize("shape", fr.WIDE, ids=ID)
def test_wide_phi_in_two_panels(ctx, shape):
    res = _run(ctx, "u8", shape)
    assert res["info"]["panels"] == 2 and res["info"]["grid_strided"] == int(shape[0] * shape[1] > 4 * fr.MAX_BLOCKS)
    _verify(res, "wide-" + ID(shape))
    pad = _run(ctx, "u8", shape, pad=0.37)    # the second panel's 212 padded columns hold a sentinel: no bit changes
    assert (res["out"] == pad["out"]).all() and (res["zf"].view(np.uint32) == pad["zf"].view(np.uint32)).all()


# ---- planes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [fr.REFERENCE, fr.SMOOTH], ids=["reference", "smooth"])
@pytest.mark.parametrize("shape", [fr.TINY[0], fr.TINY[5], fr.STRIDE[0]], ids=ID)
def test_planes_of_a_grey_guide(ctx, shape, mode):
    w, h = shape[:2]
    sig = fr.planes(4, w, h)
    four = _run(ctx, "u8", shape, mode=mode, sig=sig)
    _verify(four, "planes4-%s-mode%d" % (ID(shape), mode), vacuity=False)
    one = _run(ctx, "u8", shape, mode=mode, sig=sig[:1])
    _verify(one, "planes1-%s-mode%d" % (ID(shape), mode), vacuity=False)
    # a plane's output bits do not depend on the planes beside it; the guide's do not depend on the planes
    assert (one["sig_out"][0].view(np.uint32) == four["sig_out"][0].view(np.uint32)).all()
    assert (one["out"] == four["out"]).all() and (one["corr"].view(np.uint32) == four["corr"].view(np.uint32)).all()
    moved = np.abs(four["sig_out"] - sig).reshape(4, -1).max(axis=1)
    assert (moved > 1e-2).all()               # the filter moves the planes, by far more than any bound here


def test_planes_under_a_row_range(ctx):
    """The plane stride is N, not the length of the range."""
    shape = fr.TINY[0]
    w, h = shape[:2]
    sig = fr.planes(2, w, h)
    res = _run(ctx, "u8", shape, sig=sig, rows=(20, 30))
    _verify(res, "planes2-rows-" + ID(shape), vacuity=False)


# ---- the pixel formats ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsig", [0, 2], ids=["plain", "planes2"])
@pytest.mark.parametrize("shape", [fr.TINY[0], fr.TINY[7], fr.STRIDE[2]], ids=ID)
@pytest.mark.parametrize("fmt", ["rgb8", "u16", "f32", "rgbf32"])
def test_pixel_formats(ctx, fmt, shape, nsig):
    w, h = shape[:2]
    sig = fr.planes(nsig, w, h) if nsig else None
    res = _run(ctx, fmt, shape, sig=sig)
    if shape in fr.STRIDE:
        assert res["info"]["grid_strided"] == 1
    _verify(res, "%s-%s-%s" % (fmt, "planes%d" % nsig if nsig else "plain", ID(shape)))
    if fmt == "u16":
        assert res["img"].min() == 0 and res["img"].max() == 65535


@pytest.mark.parametrize("fmt", ["rgb8", "u16"])
def test_pixel_formats_in_smoothing_mode_under_a_row_range(ctx, fmt):
    shape = fr.TINY[2]
    w, h = shape[:2]
    res = _run(ctx, fmt, shape, mode=fr.SMOOTH, rows=(20, 30), sig=fr.planes(1, w, h))
    _verify(res, "%s-smooth-rows-%s" % (fmt, ID(shape)), vacuity=False)


# ---- NaN, refusals -------------------------------------------------------------------------------------------------------------------
def test_a_nan_row_of_phi_with_a_clean_projection(ctx):
    shape = fr.TINY[0]
    w, h, ld, m = shape
    clean = _run(ctx, "u8", shape)
    phi = clean["phi"].copy()
    bad_px = 1234
    phi[bad_px, 5] = np.nan
    res = _run(ctx, "u8", shape, phi=phi, c_in=np.ascontiguousarray(clean["c"]))
    assert res["out"].reshape(-1)[bad_px] == 0 and np.isnan(res["corr"][bad_px])
    keep = np.arange(w * h) != bad_px
    assert (res["out"].reshape(-1)[keep] == clean["out"].reshape(-1)[keep]).all()
    assert (res["corr"].view(np.uint32)[keep] == clean["corr"].view(np.uint32)[keep]).all()
    assert (res["zf"].reshape(-1).view(np.uint32)[keep] == clean["zf"].reshape(-1).view(np.uint32)[keep]).all()


def _refused(ctx, status, fmt, shape, **kw):
    """A refusal: the status, a reason from glf_ctx_last_error, and every sentinel-filled output untouched."""
    w, h, ld, m = shape
    nch = fr.CHANNELS[fmt]
    phi_np, lam = _inputs(shape)
    mat = kw.pop("mat", None) or _mat(ctx, phi_np, m, shape + (0.0,))
    img = kw.pop("img", None)
    img = fr.guide(fmt, w, h) if img is None else img
    sig = kw.pop("sig", None)
    out0 = np.full((h, w, nch) if nch == 3 else (h, w), INT_SENTINEL.get(fmt, 0), dtype=OUT_DTYPE[fmt])
    d_out, d_zf = _dev(ctx, out0), _dev(ctx, np.full((nch, h, w), SENTINEL, dtype=np.float32))
    d_corr = _dev(ctx, np.full(w * h, SENTINEL, dtype=np.float32)) if kw.pop("corr", False) else None
    d_sig = None if sig is None else _dev(ctx, sig)
    d_sig_out = None if sig is None else _dev(ctx, np.full(sig.shape, SENTINEL, dtype=np.float32))
    c_out, gram = np.full((nch + (0 if sig is None else sig.shape[0]), m), SENTINEL), np.full((m, m), SENTINEL)
    with pytest.raises(glf.GlfError) as e:
        ctx.Filter_ex(PIX[fmt], _dev(ctx, img), mat, lam, sig=d_sig, sig_out=d_sig_out, c_out=c_out, gram_out=gram, out=d_out, zf=d_zf,
                      corr=d_corr, **kw)
    assert e.value.status == status, str(e.value)
    assert len(str(e.value).split("Filter_ex ", 1)[-1].strip()) > 8, str(e.value)
    assert (d_out.cpu().numpy() == out0).all() and (d_zf.cpu().numpy() == SENTINEL).all()
    assert (c_out == SENTINEL).all() and (gram == SENTINEL).all()
    assert d_corr is None or (d_corr.cpu().numpy() == SENTINEL).all()
    assert d_sig_out is None or (d_sig_out.cpu().numpy() == SENTINEL).all()


def test_refusals_leave_every_output_untouched(ctx):
    shape = fr.TINY[0]
    w, h, ld, m = shape
    phi_np, _ = _inputs(shape)
    first = _mat(ctx, phi_np, m)
    first.row_order = glf.ROWS_SAMPLE_FIRST
    over = _mat(ctx, phi_np, m)
    over.cols = ld + 1
    try:
        _refused(ctx, glf.ERR_INVALID, "u8", shape, mat=first)                                   # sample-first Phi
        _refused(ctx, glf.ERR_INVALID, "u8", shape, mat=over)                                    # m > ld
    finally:
        over.cols = m
        ctx.destroy(first, over)
    for rows in ((5, 5), (7, 3), (0, h + 1)):                                                    # a bad row range
        _refused(ctx, glf.ERR_INVALID, "u8", shape, rows=rows)
    five = np.zeros((glf.MAX_SIGNALS + 1, h, w), dtype=np.float32)
    _refused(ctx, glf.ERR_INVALID, "u8", shape, sig=five)                                        # nsig out of range
    _refused(ctx, glf.ERR_INVALID, "rgb8", shape, corr=True)                                     # d_corr with a non-grey guide
    bad = fr.guide("f32", w, h).copy()
    bad[11, 13] = np.nan
    _refused(ctx, glf.ERR_INVALID, "f32", shape, img=bad)                                        # a float guide holding NaN
    bad[11, 13] = np.inf
    _refused(ctx, glf.ERR_INVALID, "f32", shape, img=bad)
    _refused(ctx, glf.ERR_UNSUPPORTED, "u8", shape, filter_mode=fr.SHARPEN, rows=(3, 9))         # sharpening needs all rows' Gram matrix
    wide = fr.WIDE[0]
    _refused(ctx, glf.ERR_UNSUPPORTED, "u8", wide, sig=fr.planes(1, w, h))                       # planes with wide ld
    _refused(ctx, glf.ERR_UNSUPPORTED, "u16", wide)                                              # (a 16-bit guide's values are planes)
    _refused(ctx, glf.ERR_UNSUPPORTED, "u8", wide, filter_mode=fr.SHARPEN)


def test_compute_result_from_laplacian_is_the_stage_call_with_its_defaults(ctx):
    shape = fr.TINY[1]
    w, h, ld, m = shape
    res = _run(ctx, "u8", shape)
    phi_np, lam = _inputs(shape)
    Pi = ctx.diag_from_numpy(lam.astype(np.float32))
    out, zf = ctx.ComputeResultFromLaplacian(ctx.to_device(res["img"]), _mat(ctx, phi_np, m, shape + (0.0,)), Pi, gain=3.0)
    ctx.destroy(Pi)
    # Pi travels as f32: the stage call with lam rounded the same way gives the same bits
    lam32 = lam.astype(np.float32).astype(np.float64)
    d_out, d_zf = _dev(ctx, np.zeros((h, w), np.uint8)), _dev(ctx, np.zeros((1, h, w), np.float32))
    ctx.Filter_ex(glf.PIX_U8, ctx.to_device(res["img"]), _mat(ctx, phi_np, m, shape + (0.0,)), lam32, out=d_out, zf=d_zf)
    assert (out.cpu().numpy() == d_out.cpu().numpy()).all()
    assert (zf.cpu().numpy().view(np.uint32) == d_zf.cpu().numpy().reshape(h, w).view(np.uint32)).all()


# ---- the whole path: c from the Nystroem forms' epilogue ------------------------------------------------------------------------------
# form -> (tuning, contraction, nystroem_path the run must report)
PATH_FORMS = {
    "direct_f32": (dict(NYS_PATH="direct"), glf.CONTRACT_F32_MFMA, 0),
    "direct_f16s": (dict(NYS_PATH="direct", NYS_NO_LUT="1"), glf.CONTRACT_F16_SPLIT, 0),
    "lut": (dict(NYS_PATH="direct"), glf.CONTRACT_F16_SPLIT, 0),
    "grid": (dict(NYS_PATH="grid"), glf.CONTRACT_F16_SPLIT, 1),
    "rank": (dict(NYS_PATH="rank"), glf.CONTRACT_F16_SPLIT, 3),
    "band": (dict(NYS_PATH="band", NO_FUSED_FILTER="1"), glf.CONTRACT_F16_SPLIT, 4),
}
# (shape of nystroem_ref.SHAPES, eigenpairs): ld 32 on both, ld 128 on the one with samples enough. The band form takes ld 32 or 64;
# the table-driven generation runs where nystroem_ref.lut_runs says so (elsewhere that launch is direct_f16s' kernel).
PATH_CASES = [(form, name, m) for name, m in (("tiny", 20), ("lut", 20), ("lut", 100)) for form in sorted(PATH_FORMS)
              if not (form == "band" and m > 64) and not (form == "lut" and not nref.lut_runs(name, 32 if m <= 32 else 128))]


@pytest.mark.parametrize("form,name,m", PATH_CASES, ids=lambda v: str(v))
def test_whole_path_c_corr_and_out_per_nystroem_form(ctx, form, name, m):
    """One captured run: the captured c against float64 Phi_cap^T y under the bound of the form's epilogue and sum_rows, the captured
    corr against the float64 apply of the captured Phi and c, out and zf exactly to their rules."""
    w, h, samples, seed, h_loc = nref.SHAPES[name][:5]
    ld = 32 if m <= 32 else 128
    tuning, contraction, path = PATH_FORMS[form]
    img = glf.synth_image(w, h, seed=seed)
    opt = glf.default_options(num_samples=samples, num_eigvals=m, h_loc=h_loc, epsilon=0.1)
    ctx.reset_tuning()
    ctx.set_tuning(**tuning)
    ctx.set_contraction(contraction)
    try:
        out, zf, info = ctx.image_processing(ctx.to_device(img), opt, want_float=True, capture=True)
    finally:
        ctx.reset_tuning()
        ctx.set_contraction(glf.CONTRACT_F16_SPLIT)
    cap = info["capture"]
    assert (info["nystroem_path"], info["filter_fused"], info["m"], cap["ld"]) == (path, 0, m, ld), info
    N, p = w * h, info["p"]
    phi = cap["phi"].cpu().numpy()
    y = img.ravel()
    case = "path-%s-%s-ld%d" % (form, name, ld)
    c_ref, c_abs = fr.proj_ref(phi, y, 0, N)
    g = fr.nystroem_c_gamma(form, ld, w, N, p)
    _within("nystroem_c_" + form, case, "c", cap["c"], c_ref[:m], g * c_abs[:m], g)
    lam = info["eigvals"]
    w64, dw = fr.weights(fr.REFERENCE, lam, cap["c"])
    corr_ref, bound = fr.apply_ref(phi, m, w64, dw, 3.0, 0.0, y, 0, N, ld)
    corr = cap["corr"].cpu().numpy()
    _within("k_apply_filter", case, "corr", corr, corr_ref, bound, fr.gamma(fr.apply_K(ld), fr.U))
    assert (zf.cpu().numpy().reshape(-1).view(np.uint32) == fr.zf_rule(y, corr).view(np.uint32)).all()
    assert (out.cpu().numpy().reshape(-1).astype(np.int64) == fr.out_rule(y, corr, 255)).all()
