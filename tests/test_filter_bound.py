"""The derived bounds of tests/filter_ref.py against a numpy emulation of k_phi_t_y, k_apply_filter and the panel form in their exact
operation order, on the shapes tests/test_gpu_filter.py runs; the share of pixels whose floor is in doubt under the reference alone;
and the seeded defects, each rejected by a named case (or shown to be invisible, with the reason). CPU only.

Seeded defect                                              rejected by
the last partial 1024-block of the projection is dropped   tiny (53 x 37: 1961 = 1024 + 937 pixels), the projection bound
pixels beyond 8192 x (256 / (LD / 4)) are not written      every stride shape: the last N - 8192 ppb pixels stay unwritten
the shuffle tree is one level short                        tiny at every ld, the apply bound
floor is replaced by truncation                            tiny ld 32: negative fractional corrections give out + 1
the clamp at 255 is missing (the value wraps)              tiny ld 32 at gain 3: clamped pixels wrap to small values
the plane stride is pix1 - pix0 instead of N               rows (inner range of the tiny shape), second plane
the weights of the padded columns are live                 tiny m = ld - 12 with a finite sentinel in Phi's padded columns
ysub is applied to the guide but not to the planes         tiny, smoothing mode with planes
the second panel's weights take the first panel's lam      wide (53 x 37, m = 300)
The first plane (k = 0) cannot see the stride defect: k N = k (pix1 - pix0) = 0. That is asserted too."""
import numpy as np
import pytest

import filter_ref as fr

_CACHE = {}
SENTINEL = -12345.5


def _case(w, h, ld, m, pad=0.0):
    key = (w, h, ld, m, pad)
    if key not in _CACHE:
        _CACHE[key] = (fr.make_phi(w, h, m, ld, pad=pad), fr.image(w, h), fr.lam_ramp(m))
    return _CACHE[key]


def _grey(w, h, ld, m, mode=fr.REFERENCE, gain=3.0, rows=None, contract=False, defect=None, pad=0.0, live_pad=False):
    """The emulated grey route over a row range: (c, c_ref, cbound, corr, corr_ref, bound, y)."""
    phi, img, lam = _case(w, h, ld, m, pad)
    r0, r1 = (0, h) if rows is None else rows
    pix0, pix1 = r0 * w, r1 * w
    c = fr.emu_phi_t_y(phi, img, pix0, pix1, defect=defect)
    c_ref, cabs = fr.proj_ref(phi, img, pix0, pix1)
    cb = fr.proj_gamma("phi_t_y", ld, pix1 - pix0) * cabs
    g, ys = fr.filter_gain(mode, gain), fr.filter_ysub(mode)
    w64, dw = fr.weights(mode, lam, c[:m])
    w32 = np.zeros(ld, dtype=np.float32)
    w32[:m] = w64.astype(np.float32)
    if live_pad:                                    # the seeded defect: the rule runs over all ld columns
        w32[m:] = (c[m:] * 0.5).astype(np.float32)
    corr = fr.emu_apply(phi, w32, img, g, ys, pix0, pix1, contract=contract, defect=defect)
    corr_ref, bound = fr.apply_ref(phi, m, w64, dw, g, ys, img, pix0, pix1, ld)
    return c, c_ref, cb, corr, corr_ref, bound, img.ravel()[pix0:pix1]


@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("shape", fr.TINY + fr.STRIDE, ids=lambda s: "%dx%d-ld%d-m%d" % s)
def test_the_emulated_grey_kernels_meet_their_bounds(shape, contract):
    c, c_ref, cb, corr, corr_ref, bound, y = _grey(*shape, contract=contract)
    m = shape[3]
    worst_c, ok_c = fr.check(c[:m], c_ref[:m], cb[:m])
    worst, ok = fr.check(corr, corr_ref, bound)
    print("c: %.3f of its bound; corr: %.3f of its bound" % (worst_c, worst))
    assert ok_c and ok
    assert worst_c > 1e-4 and worst > 1e-3           # (a bound a thousand times too wide would say nothing)
    out = fr.out_rule(y, corr, 255)
    print("moved %.3f, clamped at 255: %d" % ((out != y).mean(), (out == 255).sum()))
    assert (out != y).mean() > 0.8 and (out == 255).sum() >= 3                                # the case is not vacuous


@pytest.mark.parametrize("mode", [fr.POC, fr.SMOOTH])
def test_the_emulated_grey_kernels_meet_their_bounds_in_the_other_modes(mode):
    for shape in (fr.TINY[0], fr.STRIDE[3]):
        c, c_ref, cb, corr, corr_ref, bound, y = _grey(*shape, mode=mode)
        assert fr.check(corr, corr_ref, bound)[1]


@pytest.mark.parametrize("shape", [fr.TINY[0], fr.STRIDE[1]], ids=lambda s: "%dx%d-ld%d-m%d" % s)
def test_the_emulated_grey_kernels_meet_their_bounds_under_row_ranges(shape):
    w, h, ld, m = shape
    inner = (20, 30) if h < 100 else (101, 230)
    assert (inner[0] * w) % 1024 != 0                # the range's first pixel is no multiple of a projection block
    total, cuts = np.zeros(ld), (0, inner[0], inner[1], h)
    thirds = tuple(zip(cuts[:-1], cuts[1:]))
    for rows in ((0, 1), (h - 1, h)) + thirds:
        c, c_ref, cb, corr, corr_ref, bound, y = _grey(w, h, ld, m, rows=rows)
        assert fr.check(c[:m], c_ref[:m], cb[:m])[1] and fr.check(corr, corr_ref, bound)[1], rows
        if rows in thirds:
            total = total + c
    # the projections of three disjoint ranges, summed on the host, match the full one within the bound
    phi, img, _ = _case(w, h, ld, m)
    full_ref, full_abs = fr.proj_ref(phi, img, 0, w * h)
    assert fr.check(total[:m], full_ref[:m], (fr.proj_gamma("phi_t_y", ld, w * h) + 4 * fr.E) * full_abs[:m])[1]


@pytest.mark.parametrize("shape", fr.WIDE, ids=lambda s: "%dx%d-ld%d-m%d" % s)
def test_the_emulated_panel_form_meets_its_bound(shape):
    w, h, ld, m = shape
    phi, img, lam = _case(w, h, ld, m)
    N = w * h
    c = np.concatenate([fr.emu_phi_t_y(np.ascontiguousarray(phi[:, q * 256:(q + 1) * 256]), img, 0, N) for q in range(ld // 256)])
    c_ref, cabs = fr.proj_ref(phi, img, 0, N)
    assert fr.check(c[:m], c_ref[:m], fr.proj_gamma("phi_t_y", 256, N) * cabs[:m])[1]
    w64, dw = fr.weights(fr.REFERENCE, lam, c[:m])
    corr = fr.emu_panels(phi, m, fr.panel_weights(fr.REFERENCE, lam, c, m), img, 3.0, 0.0, 0, N)
    corr_ref, bound = fr.apply_ref(phi, m, w64, dw, 3.0, 0.0, img, 0, N, 256, panels=2)
    assert fr.check(corr, corr_ref, bound)[1]
    # seeded: the second panel's weights from the first panel's lam; the first flag stuck at 1
    bad = fr.emu_panels(phi, m, fr.panel_weights(fr.REFERENCE, lam, c, m, lam_from_first=True), img, 3.0, 0.0, 0, N)
    assert not fr.check(bad, corr_ref, bound)[1]
    stuck = fr.emu_panels(phi, m, fr.panel_weights(fr.REFERENCE, lam, c, m), img, 3.0, 0.0, 0, N, stuck_first=True)
    assert not fr.check(stuck, corr_ref, bound)[1]


@pytest.mark.parametrize("fmt,top", [("rgb8", 255), ("u16", 65535)])
@pytest.mark.parametrize("shape", [fr.TINY[0], fr.TINY[7], fr.STRIDE[2]], ids=lambda s: "%dx%d-ld%d-m%d" % s)
def test_the_ambiguous_share_of_the_integer_formats_is_under_the_cap(shape, fmt, top):
    w, h, ld, m = shape
    phi, _, lam = _case(w, h, ld, m)
    g = fr.guide(fmt, w, h)
    N = w * h
    for k in range(fr.CHANNELS[fmt]):
        x = g.reshape(N, -1)[:, k]
        c_ref, _ = fr.proj_ref(phi, x, 0, N)
        w64, dw = fr.weights(fr.REFERENCE, lam, c_ref[:m])
        corr_ref, bound = fr.apply_ref(phi, m, w64, dw, 3.0, 0.0, x, 0, N, ld, f64_kernel=True)
        if fmt == "rgb8":
            bound = bound + fr.U * np.abs(corr_ref)
        share = float(fr.ambiguous(corr_ref, bound).mean())
        print(fmt, k, "ambiguous share %.2e" % share)
        assert share < fr.AMBIGUOUS_CAP
        out = fr.out_rule(x, corr_ref, top)
        assert (out != x).mean() > 0.9 and (out == top).any()


def test_each_seeded_defect_is_rejected():
    w, h, ld, m = fr.TINY[0]
    c, c_ref, cb, corr, corr_ref, bound, y = _grey(w, h, ld, m)
    good_out = fr.out_rule(y, corr, 255)
    # the last partial block of the projection dropped: tiny
    cd = _grey(w, h, ld, m, defect="drop_last_block")[0]
    assert not fr.check(cd[:m], c_ref[:m], cb[:m])[1]
    # the shuffle tree one level short: tiny at every ld
    for shape in fr.TINY[::2]:
        _, _, _, cs, cr, b, _ = _grey(*shape, defect="short_tree")
        assert not fr.check(cs, cr, b)[1], shape
    # pixels beyond 8192 x ppb not written: every stride shape
    for shape in fr.STRIDE:
        cn = _grey(*shape, defect="no_stride")[3]
        assert np.isnan(cn).sum() == shape[0] * shape[1] - fr.MAX_BLOCKS * fr.ppb(shape[2]) > 0
    # floor replaced by truncation
    trunc = np.clip(y.astype(np.int64) + np.trunc(corr).astype(np.int64), 0, 255)
    assert ((corr < 0) & (corr != np.floor(corr))).any() and (trunc != good_out).any()
    # the clamp at 255 missing: the value wraps
    wrap = (y.astype(np.int64) + np.floor(corr).astype(np.int64)) % 256
    assert (good_out == 255).any() and (wrap != good_out).any()
    # the weights of the padded columns live: m = ld - 12, a finite sentinel in Phi's padded columns
    w2, h2, ld2, m2 = fr.TINY[1]
    zero = _grey(w2, h2, ld2, m2)[3]
    same = _grey(w2, h2, ld2, m2, pad=0.37)[3]
    live = _grey(w2, h2, ld2, m2, pad=0.37, live_pad=True)[3]
    assert (zero.view(np.uint32) == same.view(np.uint32)).all()          # zero weights: the padding changes no bit
    assert (zero.view(np.uint32) != live.view(np.uint32)).any()


def test_the_plane_defects_are_rejected():
    w, h, ld, m = fr.TINY[0]
    phi, img, lam = _case(w, h, ld, m)
    N = w * h
    sig = fr.planes(2, w, h)
    r0, r1 = 20, 30                                   # first pixel 1060: no multiple of 1024
    pix0, pix1 = r0 * w, r1 * w
    for mode in (fr.REFERENCE, fr.SMOOTH):
        g, ys = fr.filter_gain(mode, 3.0), fr.filter_ysub(mode)
        for k in range(2):
            c_ref, _ = fr.proj_ref(phi, sig[k], 0, N)
            w64, dw = fr.weights(mode, lam, c_ref[:m])
            w32 = w64.astype(np.float32)
            corr = fr.emu_apply(phi, w32, sig[k], g, ys, pix0, pix1)
            corr_ref, bound = fr.apply_ref(phi, m, w64, dw, g, ys, sig[k], pix0, pix1, ld)
            assert fr.check(corr, corr_ref, bound)[1]
            out_ref = sig[k].ravel()[pix0:pix1] + corr_ref
            # the plane stride pix1 - pix0 instead of N: plane k is read, and written, at k (pix1 - pix0) + px. (With ysub = 1 the
            # value read cancels: out = v + (Phi w - v); the write position still shows.)
            flat = sig.reshape(-1)
            at = k * (pix1 - pix0) + np.arange(pix0, pix1)
            bad = flat[at] + fr.emu_apply(phi, w32, np.concatenate([np.zeros(pix0, np.float32), flat[at]]), g, ys, pix0, pix1)
            buf = np.full(2 * N, SENTINEL)
            buf[at] = bad
            want = np.full(2 * N, SENTINEL)
            want[k * N + pix0:k * N + pix1] = out_ref
            tol = np.zeros(2 * N)
            tol[k * N + pix0:k * N + pix1] = bound + fr.stored_f32_slack(out_ref)
            rejected = not fr.check(buf, want, tol)[1]
            assert rejected == (k > 0)                # invisible by design for the first plane: k N = k (pix1 - pix0) = 0
            if mode == fr.SMOOTH:                     # ysub applied to the guide but not to the planes
                no_ysub = fr.emu_apply(phi, w32, sig[k], g, 0.0, pix0, pix1)
                assert not fr.check(no_ysub, corr_ref, bound)[1]
