"""The Nystroem extension Phi_B = L_B^T (phi_A Pi^-1) in every form, through glf_Nystroem_ex (the stage call, with the window, the row
range and the report of the whole path), against a float64 product with a componentwise bound derived from each form's arithmetic.
Needs an MI355X: -m gpu.

Reference and bound: tests/nystroem_ref.py (its docstring holds K, s, c and the dropped parts a per form, with the code each comes
from; its SHAPES table says what each shape is for). Grey guides and the other formats alike: the kernel's definition in float64
(tests/u16_ref.py, tests/rgb_ref.py) in chunks of image rows; the scale s of L_B is the GPU's own (the degree stage has its tests).
The block (nystroem_ref.make_block): m = ld - 5 real columns of magnitudes 2^-30 .. 2^+30, an all-zero column, a column that is zero on
the even samples, unit vectors at the samples 0, 63, 64, p // 2 and p - 1 -- each of those reads one row of K_B entry by entry at every
pixel, against gamma K(x, s_i) |psi_i| plus the form's floor -- and inverse eigenvalues that are powers of two on every other column.
Every element of every non-sample row is compared; where the bound is zero (the zero column, the padding) the result must be zero.
Under the f32 contraction the factored forms do not exist: every form's run must report path 0 and give the direct run's bits.

What these tests cannot see: an error below a form's floor a (for the split-f16 forms 2^-40 of the column's 1-norm: entries of K_B
under 2^-40 are zero pairs by design), and the NLM kernel, the fused band filter and multi-rank runs, which have their own tests.

Set GLF_NYSTROEM_ERROR_JSON to a path to have the largest observed |Phi - Phi_ref| / bound per form and ld written there (a record:
the asserted bound is the derived one)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import nystroem_ref as nref  # noqa: E402
import pix_cases  # noqa: E402

# form -> (tuning, glf_nystroem_info.path under the split-f16 contraction, form of the bound there)
FORMS = {
    "direct": (dict(NYS_PATH="direct"), 0, "f16s"),
    "direct_nolut": (dict(NYS_PATH="direct", NYS_NO_LUT="1"), 0, "f16s"),
    "grid": (dict(NYS_PATH="grid"), 1, "grid"),
    "grid_noecr": (dict(NYS_PATH="grid", NO_ECR="1"), 1, "grid"),
    "grid_v1": (dict(NYS_PATH="grid", ROWPASS="v1"), 1, "grid"),
    "grid_v1_noecr": (dict(NYS_PATH="grid", ROWPASS="v1", NO_ECR="1"), 1, "grid"),
    "rank": (dict(NYS_PATH="rank"), 3, "rank"),
    "rank_v1": (dict(NYS_PATH="rank", COLPASS="v1"), 3, "rank"),
    "band": (dict(NYS_PATH="band"), 4, "band"),
}
MAIN_FORMS = ["direct", "direct_nolut", "grid", "rank", "band"]
BLOCK_SEED = 31
_RECORD = {}


@pytest.fixture(scope="module", params=["f16s", "f32"])
def ctx(request):
    """Both contraction modes, as in test_gpu_operator.py."""
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = glf.Context(0)
    c.set_contraction(glf.CONTRACT_F16_SPLIT if request.param == "f16s" else glf.CONTRACT_F32_MFMA)
    c.mode = request.param
    c.graphs = {}
    yield c
    for d_img, K_B, L_B in c.graphs.values():
        c.destroy(K_B)
    c.close()


@pytest.fixture(autouse=True)
def _default_kernel_selection(request):
    yield
    if "ctx" in request.fixturenames:
        request.getfixturevalue("ctx").reset_tuning()


@pytest.fixture(scope="module", autouse=True)
def _error_record():
    yield
    path = os.environ.get("GLF_NYSTROEM_ERROR_JSON")
    if path and _RECORD:       # one row per (form of the run / form of the bound, ld)
        agg = {}
        for (form, ld, label), (ratio, g) in sorted(_RECORD.items()):
            a = agg.setdefault((form, ld), dict(form=form, ld=ld, gamma_min=g, gamma_max=g, worst_error_over_bound=-1.0, worst_case=None))
            a["gamma_min"], a["gamma_max"] = min(a["gamma_min"], g), max(a["gamma_max"], g)
            if ratio > a["worst_error_over_bound"]:
                a["worst_error_over_bound"], a["worst_case"] = ratio, label
        what = ("largest observed |Phi - Phi_ref| / (gamma (K_B^T |Psi|) + a) per form (form of the run / form of the bound) and ld over the "
                "shapes and tests of tests/test_gpu_nystroem.py on an MI355X (GLF_NYSTROEM_ERROR_JSON=<this file> python -m pytest "
                "tests/test_gpu_nystroem.py -m gpu); gamma: the derived value asserted (its range over the shapes). A record only.")
        with open(path, "w") as f:
            json.dump(dict(what=what, rows=[agg[k] for k in sorted(agg)]), f, indent=1)


class _Shape:
    pass


_SHAPES, _REFS = {}, {}


def _shape(name):
    """The CPU side of a grey shape: image, samples, the realised grid (asserted against the table)."""
    if name not in _SHAPES:
        w, h, ns, seed, h_loc, p, nr, nc = nref.SHAPES[name]
        r = _Shape()
        r.name, r.w, r.h, r.h_loc, r.h_val, r.kern = name, w, h, h_loc, nref.H_VAL, nref.u16_ref.kernel
        r.img = glf.synth_image(w, h, seed=seed)
        r.idx = glf.Sampling(w, h, ns)
        r.p, r.N = int(r.idx.size), w * h
        assert r.p == p and nref.grid_shape(r.idx, w) == (nr, nc), (name, r.p, nref.grid_shape(r.idx, w))
        r.nr, r.nc, r.kernel = nr, nc, glf.KERNEL_BILATERAL
        _SHAPES[name] = r
    return _SHAPES[name]


def _pix_shape(fmt, name):
    if (fmt, name) not in _SHAPES:
        g = _shape(name)
        r = _Shape()
        r.__dict__.update(g.__dict__)
        r.name = "%s/%s" % (fmt, name)
        r.img, r.kernel, r.h_val, mod = pix_cases.pix_case(fmt, g.w, g.h, nref.SHAPES[name][3])
        r.kern, r.fmt = mod.kernel, fmt
        _SHAPES[(fmt, name)] = r
    return _SHAPES[(fmt, name)]


def _graph(ctx, r):
    """(d_img, K_B, L_B) of a guide on this context, built once."""
    if r.name not in ctx.graphs:
        d_img = ctx.to_device(r.img) if r.img.dtype == np.uint8 and r.img.ndim == 2 else torch.from_numpy(np.ascontiguousarray(r.img)).to(ctx.device)
        _, K_B = ctx.ComputeAffinityMatrices(d_img, r.idx, want_KA=False, kernel=r.kernel, h_loc=r.h_loc, h_val=r.h_val)
        L_A, L_B, alpha = ctx.ComputeLaplacianMatrix(None, K_B)
        ctx.destroy(L_A)
        ctx.graphs[r.name] = (d_img, K_B, L_B)
    return ctx.graphs[r.name]


def _reference(r, s, seed=BLOCK_SEED):
    """The float64 side of a shape at 256 columns, computed once per (guide, scale, block) and left unchanged: every narrower ld
    takes its leading columns."""
    key = (r.name, float(s), seed)
    if key not in _REFS:
        phi_A, pinv = nref.make_block(r.p, nref.FULL_LD, nref.FULL_LD - 5, seed)
        Psi = nref.psi64(phi_A, np.r_[pinv, np.zeros(5, dtype=np.float32)], s)
        _REFS[key] = (Psi, nref.reference(r.img, r.idx, Psi, r.h_loc, r.h_val, kern=r.kern))
    return _REFS[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(ctx, form, L_B, phi_A, pinv, ld, skip=0, rows=None, fill=None, tuning=None):
    """One stage call under a form's tuning: (Phi as stored [N, ld], info)."""
    ctx.reset_tuning()
    ctx.set_tuning(**(FORMS[form][0] if tuning is None else tuning))
    m = pinv.size
    dA, dP = ctx.dense_from_numpy(phi_A[:, :m], ld=ld), ctx.diag_from_numpy(pinv)
    given = None
    if fill is not None:
        given = ctx.dense_from_numpy(fill, ld=ld, row_order=glf.ROWS_SAMPLE_FIRST)
        given.cols = m
    ctx.last_given = given               # (a refusal leaves it to the caller, who looks at its bits)
    try:
        phi, info = ctx.Nystroem_ex(L_B, dA, dP, skip_exact_zeros=skip, rows=rows, phi=given)
    finally:
        ctx.destroy(dA, dP)
    assert (phi.cols, phi.ld, phi.row_order) == (m, ld, glf.ROWS_SAMPLE_FIRST)
    out = ctx.mat_to_numpy(phi, padded=True)
    ctx.destroy(phi)
    ctx.last_given = None
    return out, info


def _expected(ctx, r, form, ld, no_lut=False):
    """(path, form of the bound, lut) a form's run must report at this shape and width."""
    if ctx.mode == "f32":
        return 0, "f32", 0
    tuning, path, bform = FORMS[form]
    lut = int(path == 0 and nref.lut_runs(r.name, ld, no_lut=no_lut or "NYS_NO_LUT" in tuning))
    return path, ("f16s_lut" if lut else bform), lut


def _assert_within(r, bform, Phi, phi_A, pinv, s, ld, label, form, rows=None, fill=None, fmt=None):
    """Every element of the non-sample rows of the range within the bound (exactly zero where it is zero: the zero column, the
    padding); the sample rows phi_A's bits; with a fill, every other row the fill's bits."""
    m = pinv.size
    Psi, ref = _reference(r, s)
    np.testing.assert_array_equal(_bits(Phi[:r.p]), _bits(phi_A[:, :ld]), err_msg="sample rows")
    sel = np.ones(ref.pixels.size, dtype=bool) if rows is None else (ref.pixels >= rows[0] * r.w) & (ref.pixels < rows[1] * r.w)
    g = nref.gamma(bform, r.p, nr=r.nr, nc=r.nc, fmt=fmt)
    B = np.zeros((int(sel.sum()), ld))
    B[:, :m] = nref.bound(bform, g, ref, Psi, cols=slice(0, m))[sel]
    want = np.zeros_like(B)
    want[:, :m] = ref.phi[sel, :m]
    got = Phi[r.p:][sel]
    assert np.isfinite(got).all()
    ratio, ok = nref.check(got, want, B)
    print("%s %s ld %d%s: gamma 2^%.2f, worst |Phi - Phi_ref| / bound %.3f" % (label, form, ld, "" if rows is None else " rows %s" % (rows,), np.log2(g), ratio))
    key = ("%s/%s" % (form, bform), ld, label)
    if ratio > _RECORD.get(key, (-1.0, g))[0]:
        _RECORD[key] = (ratio, g)
    if not ok:
        err = np.abs(got.astype(np.float64) - want)
        bad = np.argwhere(err > B)
        assert bad.size == 0, "%d elements beyond the bound, first (pixel %d, column %d): error %.3e, bound %.3e; worst ratio %.2f" % (
            len(bad), ref.pixels[sel][bad[0][0]], bad[0][1], err[tuple(bad[0])], B[tuple(bad[0])], ratio)
        assert not got[B == 0].any(), "an element whose bound is zero is not exactly zero"
    assert (B[want != 0] > 0).all()
    if fill is not None:
        np.testing.assert_array_equal(_bits(Phi[r.p:][~sel]), _bits(fill[r.p:][~sel]), err_msg="rows outside the range")
    return ratio


def _lds(shape):
    return nref.LDS.get(shape, nref.ALL_LDS)


AGAINST = [(s, f, ld) for s in nref.SHAPES for f in FORMS for ld in _lds(s)]


@pytest.mark.parametrize("shape,form,ld", AGAINST, ids=["%s-%s-%d" % c for c in AGAINST])
def test_against_fp64(ctx, shape, form, ld):
    r = _shape(shape)
    d_img, K_B, L_B = _graph(ctx, r)
    m = ld - 5
    phi_A, pinv = nref.make_block(r.p, ld, m, BLOCK_SEED)
    Phi, info = _run(ctx, form, L_B, phi_A, pinv, ld)
    path, bform, lut = _expected(ctx, r, form, ld)
    assert (info["path"], info["lut"]) == (path, lut), info
    assert info["contraction"] == (glf.CONTRACT_F32_MFMA if ctx.mode == "f32" else glf.CONTRACT_F16_SPLIT)
    assert (info["row0"], info["row1"], info["skipping"]) == (0, r.h, 1 if path == 4 else 0), info
    assert Phi.shape == (r.N, ld)
    _assert_within(r, bform, Phi, phi_A, pinv, L_B.scale, ld, shape, form)
    if ctx.mode == "f32" and form != "direct":       # no factored form under the f32 contraction: the direct kernel's bits
        np.testing.assert_array_equal(_bits(Phi), _bits(_run(ctx, "direct", L_B, phi_A, pinv, ld)[0]))


def test_partial_band_and_windows(ctx):
    """narrow: the kernel's radius is a fraction of the image side, so the band is part of the sample grid and the windowed direct
    kernels pass over chunks. Within the bound, fewer entries evaluated than K_B has, and the same bits as without the window."""
    r = _shape("narrow")
    d_img, K_B, L_B = _graph(ctx, r)
    s_loc = np.log2(np.e) / r.h_loc ** 2
    assert int(np.sqrt(40.5 / s_loc)) + 1 == 27 and int(np.sqrt(151.0 / s_loc)) + 1 == 52
    full = r.p * (r.N - r.p)
    for ld in (32, 64, 128, 256):
        m = ld - 5
        phi_A, pinv = nref.make_block(r.p, ld, m, BLOCK_SEED)
        for form in ("direct", "direct_nolut"):
            path, bform, lut = _expected(ctx, r, form, ld)
            off, info0 = _run(ctx, form, L_B, phi_A, pinv, ld, skip=0)
            on, info1 = _run(ctx, form, L_B, phi_A, pinv, ld, skip=1)
            assert (info0["skipping"], info1["skipping"], info1["path"], info1["lut"]) == (0, 1, 0, lut), (info0, info1)
            assert 0 < info1["entries_evaluated"] < full <= info0["entries_evaluated"], (info0, info1, full)
            _assert_within(r, bform, on, phi_A, pinv, L_B.scale, ld, "narrow/window", form)
            np.testing.assert_array_equal(_bits(on), _bits(off))
        if ctx.mode == "f32":
            continue
        band, info = _run(ctx, "band", L_B, phi_A, pinv, ld)
        assert (info["path"], info["skipping"]) == (4, 1) and 0 < info["entries_evaluated"] < full, info
        _assert_within(r, "band", band, phi_A, pinv, L_B.scale, ld, "narrow/band", "band")
        noskip, info_ns = _run(ctx, "band", L_B, phi_A, pinv, ld, tuning=dict(NYS_PATH="band", BAND_NOSKIP="1"))
        assert (info_ns["path"], info_ns["skipping"]) == (4, 0), info_ns
        np.testing.assert_array_equal(_bits(band), _bits(noskip))


PIX = [(f, s, ld) for f in pix_cases.FORMATS for s in ("tiny", "mid") for ld in (32, 64, 128, 256)]


@pytest.mark.parametrize("fmt,shape,ld", PIX, ids=["%s-%s-%d" % c for c in PIX])
def test_pixel_formats(ctx, fmt, shape, ld):
    """The colour, 16-bit and float guides: entry by entry in f32 (PB = 2, 2, 2, 1 at ld 32 .. 256, always with the window) whatever
    the contraction mode; behind PIX_BAND the band form at ld 32 and 64 under the split-f16 contraction, and the entry-by-entry
    kernel's bits at ld 128 and 256 and under the f32 contraction."""
    r = _pix_shape(fmt, shape)
    d_img, K_B, L_B = _graph(ctx, r)
    m = ld - 5
    phi_A, pinv = nref.make_block(r.p, ld, m, BLOCK_SEED)
    Phi, info = _run(ctx, "direct", L_B, phi_A, pinv, ld, tuning={})
    assert (info["path"], info["contraction"], info["skipping"], info["lut"]) == (0, glf.CONTRACT_F32_MFMA, 1, 0), info
    _assert_within(r, "pix_f32", Phi, phi_A, pinv, L_B.scale, ld, r.name, "entrywise", fmt=fmt)
    band, binfo = _run(ctx, "band", L_B, phi_A, pinv, ld, tuning=dict(NYS_PATH="band", PIX_BAND="1"))
    if ctx.mode == "f16s" and ld <= 64:
        assert (binfo["path"], binfo["contraction"], binfo["skipping"]) == (4, glf.CONTRACT_F16_SPLIT, 1), binfo
        _assert_within(r, "pix_band", band, phi_A, pinv, L_B.scale, ld, r.name, "pix_band")
    else:
        assert (binfo["path"], binfo["contraction"]) == (0, glf.CONTRACT_F32_MFMA), binfo
        np.testing.assert_array_equal(_bits(band), _bits(Phi))


def _row_ranges(r):
    """One image row at either end; a range that starts off any multiple of a workgroup's pixels (128, 256 or 512) and holds no whole
    number of workgroups (they count from the range's first pixel: the last one is ragged); two pairs of adjacent ranges that make
    the image, split at a multiple of 8 image rows and off it."""
    odd = (3, 10)
    assert (odd[0] * r.w) % 128 and ((odd[1] - odd[0]) * r.w) % 128
    k = r.h // 3
    assert k % 8 and (k * r.w) % 64 == 0 and (k // 8 * 8 * r.w) % 64 == 0
    return [(0, 1), (r.h - 1, r.h), odd], [k // 8 * 8, k]


@pytest.mark.parametrize("form", MAIN_FORMS)
@pytest.mark.parametrize("shape", ["mid", "narrow"])
def test_row_ranges(ctx, shape, form):
    """The rows one rank of the sharded whole path owns, written into an existing Phi: inside the range within the bound, outside a
    fill pattern's bits, the sample rows phi_A's. Two adjacent ranges give the full call's bits: an output's sums run over the samples
    in an order that depends on neither the workgroup nor the pass it falls into, and the operand scales come from Psi alone. (The
    splits at a multiple of 64 pixels keep the LUT kernel's rule on pix0 satisfied: both halves run the kernel the full call runs.)
    The band form promises this only for a split at a multiple of its workgroup's 8 image rows (BAND_NW), or where the band is the
    whole grid (mid): a workgroup contracts the union of its rows' bands, two consecutive grid rows per k-step from the union's first
    row on (nystroem_band.inc, "pixel targets"), so a split elsewhere regroups the image rows, pairs other grid rows and rounds in
    another order. There the union of the halves is held to the bound instead."""
    r = _shape(shape)
    d_img, K_B, L_B = _graph(ctx, r)
    ld, m = 64, 59
    phi_A, pinv = nref.make_block(r.p, ld, m, BLOCK_SEED)
    fill = np.full((r.N, ld), -7.25, dtype=np.float32)
    singles, splits = _row_ranges(r)
    path, bform, lut = _expected(ctx, r, form, ld)
    for rows in singles:
        Phi, info = _run(ctx, form, L_B, phi_A, pinv, ld, rows=rows, fill=fill)
        lut_here = int(lut and (rows[0] * r.w) % 64 == 0)
        assert (info["path"], info["row0"], info["row1"], info["lut"]) == (path, rows[0], rows[1], lut_here), info
        _assert_within(r, bform if lut_here == lut else "f16s", Phi, phi_A, pinv, L_B.scale, ld, "%s/rows" % shape, form, rows=rows, fill=fill)
    whole, _ = _run(ctx, form, L_B, phi_A, pinv, ld)
    for k in splits:
        both, info = _run(ctx, form, L_B, phi_A, pinv, ld, rows=(0, k), fill=fill)
        assert (info["path"], info["lut"]) == (path, lut)
        both, info = _run(ctx, form, L_B, phi_A, pinv, ld, rows=(k, r.h), fill=both)
        assert (info["path"], info["lut"]) == (path, lut)
        if path == 4 and shape == "narrow" and k % 8:
            assert not np.array_equal(_bits(both), _bits(whole))          # (the reason above is real: the bits do move)
            _assert_within(r, bform, both, phi_A, pinv, L_B.scale, ld, "%s/halves" % shape, form)
        else:
            np.testing.assert_array_equal(_bits(both), _bits(whole), err_msg="split at image row %d" % k)


@pytest.mark.parametrize("form", list(FORMS))
def test_power_of_two_column_scaling_is_exact(ctx, form):
    """A column of phi_A scaled by 2^k, k = -20 and +17, scales that column of Phi exactly and leaves the others' bits alone: every
    form takes its operand scales per column as powers of two, and nothing here leaves the normal f32 range."""
    r = _shape("edge")
    d_img, K_B, L_B = _graph(ctx, r)
    ld, m = 64, 59
    phi_A, pinv = nref.make_block(r.p, ld, m, BLOCK_SEED)
    e = np.zeros(ld, dtype=int)
    e[10], e[11], e[nref.COL_UNIT0], e[nref.COL_EVEN_ZERO] = -20, 17, 17, -20
    sc = np.ldexp(np.float32(1), e).astype(np.float32)
    Phi, _ = _run(ctx, form, L_B, phi_A, pinv, ld)
    Phis, _ = _run(ctx, form, L_B, phi_A * sc[None, :], pinv, ld)
    assert (np.abs(Phi[r.p:, [10, 11, nref.COL_UNIT0, nref.COL_EVEN_ZERO]]).max(axis=0) > 0).all()
    np.testing.assert_array_equal(_bits(Phis), _bits(Phi * sc[None, :]))


@pytest.mark.parametrize("form", list(FORMS))
def test_a_column_does_not_depend_on_its_neighbours(ctx, form):
    """Every other column of phi_A replaced (other values, other magnitudes, one zeroed): the untouched columns of Phi keep their bits."""
    r = _shape("edge")
    d_img, K_B, L_B = _graph(ctx, r)
    for ld in (32, 128):
        m = ld - 5
        phi_A, pinv = nref.make_block(r.p, ld, m, BLOCK_SEED)
        other, _ = nref.make_block(r.p, ld, m, BLOCK_SEED + 1)
        A2 = phi_A.copy()
        A2[:, 1::2] = other[:, 1::2][:, ::-1]
        A2[:, 5] = 0.0
        Phi, _ = _run(ctx, form, L_B, phi_A, pinv, ld)
        Phi2, _ = _run(ctx, form, L_B, A2, pinv, ld)
        assert not np.array_equal(_bits(Phi[:, 1::2]), _bits(Phi2[:, 1::2]))
        np.testing.assert_array_equal(_bits(Phi[:, 0::2]), _bits(Phi2[:, 0::2]))


def test_more_than_256_columns(ctx):
    """m = 261 at ld = 512: two 256-column panels, the second with 5 real columns. Both within the direct form's bound, the columns
    from 261 on zero, the sample rows phi_A's bits."""
    r = _shape("edge")
    d_img, K_B, L_B = _graph(ctx, r)
    m, ld = 261, 512
    rng = np.random.default_rng(77)
    phi_A = np.zeros((r.p, ld), dtype=np.float32)
    phi_A[:, :m] = (rng.normal(size=(r.p, m)) * 2.0 ** rng.integers(-30, 31, size=m)[None, :]).astype(np.float32)
    phi_A[:, 258] = 0.0
    phi_A[r.p - 1, 258] = 1.0                              # a unit vector in the second panel, at the ragged chunk's last sample
    pinv = rng.uniform(0.5, 2.0, size=m).astype(np.float32)
    Psi = nref.psi64(phi_A[:, :m], pinv, L_B.scale)
    ref = nref.reference(r.img, r.idx, Psi, r.h_loc, r.h_val)
    Phi, info = _run(ctx, "direct", L_B, phi_A, pinv, ld)
    bform = "f32" if ctx.mode == "f32" else "f16s"
    assert (info["path"], info["lut"]) == (0, 0) and Phi.shape == (r.N, ld)
    assert info["entries_evaluated"] >= 2 * r.p * (r.N - r.p)
    np.testing.assert_array_equal(_bits(Phi[:r.p]), _bits(phi_A))
    assert not Phi[:, m:].any()
    g = nref.gamma(bform, r.p)
    for name, cols in (("first", slice(0, 256)), ("second", slice(256, m))):
        ratio, ok = nref.check(Phi[r.p:, cols], ref.phi[:, cols], nref.bound(bform, g, ref, Psi, cols=cols))
        print("edge %s panel: worst |Phi - Phi_ref| / bound %.3f" % (name, ratio))
        _RECORD[("panels/%s" % bform, ld, "edge/%s" % name)] = (ratio, g)
        assert ok, (name, ratio)
    # a row range or a given phi is refused for more than 256 eigenpairs (include/glf.h)
    with pytest.raises(glf.GlfError) as e:
        _run(ctx, "direct", L_B, phi_A, pinv, ld, rows=(0, 4))
    assert e.value.status == glf.ERR_UNSUPPORTED and "256" in str(e.value)


def test_make_psi_and_inverse_diag(ctx):
    """InverseDiagMat within 1 ulp of 1 / x over 2^-60 .. 2^60; a zero column of phi_A and a column with pinv = 0 give exact zeros in
    Phi in every form."""
    rng = np.random.default_rng(5)
    x = (rng.uniform(1.0, 2.0, size=484) * 2.0 ** np.repeat(np.arange(-60, 61), 4)).astype(np.float32)
    x[::7] *= -1.0
    dx = ctx.diag_from_numpy(x)
    inv = ctx.InverseDiagMat(dx)
    y = ctx.mat_to_numpy(inv)
    ctx.destroy(dx, inv)
    exact = 1.0 / x.astype(np.float64)
    assert (np.abs(y.astype(np.float64) - exact) <= np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)).all()
    r = _shape("lut")
    d_img, K_B, L_B = _graph(ctx, r)
    ld, m = 32, 27
    phi_A, pinv = nref.make_block(r.p, ld, m, BLOCK_SEED)
    pinv[8] = 0.0
    for form in FORMS:
        Phi, _ = _run(ctx, form, L_B, phi_A, pinv, ld)
        assert not Phi[r.p:, [nref.COL_ZERO, 8]].any(), form
        assert np.abs(Phi[r.p:, 9]).min() > 0


def test_refusals_leave_phi_untouched(ctx):
    """A bad row range, a given phi of another ld or shape, and m > ld: each names its reason and leaves the given phi's bits alone."""
    r = _shape("tiny")
    d_img, K_B, L_B = _graph(ctx, r)
    ld, m = 32, 27
    phi_A, pinv = nref.make_block(r.p, ld, m, BLOCK_SEED)
    fill = np.full((r.N, ld), 3.5, dtype=np.float32)

    def refused(word, status=glf.ERR_INVALID, **kw):
        with pytest.raises(glf.GlfError) as e:
            _run(ctx, "direct", L_B, phi_A, pinv, ld, **kw)
        assert e.value.status == status and word in str(e.value), str(e.value)
        if ctx.last_given is not None:
            np.testing.assert_array_equal(_bits(ctx.mat_to_numpy(ctx.last_given, padded=True)), _bits(kw["fill"]))
            ctx.destroy(ctx.last_given)

    for rows in ((5, 5), (10, 5), (0, r.h + 1), (r.h, r.h + 2)):
        refused("image rows", rows=rows, fill=fill)
        refused("image rows", rows=rows)
    # a given phi of another ld, of too few rows, in raster order
    dA, dP = ctx.dense_from_numpy(phi_A[:, :m], ld=ld), ctx.diag_from_numpy(pinv)
    for make in (lambda: ctx.dense_from_numpy(np.full((r.N, m), 3.5, dtype=np.float32), ld=64, row_order=glf.ROWS_SAMPLE_FIRST),
                 lambda: ctx.dense_from_numpy(np.full((r.N - 1, m), 3.5, dtype=np.float32), ld=ld, row_order=glf.ROWS_SAMPLE_FIRST),
                 lambda: ctx.dense_from_numpy(np.full((r.N, m), 3.5, dtype=np.float32), ld=ld, row_order=glf.ROWS_RASTER)):
        given = make()
        before = ctx.mat_to_numpy(given, padded=True)
        with pytest.raises(glf.GlfError) as e:
            ctx.Nystroem_ex(L_B, dA, dP, phi=given)
        assert e.value.status == glf.ERR_INVALID and "given phi" in str(e.value), str(e.value)
        np.testing.assert_array_equal(_bits(ctx.mat_to_numpy(given, padded=True)), _bits(before))
        ctx.destroy(given)
    # m > ld
    wide = glf.Mat.from_buffer_copy(dA)
    wide.cols = ld + 1
    given = ctx.dense_from_numpy(fill[:, :m], ld=ld, row_order=glf.ROWS_SAMPLE_FIRST)
    with pytest.raises(glf.GlfError) as e:
        ctx.Nystroem_ex(L_B, wide, dP, phi=given)
    assert e.value.status == glf.ERR_INVALID and "shape mismatch" in str(e.value), str(e.value)
    assert (ctx.mat_to_numpy(given, padded=True)[:, :m] == 3.5).all()
    # and the stage still works, into the same matrix
    phi, info = ctx.Nystroem_ex(L_B, dA, dP, phi=given)
    out = ctx.mat_to_numpy(phi, padded=True)
    np.testing.assert_array_equal(_bits(out[:r.p]), _bits(phi_A))
    assert np.isfinite(out).all() and not (out[:, :m] == 3.5).all(axis=1).any()
    ctx.destroy(dA, dP, given)
