"""One sweep Y = L_A X of the eigen-solve's operator in every form, through glf_operator_* (the function and the arguments the block PCG
uses), against a float64 product with a componentwise bound derived from each form's arithmetic. Needs an MI355X: -m gpu.

Reference and bound: tests/operator_ref.py (its docstring holds K, s, c and the dropped parts a_ij per form, with the code each comes
from). Grey guides: K_A in float64 from the oracle; the other formats: tests/u16_ref.py (format-neutral: it serves the float guides
too) and tests/rgb_ref.py; D and alpha are the GPU's own (the degree stage has its tests). Stored forms: the stored matrix as
downloaded, f32 bits widened.

Shapes (grey u8, glf.synth_image, glf.Sampling; p, nr x nc as realised):
  tiny     53 x 37, 20      p = 24 (4 x 6): one partial wave, one K tile, nr and nc below 16
  edge128  60 x 58, 120     p = 132 (11 x 12): the second 128-row block holds 4 rows; p % 64 != 0; nc no multiple of 16
  mid      192 x 64, 300    p = 320 (10 x 32): several row blocks
  slabs    450 x 300, 1350  p = 1350 (30 x 45): 22 K tiles, on an MI355X 8 K slabs, which do not divide 22; nc no multiple of 16
X (operator_ref.make_block): m = ld - 5 real columns of magnitudes 2^-30 .. 2^+30, one all-zero column, one unit vector, one column
that is zero on every even row, zero rows from p on. What the bound can see: |L| is dominated by its diagonal (D sums a sample's
kernel over all pixels: alpha D ~ 1 against alpha K_A entries ~ 1e-2 .. 1e-4), so on a dense random column an error of 2^-11 in the
K_A X contraction of a factored form can hide under gamma alpha D |X_ij|. The elements that carry the sensitivity to the contraction
are those with X_ij = 0: the unit vector's column (entries of K_A one at a time; its single operand is a power of two, so it has no
lo half) and the even rows of the half-zero column, where the bound is gamma alpha (K_A |X|)_ij + a_ij alone and the operands have
hi and lo halves. Under the f32 contraction the factored forms do not exist: their tests assert the refusal.

Set GLF_OPERATOR_ERROR_JSON to a path to have the largest observed |Y - Yref| / bound per form and ld written there (a record: the
asserted bound is the derived one)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import oracle as orc  # noqa: E402
import operator_ref as oref  # noqa: E402
import pix_cases  # noqa: E402

SHAPES = {"tiny": (53, 37, 20, 3), "edge128": (60, 58, 120, 4), "mid": (192, 64, 300, 5), "slabs": (450, 300, 1350, 6)}   # w, h, samples, seed
H_LOC, H_VAL = 40.0, 30.0
# form -> (tuning, form of the bound, glf_operator_info.path)
FORMS = {
    "dense": (dict(MV_PATH="dense"), None, 0),
    "grid": (dict(MV_PATH="grid"), "grid", 1),
    "grid_rt": (dict(MV_PATH="grid", ROWPASS_OP="rt"), "grid", 1),
    "rank": (dict(MV_PATH="rank", SWEEP_COLPASS="segments"), "rank", 3),
    "rank_samples": (dict(MV_PATH="rank", SWEEP_COLPASS="samples"), "rank", 3),
    "band": (dict(MV_PATH="band"), "band", 4),
}
FACTORED = [f for f in FORMS if f != "dense"]
DENSE_LD, FACTORED_LD = (32, 64, 128, 256), (32, 64, 128, 192, 256)
_RECORD = {}


@pytest.fixture(scope="module", params=["f16s", "f32"])
def ctx(request):
    """Both contraction modes, as in test_gpu_parity.py. The factored forms exist under the split-f16 mode only: under f32 their
    creation must be refused."""
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = glf.Context(0)
    c.set_contraction(glf.CONTRACT_F16_SPLIT if request.param == "f16s" else glf.CONTRACT_F32_MFMA)
    c.mode = request.param
    c.graphs = {}
    yield c
    for d_img, K_B, L_B, alpha, D in c.graphs.values():
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
    path = os.environ.get("GLF_OPERATOR_ERROR_JSON")
    if path and _RECORD:       # the layout of profiles/operator_error.json: one row per (form of the run / form of the bound, ld)
        agg = {}
        for (form, ld, label), (ratio, g) in sorted(_RECORD.items()):
            a = agg.setdefault((form, ld), dict(form=form, ld=ld, gamma_min=g, gamma_max=g, worst_error_over_bound=-1.0, worst_case=None))
            a["gamma_min"], a["gamma_max"] = min(a["gamma_min"], g), max(a["gamma_max"], g)
            if ratio > a["worst_error_over_bound"]:
                a["worst_error_over_bound"], a["worst_case"] = ratio, label
        what = ("largest observed |Y - Yref| / (gamma (|L| |X|) + a) per form (form of the run / form of the bound) and ld over the shapes and "
                "tests of tests/test_gpu_operator.py on an MI355X (GLF_OPERATOR_ERROR_JSON=<this file> python -m pytest "
                "tests/test_gpu_operator.py -m gpu); gamma: the derived value asserted (its range over the shapes). A record only.")
        with open(path, "w") as f:
            json.dump(dict(what=what, rows=[agg[k] for k in sorted(agg)]), f, indent=1)


class _Ref:
    pass


_REFS = {}


def _ref(shape):
    """The CPU side of a grey shape, computed once: image, samples, K_A (oracle, float64), the spatial factor K_sp alone."""
    if shape not in _REFS:
        w, h, ns, seed = SHAPES[shape]
        r = _Ref()
        r.w, r.h = w, h
        r.img = glf.synth_image(w, h, seed=seed)
        r.idx = glf.Sampling(w, h, ns)
        r.p = int(r.idx.size)
        r.nr, r.nc = oref.grid_shape(r.idx, w)
        r.KA, _ = orc.affinity(r.img, r.idx, want_KB=False)
        rr, cc = (r.idx // w).astype(np.float64), (r.idx % w).astype(np.float64)
        r.Ksp = np.exp(-((rr[:, None] - rr[None, :]) ** 2 + (cc[:, None] - cc[None, :]) ** 2) / H_LOC ** 2)
        _REFS[shape] = r
    return _REFS[shape]


def _graph(ctx, key, d_img, idx, kernel=glf.KERNEL_BILATERAL, h_loc=H_LOC, h_val=H_VAL):
    """(d_img, K_B, L_B, alpha, D) of a guide on this context, built once."""
    if key not in ctx.graphs:
        _, K_B = ctx.ComputeAffinityMatrices(d_img, idx, want_KA=False, kernel=kernel, h_loc=h_loc, h_val=h_val)
        L_A, L_B, alpha = ctx.ComputeLaplacianMatrix(None, K_B)
        ctx.destroy(L_A)
        ctx.graphs[key] = (d_img, K_B, L_B, alpha, ctx.degree_of(K_B))
    return ctx.graphs[key]


def _grey(ctx, shape, h_loc=H_LOC):
    r = _ref(shape)
    return _graph(ctx, (shape, h_loc), ctx.to_device(r.img), r.idx, h_loc=h_loc)


def _operator(ctx, form, L_B, **kw):
    ctx.reset_tuning()
    ctx.set_tuning(**FORMS[form][0])
    return ctx.operator(L_B, **kw)


def _refused_under_f32(ctx, form, L_B, **kw):
    """Under the f32 contraction a factored form does not exist (grid_op_create's rule): its creation is refused, and that is all
    there is to assert for it. True when that was the case."""
    if ctx.mode != "f32" or form == "dense":
        return False
    with pytest.raises(glf.GlfError) as e:
        _operator(ctx, form, L_B, **kw)
    assert e.value.status == glf.ERR_UNSUPPORTED and "MV_PATH" in str(e.value)
    return True


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _expect(ctx, form, op, X, p, alpha, D, KA, Ksp, nr, nc, pix=False):
    """(Yref [row1 - row0, ld], bound, gamma, form of the bound) for the rows of the operator's last apply."""
    row0, row1 = op.info["row0"], op.info["row1"]
    X64 = X[:p].astype(np.float64)
    aX = np.abs(X64)
    if form == "dense":
        S = op.stored().astype(np.float64)
        L = S[row0:row1] if ctx.mode == "f32" else S.T       # the f32 kernel reads row `row`, the split-f16 one column `row` (symmetric L_A)
        bform = ctx.mode
        g = oref.gamma(bform, p, ksplit=max(op.info["ksplit"], 1))
        absL = np.abs(L)
        return L @ X64, oref.bound(bform, g, absL @ aX, X64, p, absL_rowsum=absL.sum(axis=1)), g, bform
    bform = "pix_band" if pix else FORMS[form][1]
    g = oref.gamma(bform, p, nr=nr, nc=nc)
    Kabs = Ksp if bform == "rank" else KA
    Yref = alpha * (D[:, None] * X64 - KA @ X64)
    absLX = alpha * (D[:, None] * aX + Kabs @ aX)
    B = oref.bound(bform, g, absLX, X64, p, alpha=alpha, Ksp_X=(Ksp @ aX) if bform == "rank" else None)
    return Yref[row0:row1], B[row0:row1], g, bform


def _assert_within(ctx, form, op, X, Y, m, ref, alpha, D, label, pix=False, fill=None):
    """The bound on every element of the operator's rows; padding columns exactly zero; rows outside keep `fill`'s bits."""
    p = ref.p
    row0, row1 = op.info["row0"], op.info["row1"]
    Yref, B, g, bform = _expect(ctx, form, op, X, p, alpha, D, ref.KA, ref.Ksp, ref.nr, ref.nc, pix)
    err = np.abs(Y[row0:row1].astype(np.float64) - Yref)
    pos = B > 0
    ratio = float((err[pos] / B[pos]).max()) if pos.any() else 0.0
    print("%s %s ld %d rows [%d, %d): gamma 2^%.2f, worst |Y - Yref| / bound %.3f" % (label, form, X.shape[1], row0, row1, np.log2(g), ratio))
    key = ("%s/%s" % (form, bform), X.shape[1], label)
    if ratio > _RECORD.get(key, (-1.0, g))[0]:
        _RECORD[key] = (ratio, g)
    assert np.isfinite(Y[row0:row1]).all()
    bad = np.argwhere(err > B)
    assert bad.size == 0, "%d elements beyond the bound, first (row %d, column %d): error %.3e, bound %.3e; worst ratio %.2f" % (
        len(bad), bad[0][0] + row0, bad[0][1], err[tuple(bad[0])], B[tuple(bad[0])], ratio)
    assert not Y[row0:row1, m:].any(), "padding columns of Y are not exactly zero"
    if fill is not None:
        outside = np.r_[0:row0, row1:Y.shape[0]]
        np.testing.assert_array_equal(_bits(Y[outside]), _bits(fill[outside]))
    return ratio


AGAINST = [("dense", ld) for ld in DENSE_LD] + [(f, ld) for f in FACTORED for ld in FACTORED_LD]


@pytest.mark.parametrize("form,ld", AGAINST, ids=["%s-%d" % fl for fl in AGAINST])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_fp64(ctx, shape, form, ld):
    r = _ref(shape)
    d_img, K_B, L_B, alpha, D = _grey(ctx, shape)
    if _refused_under_f32(ctx, form, L_B):
        return
    m = ld - 5
    X = oref.make_block(r.p, ld, m, seed=100 + ld)
    with _operator(ctx, form, L_B, ld_hint=ld) as op:
        Y = op.apply_numpy(X)
        assert op.info["path"] == FORMS[form][2] and (op.info["row0"], op.info["row1"]) == (0, r.p)
        _assert_within(ctx, form, op, X, Y, m, r, alpha, D, shape)
    assert not Y[r.p:].any()


def test_k_slabs_one_and_several(ctx):
    """The stored split-f16 form runs with one K slab on one shape and with several, which do not divide the tile count, on another
    (so that the coverage above does not silently depend on the CU count); the f32 form reports none."""
    seen = {}
    for shape in ("tiny", "slabs"):
        r = _ref(shape)
        with _operator(ctx, "dense", _grey(ctx, shape)[2], ld_hint=32) as op:
            op.apply_numpy(oref.make_block(r.p, 32, 27, seed=1))
            seen[shape] = op.info["ksplit"]
    if ctx.mode == "f32":
        assert seen == {"tiny": 0, "slabs": 0}
        return
    tiles = oref.round_up(_ref("slabs").p, 64) // 64
    assert seen["tiny"] == 1 and seen["slabs"] > 1 and tiles == 22 and tiles % seen["slabs"] != 0, seen


def _pix_case(fmt, shape):
    w, h, ns, seed = SHAPES[shape]
    return pix_cases.pix_case(fmt, w, h, seed)


@pytest.mark.parametrize("ld", [32, 64])
@pytest.mark.parametrize("shape", ["tiny", "mid"])
@pytest.mark.parametrize("fmt", ["rgb8", "u16", "f32", "rgbf32"])
def test_pixel_formats_band(ctx, fmt, shape, ld):
    """The band form of the colour, 16-bit and float kernels (PIX_BAND) against the format's numpy kernel; ld 128 is refused."""
    g = _ref(shape)
    img, kernel, h_val, ref = _pix_case(fmt, shape)
    d_img = torch.from_numpy(np.ascontiguousarray(img)).to(ctx.device)
    _, K_B, L_B, alpha, D = _graph(ctx, (fmt, shape), d_img, g.idx, kernel=kernel, h_val=h_val)
    ctx.reset_tuning()
    ctx.set_tuning(MV_PATH="band", PIX_BAND="1")
    if ctx.mode == "f32":
        with pytest.raises(glf.GlfError) as e:
            ctx.operator(L_B, ld_hint=ld)
        assert e.value.status == glf.ERR_UNSUPPORTED
        return
    r = _Ref()
    r.p, r.nr, r.nc, r.Ksp = g.p, g.nr, g.nc, g.Ksp
    r.KA = ref.kernel(img, g.idx, g.idx, H_LOC, h_val)
    m = ld - 5
    X = oref.make_block(r.p, ld, m, seed=200 + ld)
    with ctx.operator(L_B, ld_hint=ld) as op:
        Y = op.apply_numpy(X)
        assert op.info["path"] == 4
        _assert_within(ctx, "band", op, X, Y, m, r, alpha, D, "%s/%s" % (fmt, shape), pix=True)
        fill = np.full((oref.round_up(r.p, 64), 128), 12345.0, dtype=np.float32)
        with pytest.raises(glf.GlfError) as e:
            op.apply_numpy(oref.make_block(r.p, 128, 100, seed=3), fill=fill)
        assert e.value.status == glf.ERR_INVALID and "ld" in str(e.value)
        np.testing.assert_array_equal(_bits(op.last_Y), _bits(fill))
    with pytest.raises(glf.GlfError) as e:
        ctx.operator(L_B, ld_hint=128)
    assert e.value.status == glf.ERR_UNSUPPORTED


def _boxes(idx, w, p):
    """Bounding boxes (rmin, rmax, cmin, cmax) of the 64-sample chunks, as chunk_boxes builds them."""
    rr, cc = idx // w, idx % w
    return [(rr[c:c + 64].min(), rr[c:c + 64].max(), cc[c:c + 64].min(), cc[c:c + 64].max()) for c in range(0, p, 64)]


@pytest.mark.parametrize("form", ["dense", "grid", "rank"])
def test_skipping_is_bit_identical(ctx, form):
    """skip_exact_zeros on and off give the same bits -- the forms for which the whole-path test promises it -- on a graph whose
    radius (pipeline.hip: floor(sqrt((35.5 + log2 alpha) / s_loc)) + 1) is under a quarter of the image side, so that tiles are skipped."""
    shape, h_loc = "slabs", 5.0
    r = _ref(shape)
    d_img, K_B, L_B, alpha, D = _grey(ctx, shape, h_loc=h_loc)
    if _refused_under_f32(ctx, form, L_B, skip_exact_zeros=1):
        return
    s_loc = float(np.float32(np.log2(np.e) / h_loc ** 2))
    radius = int(np.floor(np.sqrt((35.5 + np.log2(alpha)) / s_loc))) + 1
    assert 0 < radius < min(r.w, r.h) / 4
    box = _boxes(r.idx.astype(np.int64), r.w, r.p)
    far = 0
    for b0 in range(0, len(box), 2):                          # a 128-row block: two chunks
        rb = box[b0] if b0 + 1 >= len(box) else (min(box[b0][0], box[b0 + 1][0]), max(box[b0][1], box[b0 + 1][1]),
                                                 min(box[b0][2], box[b0 + 1][2]), max(box[b0][3], box[b0 + 1][3]))
        far += sum(not (b[1] >= rb[0] - radius and b[0] <= rb[1] + radius and b[3] >= rb[2] - radius and b[2] <= rb[3] + radius) for b in box)
    assert far >= 1, "no (128-row block, 64-column tile) pair lies beyond the radius %d" % radius
    for ld in (64, 256):
        X = oref.make_block(r.p, ld, ld - 5, seed=300 + ld)
        res = {}
        for skip in (0, 1):
            with _operator(ctx, form, L_B, skip_exact_zeros=skip, ld_hint=ld) as op:
                res[skip] = op.apply_numpy(X)
                assert op.info["path"] == FORMS[form][2]
                if ctx.mode == "f16s":
                    assert op.info["skipping"] == skip, (form, skip, op.info)
        np.testing.assert_array_equal(_bits(res[0]), _bits(res[1]))
        assert np.abs(res[0][:r.p, :ld - 5]).max() > 0


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", ["edge128", "mid"])
def test_power_of_two_column_scaling_is_exact(ctx, shape, form):
    """Y(X diag(2^e)) = Y(X) diag(2^e) bit for bit, e = +-20: every form takes its operand scales per column as powers of two (from the
    column maximum's exponent), and every later step is a product or a sum of products, which a power of two passes through
    exactly as long as nothing leaves the normal f32 range (magnitudes here: 2^-50 .. 2^+60)."""
    r = _ref(shape)
    L_B = _grey(ctx, shape)[2]
    if _refused_under_f32(ctx, form, L_B):
        return
    ld, m = 64, 59
    X = oref.make_block(r.p, ld, m, seed=400)
    e = np.where(np.arange(ld) % 2 == 0, 20, -20)
    s = np.ldexp(np.float32(1), e).astype(np.float32)
    with _operator(ctx, form, L_B, ld_hint=ld) as op:
        Y = op.apply_numpy(X)
        Ys = op.apply_numpy(X * s[None, :])
    assert np.abs(Y[:r.p, :m]).max() > 0
    np.testing.assert_array_equal(_bits(Ys), _bits(Y * s[None, :]))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", ["edge128", "mid"])
def test_a_column_does_not_depend_on_its_neighbours(ctx, shape, form):
    """Every other column of X replaced (other values, other magnitudes, some zeroed): the untouched columns of Y keep their bits."""
    r = _ref(shape)
    L_B = _grey(ctx, shape)[2]
    if _refused_under_f32(ctx, form, L_B):
        return
    for ld in (32, 128):
        X = oref.make_block(r.p, ld, ld - 5, seed=500 + ld)
        X2 = X.copy()
        other = oref.make_block(r.p, ld, ld - 5, seed=600 + ld)
        X2[:, 1::2] = other[:, 1::2][:, ::-1]
        X2[:, 5] = 0.0
        with _operator(ctx, form, L_B, ld_hint=ld) as op:
            Y, Y2 = op.apply_numpy(X), op.apply_numpy(X2)
        assert not np.array_equal(_bits(Y[:, 1::2]), _bits(Y2[:, 1::2]))
        np.testing.assert_array_equal(_bits(Y[:, 0::2]), _bits(Y2[:, 0::2]))


@pytest.mark.parametrize("form", FACTORED)
@pytest.mark.parametrize("shape", ["edge128", "slabs"])
def test_widths_in_sequence_on_one_operator(ctx, shape, form):
    """One handle applied at ld 256, 64, 32, 192, 256 and then 32, 256 (a narrower block reuses the wider block's buffers), and a
    second handle applied at 32, 64, 192, 256, 32 (work_ld and rank_ld grow: Bp, T and rank_S are allocated again for another
    n-tile count, rank_nt is reset): every result within the bound, equal widths equal bits, on either handle and between them."""
    r = _ref(shape)
    d_img, K_B, L_B, alpha, D = _grey(ctx, shape)
    if _refused_under_f32(ctx, form, L_B):
        return
    X = {ld: oref.make_block(r.p, ld, ld - 5, seed=700 + ld) for ld in (32, 64, 192, 256)}
    first = {}
    for order in ((256, 64, 32, 192, 256, 32, 256), (32, 64, 192, 256, 32)):
        with _operator(ctx, form, L_B, ld_hint=256) as op:
            for ld in order:
                Y = op.apply_numpy(X[ld])
                _assert_within(ctx, form, op, X[ld], Y, ld - 5, r, alpha, D, "%s/sequence" % shape)
                if ld in first:
                    np.testing.assert_array_equal(_bits(Y), _bits(first[ld]), err_msg="ld %d in the order %s" % (ld, order))
                first.setdefault(ld, Y)


def _ranges(ctx, form, r):
    if form == "dense":       # ending inside a 128-row block
        return [(0, 70), (64, r.p - 3), (128, r.p)] if r.p > 140 else [(0, 70), (64, r.p - 1)]
    return [(0, r.nc), (r.nc, 3 * r.nc), ((r.nr - 1) * r.nc, r.p)]   # one grid row; two; the last one, row1 = p


@pytest.mark.parametrize("form", ["dense", "grid", "rank", "band"])
@pytest.mark.parametrize("shape", ["edge128", "mid"])
def test_row_ranges(ctx, shape, form):
    """The rows one rank of the sharded solve owns: inside the range within the bound, outside a sentinel's bits. Stored split-f16: the
    reference is the column block the operator built."""
    r = _ref(shape)
    d_img, K_B, L_B, alpha, D = _grey(ctx, shape)
    if ctx.mode == "f32":
        with pytest.raises(glf.GlfError) as e:
            _operator(ctx, form, L_B, rows=_ranges(ctx, form, r)[0])
        assert e.value.status == glf.ERR_UNSUPPORTED
        return
    ld, m = 64, 59
    X = oref.make_block(r.p, ld, m, seed=800)
    fill = np.full((oref.round_up(r.p, 64), ld), -7.25, dtype=np.float32)
    for rows in _ranges(ctx, form, r):
        with _operator(ctx, form, L_B, rows=rows, ld_hint=ld) as op:
            Y = op.apply_numpy(X, fill=fill)
            assert (op.info["row0"], op.info["row1"]) == rows and op.info["path"] == FORMS[form][2]
            if form == "dense":
                assert op.stored().shape == (r.p, rows[1] - rows[0])
            _assert_within(ctx, form, op, X, Y, m, r, alpha, D, "%s/rows" % shape, fill=fill)


def test_refusals_leave_Y_untouched(ctx):
    """Every refusal names its reason and leaves Y bit-identical."""
    r = _ref("edge128")
    d_img, K_B, L_B, alpha, D = _grey(ctx, "edge128")
    rows64 = oref.round_up(r.p, 64)

    def refused(status, word, call):
        with pytest.raises(glf.GlfError) as e:
            call()
        assert e.value.status == status and word in str(e.value), str(e.value)

    # creation: not a KERNEL_B descriptor / no degree; rows; NLM with a factored path; a forced path that does not apply
    dense = ctx.dense_from_numpy(np.zeros((64, 32), dtype=np.float32))
    refused(glf.ERR_INVALID, "KERNEL_B", lambda: ctx.operator(dense))
    no_degree = glf.Mat.from_buffer_copy(L_B)
    no_degree.degree = None
    refused(glf.ERR_INVALID, "degree", lambda: ctx.operator(no_degree))
    ctx.destroy(dense)
    refused(glf.ERR_INVALID, "rows", lambda: ctx.operator(L_B, rows=(10, 5)))
    refused(glf.ERR_INVALID, "rows", lambda: ctx.operator(L_B, rows=(0, r.p + 1)))
    refused(glf.ERR_INVALID, "ld_hint", lambda: ctx.operator(L_B, ld_hint=48))
    nlm = glf.Mat.from_buffer_copy(L_B)
    nlm.kernel = glf.KERNEL_NLM
    ctx.set_tuning(MV_PATH="grid")
    refused(glf.ERR_UNSUPPORTED, "non-local-means", lambda: ctx.operator(nlm))
    ctx.reset_tuning()
    ridx = glf.RandomSampling(r.w, r.h, 100, seed=2)        # not a tensor grid
    _, K_Br, L_Br, _, _ = _graph(ctx, ("random", "edge128"), d_img, ridx)
    for path in ("grid", "rank", "band"):
        ctx.set_tuning(MV_PATH=path)
        refused(glf.ERR_UNSUPPORTED, "MV_PATH", lambda: ctx.operator(L_Br))
    ctx.reset_tuning()
    if ctx.mode == "f32":
        refused(glf.ERR_UNSUPPORTED, "split-f16", lambda: _operator(ctx, "dense", L_B, rows=(0, 64)))
    else:
        refused(glf.ERR_INVALID, "multiple of 64", lambda: _operator(ctx, "dense", L_B, rows=(10, 100)))
        refused(glf.ERR_INVALID, "whole grid rows", lambda: _operator(ctx, "grid", L_B, rows=(0, r.nc + 1)))
        refused(glf.ERR_INVALID, "whole grid rows", lambda: _operator(ctx, "band", L_B, rows=(1, r.nc)))

    # apply: fewer than p rows; an ld the form does not take; X and Y of different ld; a tuning change since creation
    def apply_refused(op, X, word, status=glf.ERR_INVALID, fill_ld=None):
        fill = np.full((rows64, fill_ld or X.shape[1]), 3.5, dtype=np.float32)
        refused(status, word, lambda: op.apply_numpy(X, fill=fill))
        np.testing.assert_array_equal(_bits(op.last_Y), _bits(fill))

    forms = ["dense"] if ctx.mode == "f32" else ["dense", "grid", "rank", "band"]
    for form in forms:
        with _operator(ctx, form, L_B) as op:
            apply_refused(op, oref.make_block(r.p, 32, 27, seed=1)[:r.p - 1], "fewer than p")
            for ld in ((96, 192) if form == "dense" else (96, 160)):
                apply_refused(op, np.ones((r.p, ld), dtype=np.float32), "ld")
            ctx.set_tuning(MV_PATH="dense" if form != "dense" else "grid")
            apply_refused(op, oref.make_block(r.p, 32, 27, seed=1), "changed since")
            ctx.set_tuning(**FORMS[form][0])
            X = oref.make_block(r.p, 32, 27, seed=1)
            dX, dY = ctx.dense_from_numpy(X, ld=32), ctx.dense_from_numpy(np.full((rows64, 64), 3.5, dtype=np.float32), ld=64)
            refused(glf.ERR_INVALID, "ld", lambda: op.apply(dX, dY))
            np.testing.assert_array_equal(ctx.mat_to_numpy(dY), np.full((rows64, 64), 3.5, dtype=np.float32))
            refused(glf.ERR_INVALID, "dense", lambda: op.apply(dX, L_B))
            ctx.destroy(dX, dY)
            Y = op.apply_numpy(X)                                  # and the handle still works
            assert np.isfinite(Y).all() and np.abs(Y[:r.p]).max() > 0
    if ctx.mode == "f16s":
        with _operator(ctx, "grid", L_B) as op:
            refused(glf.ERR_UNSUPPORTED, "stores no matrix", op.stored)


def test_solver_reaches_these_widths(ctx):
    """A whole grey run at ld 256 on the grid form: the block PCG issues narrow sweeps (a packed block of the still-iterating columns:
    ld 32 or a multiple of 64 below 256, 192 among them), the widths applied above. No accuracy claim."""
    ctx.set_tuning(NYS_PATH="grid", DEG_PATH="grid", MV_PATH="grid")
    img = glf.synth_image(256, 256, seed=7)
    opt = glf.default_options(num_samples=655, num_eigvals=200, epsilon=0.1)
    out, zf, info = ctx.image_processing(ctx.to_device(img), opt, capture=True)
    assert info["capture"]["ld"] == 256
    if ctx.mode == "f32":      # (no grid form under the f32 contraction: L_A is stored, and this run issues no packed sweep)
        assert info["matvec_path"] == 0
        return
    assert info["matvec_path"] == 1
    assert info["narrow_sweeps"] > 0 and info["matvecs"] > info["narrow_sweeps"]
