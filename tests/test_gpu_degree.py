"""The degree stage D_A = rowsum [K_A K_B] in every form, through glf_Degree_ex (the stage call, with the whole path's window, row
range, value-weighted sums and weighted sums, and a report of what ran), against a float64 row sum with a per-sample bound derived from
each form's arithmetic. Needs an MI355X: -m gpu.

Reference and bound: tests/degree_ref.py (its docstring holds K, s, c and the floors per form with the code each comes from; its SHAPES
and TABLE say which k_dgrid_zmfma shape, how many chunks and m-groups each grid shape must report, derived on the CPU by
tests/test_degree_bound.py). Every call writes into sentinel-filled host buffers, every sample is compared, and glf_degree_info is
compared with the plan: a test that ran another kernel than it names fails.

Guides of the grid form: glf.synth_image; a flat image (the longest histogram chain, Wt at the full table mass); the sparse-support
guide of degree_ref.sparse_guide (a sample sees a handful of pixels, each worth far more than the bound).

What these tests cannot see: an error below a form's floor a (degree_ref), the full-matrix mode (k_degree_ky) and multi-rank runs.

Set GLF_DEGREE_ERROR_JSON to a path to have gamma and the largest observed |error| / bound per form and case written there (a record:
the asserted bound is the derived one)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import oracle as orc  # noqa: E402
import degree_ref as dref  # noqa: E402
import pix_cases  # noqa: E402

SENTINEL = -12345.5
_RECORD, _REFS, _GUIDES = {}, {}, {}


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = glf.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _default_kernel_selection(request):
    yield
    if "ctx" in request.fixturenames:
        request.getfixturevalue("ctx").reset_tuning()


@pytest.fixture(scope="module", autouse=True)
def _error_record():
    yield
    path = os.environ.get("GLF_DEGREE_ERROR_JSON")
    if path and _RECORD:
        agg = {}
        for (form, case, what), (ratio, g) in sorted(_RECORD.items()):
            a = agg.setdefault((form, case), dict(form=form, case=case, gamma=g, worst_error_over_bound=-1.0, worst_of=None))
            if ratio > a["worst_error_over_bound"]:
                a["worst_error_over_bound"], a["worst_of"] = ratio, what
        what = ("gamma (derived, asserted) and the largest observed |error| / (gamma reference + a) per form and case of "
                "tests/test_gpu_degree.py on an MI355X (GLF_DEGREE_ERROR_JSON=<this file> python -m pytest tests/test_gpu_degree.py -m gpu). "
                "A record only.")
        with open(path, "w") as f:
            json.dump(dict(what=what, rows=[agg[k] for k in sorted(agg)]), f, indent=1)


def _dev(ctx, img):
    if img.dtype == np.uint8 and img.ndim == 2:
        return ctx.to_device(img)
    return torch.from_numpy(np.ascontiguousarray(img)).to(ctx.device)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _call(ctx, img, idx, kernel=glf.KERNEL_BILATERAL, h_loc=40.0, h_val=dref.H_VAL, skip=0, rows=None, plane=None, ysum=False, **tuning):
    """One stage call into sentinel-filled buffers: (D, Uy or None, info)."""
    ctx.reset_tuning()
    ctx.set_tuning(**tuning)
    d_img = _dev(ctx, img)
    d_plane = None if plane is None else torch.from_numpy(np.ascontiguousarray(plane, dtype=np.float32)).to(ctx.device)
    deg = np.full(len(idx), SENTINEL)
    uy = np.full(len(idx), SENTINEL) if ysum else None
    D, Uy, info = ctx.Degree_ex(d_img, idx, kernel=kernel, h_loc=h_loc, h_val=h_val, skip_exact_zeros=skip, rows=rows, plane=d_plane,
                                out=(deg, uy))
    assert not (D == SENTINEL).any() and (Uy is None or not (Uy == SENTINEL).any())
    h, w = img.shape[:2]
    r0, r1 = (0, h) if rows is None else rows
    assert (info["row0"], info["row1"]) == (r0, r1)
    assert 0 <= info["entries_evaluated"] <= float(len(idx)) * (r1 - r0) * w
    return D, Uy, info


def _refused(ctx, status, img, idx, **kw):
    """A refusal: the status, a message, and sentinel-filled outputs and info untouched."""
    d_img = _dev(ctx, img)
    plane = kw.pop("plane", None)
    d_plane = None if plane is None else torch.from_numpy(np.ascontiguousarray(plane, dtype=np.float32)).to(ctx.device)
    ysum = kw.pop("ysum", False)
    deg, uy = np.full(len(idx), SENTINEL), np.full(len(idx), SENTINEL) if ysum else None
    with pytest.raises(glf.GlfError) as e:
        ctx.Degree_ex(d_img, idx, plane=d_plane, out=(deg, uy), **kw)
    assert e.value.status == status, str(e.value)
    assert len(str(e.value).split("Degree_ex ", 1)[-1].strip()) > 8, str(e.value)      # the reason, from glf_ctx_last_error
    assert (deg == SENTINEL).all() and (uy is None or (uy == SENTINEL).all())


def _guide(name, w, h):
    key = (name, w, h)
    if key not in _GUIDES:
        _GUIDES[key] = {"synth": lambda: (glf.synth_image(w, h, seed=3), dref.H_VAL),
                        "flat": lambda: (np.full((h, w), 128, dtype=np.uint8), dref.H_VAL),
                        "sparse": lambda: (dref.sparse_guide(w, h, 5), dref.SPARSE_H_VAL)}[name]()
    return _GUIDES[key]


def _ref(key, img, idx, h_loc, h_val, rows=None, kern=dref.u16_ref.kernel, plane=None):
    """The float64 side, computed once per key and left unchanged."""
    if key not in _REFS:
        _REFS[key] = dref.reference(img, idx, h_loc, h_val, rows=rows, kern=kern, plane=plane)
    return _REFS[key]


def _within(form, case, what, x, x_ref, B, g):
    ratio, ok = dref.check(x, x_ref, B)
    _RECORD[(form, case, what)] = (ratio, g)
    print("%s %s %s: gamma 2^%.2f, worst error / bound %.4f" % (form, case, what, np.log2(g), ratio))
    assert ok, (form, case, what, ratio)


def _plan_matches(info, plan, skipping):
    assert info["path"] == glf.DEG_GRID
    assert (info["shape"], info["chunks"], info["mgroups"], info["skipping"]) == (plan["shape"], plan["chunks"], plan["mgroups"], skipping), (info, plan)


# ---- the grid form ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("guide", ["synth", "flat", "sparse"])
@pytest.mark.parametrize("name", sorted(dref.SHAPES))
def test_grid_form_against_fp64(ctx, name, guide):
    """D and Uy of every grid shape and guide; the dense and the skipping sweep give the same bits; info names the planned shape."""
    w, h, rows, cols, h_loc, idx = dref.shape(name)
    img, h_val = _guide(guide, w, h)
    plan = dref.grid_plan(w, h, rows, cols, h_loc)
    assert (idx.size, plan["nr"], plan["nc"], plan["radius"], plan["shape"], plan["chunks"], plan["mgroups"]) == dref.TABLE[name]
    ref = _ref((name, guide), img, idx, h_loc, h_val)
    g, BD, BY, _ = dref.bounds("grid", ref, h_loc=h_loc, h_val=h_val, width=w, radius=plan["radius"])
    assert g < 2.0 ** -11 / 6
    D, Uy, info = _call(ctx, img, idx, h_loc=h_loc, h_val=h_val, ysum=True, DEG_PATH="grid")
    _plan_matches(info, plan, 0)
    _within("grid", "%s/%s" % (name, guide), "D", D, ref.D, BD, g)
    _within("grid", "%s/%s" % (name, guide), "Uy", Uy, ref.Uy, BY, g)
    assert info["entries_evaluated"] == float(idx.size) * h * w
    D1, Uy1, info1 = _call(ctx, img, idx, h_loc=h_loc, h_val=h_val, skip=1, ysum=True, DEG_PATH="grid")
    can_skip = plan["radius"] < max(w, h)
    _plan_matches(info1, plan, 1 if can_skip else 0)
    assert np.array_equal(_bits(D1), _bits(D)) and np.array_equal(_bits(Uy1), _bits(Uy))
    assert info1["entries_evaluated"] >= ref.pairs
    if can_skip and name.startswith("window"):
        assert info1["entries_evaluated"] < info["entries_evaluated"]


def test_forced_groups_of_five_give_the_one_group_bits(ctx):
    w, h, rows, cols, h_loc, idx = dref.shape("ten")
    img, h_val = _guide("synth", w, h)
    D, Uy, info = _call(ctx, img, idx, h_loc=h_loc, ysum=True, DEG_PATH="grid")
    D5, Uy5, info5 = _call(ctx, img, idx, h_loc=h_loc, ysum=True, DEG_PATH="grid", ZMFMA_GROUPS="1")
    assert (info["shape"], info["mgroups"]) == (glf.DEG_TEN, 1)
    forced = dref.grid_plan(w, h, rows, cols, h_loc, zmfma_groups=True)
    _plan_matches(info5, forced, 0)
    assert (info5["shape"], info5["mgroups"]) == (glf.DEG_FIVES, 2)
    assert np.array_equal(_bits(D5), _bits(D)) and np.array_equal(_bits(Uy5), _bits(Uy))


SHARDS = [(300, 900), (0, 1), (1099, 1100), (0, 300), (900, 1100)]


@pytest.mark.parametrize("name", ["window_3", "window_refused"])
def test_grid_row_shards(ctx, name):
    """Row shards: [300, 900) (row0 no multiple of 16, grid rows above the shard and out of its reach), one-row shards at both ends, and
    three shards that partition the image: their sum is the all-rows result within the sum of their bounds."""
    w, h, rows, cols, h_loc, idx = dref.shape(name)
    img, h_val = _guide("synth", w, h)
    parts, bsum = np.zeros(idx.size), np.zeros(idx.size)
    for shard in SHARDS:
        plan = dref.grid_plan(w, h, rows, cols, h_loc, row0=shard[0], row1=shard[1])
        ref = _ref((name, "synth", shard), img, idx, h_loc, h_val, rows=shard)
        g, BD, BY, _ = dref.bounds("grid", ref, h_loc=h_loc, h_val=h_val, width=w, radius=plan["radius"])
        for skip in (0, 1):
            D, Uy, info = _call(ctx, img, idx, h_loc=h_loc, skip=skip, rows=shard, ysum=True, DEG_PATH="grid")
            _plan_matches(info, plan, skip)
            _within("grid", "%s/rows %d-%d/skip %d" % (name, shard[0], shard[1], skip), "D", D, ref.D, BD, g)
            _within("grid", "%s/rows %d-%d/skip %d" % (name, shard[0], shard[1], skip), "Uy", Uy, ref.Uy, BY, g)
            if skip:
                assert np.array_equal(_bits(D), _bits(D0)) and info["entries_evaluated"] >= ref.pairs
            D0 = D
        if shard in ((0, 300), (300, 900), (900, 1100)):
            parts += D0
            bsum += BD
    if name == "window_3":
        assert dref.grid_plan(w, h, rows, cols, h_loc, row0=300, row1=900)["mt0"][0] > 0      # m-tiles above the shard are never stored
    D_all, _, _ = _call(ctx, img, idx, h_loc=h_loc, DEG_PATH="grid")
    ref_all = _ref((name, "synth"), img, idx, h_loc, h_val)
    _, B_all, _, _ = dref.bounds("grid", ref_all, h_loc=h_loc, h_val=h_val, width=w, radius=51)
    assert (np.abs(parts - D_all) <= bsum + B_all).all()


def _planes(w, h):
    s = dref.signed_plane(w, h, 1)
    one = np.zeros((h, w), dtype=np.float32)
    one[h // 2] = s[h // 2]
    return {"signed": s, "one_row": one}


@pytest.mark.parametrize("name", ["fives", "window_3", "wide_5", "wide_40"])
def test_weighted_sums(ctx, name):
    """U_s of a signed plane with cancellation and of a plane that is zero outside one row, against gamma Uabs + a; the same planes
    times 2^+100 and 2^-100 return exactly 2^+-100 times the result (power-of-two operand scales)."""
    w, h, rows, cols, h_loc, idx = dref.shape(name)
    img, h_val = _guide("synth", w, h)
    plan = dref.grid_plan(w, h, rows, cols, h_loc)
    for pname, s in _planes(w, h).items():
        ref = _ref((name, "synth", pname), img, idx, h_loc, h_val, plane=s)
        g, _, _, BS = dref.bounds("grid", ref, h_loc=h_loc, h_val=h_val, width=w, radius=plan["radius"])
        if pname == "signed":
            assert (np.abs(ref.Us) < 0.2 * ref.Uabs).any()
        for skip in (0, 1):
            Us, _, info = _call(ctx, img, idx, h_loc=h_loc, skip=skip, plane=s, DEG_PATH="grid")
            _plan_matches(info, plan, skip if plan["radius"] < max(w, h) else 0)
            _within("grid weighted", "%s/%s/skip %d" % (name, pname, skip), "Us", Us, ref.Us, BS, dref.gamma("grid", width=w, radius=plan["radius"], weighted=True))
            if skip:
                assert np.array_equal(_bits(Us), _bits(Us0))
            Us0 = Us
        for e in (100, -100):
            scaled = np.ldexp(s, e).astype(np.float32)
            assert np.array_equal(np.ldexp(scaled.astype(np.float64), -e), s.astype(np.float64))     # (the plane itself scales exactly)
            Ue, _, _ = _call(ctx, img, idx, h_loc=h_loc, plane=scaled, DEG_PATH="grid")
            assert np.isfinite(Ue).all(), (name, pname, e)
            assert np.array_equal(_bits(Ue), _bits(np.ldexp(Us0, e))), (name, pname, e, float(np.abs(Ue - np.ldexp(Us0, e)).max()))
    if name == "window_3":      # a shard of the weighted form
        s, shard = _planes(w, h)["signed"], (300, 900)
        ref = _ref((name, "synth", "signed", shard), img, idx, h_loc, h_val, rows=shard, plane=s)
        g, _, _, BS = dref.bounds("grid", ref, h_loc=h_loc, h_val=h_val, width=w, radius=plan["radius"])
        Us, _, info = _call(ctx, img, idx, h_loc=h_loc, rows=shard, plane=s, DEG_PATH="grid")
        _within("grid weighted", "%s/signed/rows 300-900" % name, "Us", Us, ref.Us, BS, g)


# ---- the direct sweeps --------------------------------------------------------------------------------------------------------------------

def _random_idx(w, h, p, seed):
    return np.sort(np.random.default_rng(seed).choice(w * h, size=p, replace=False)).astype(np.uint32)


@pytest.mark.parametrize("h,shard", [(35, None), (43, None), (35, (5, 30)), (35, (16, 17))])
def test_direct_sweep_against_fp64(ctx, h, shard):
    """k_degree on 261 columns (wider than DEGL_SEGW, no multiple of 4) with p = 257 (the second block has one live lane): 35 rows (two
    chunks plus 3: the second half of the workgroup idles), 43 rows (a last chunk of 11), and shards."""
    w, p = 261, 257
    img, idx = glf.synth_image(w, h, seed=4), _random_idx(w, h, p, 9)
    ref = _ref(("direct", h, shard), img, idx, 40.0, dref.H_VAL, rows=shard)
    g, BD, _, _ = dref.bounds("direct", ref)
    D, _, info = _call(ctx, img, idx, rows=shard, DEG_PATH="direct")
    r0, r1 = shard or (0, h)
    assert (info["path"], info["skipping"], info["chunks"]) == (glf.DEG_DENSE, 0, -(-(r1 - r0) // 16))
    assert info["entries_evaluated"] == float(p) * (r1 - r0) * w
    _within("direct", "261x%d/rows %s" % (h, shard), "D", D, ref.D, BD, g)
    _refused(ctx, glf.ERR_UNSUPPORTED, img, idx, ysum=True)                     # no value-weighted sums in this form
    ctx.set_tuning(DEG_PATH="direct")
    _refused(ctx, glf.ERR_UNSUPPORTED, img, idx, plane=np.ones((h, w), dtype=np.float32))


def test_windowed_direct_sweep_gives_the_dense_bits(ctx):
    w, h, p, h_loc = 261, 70, 257, 2.0
    img, idx = glf.synth_image(w, h, seed=4), _random_idx(w, h, p, 9)
    ref = _ref(("direct", "win"), img, idx, h_loc, dref.H_VAL)
    g, BD, _, _ = dref.bounds("direct", ref)
    D, _, info = _call(ctx, img, idx, h_loc=h_loc, DEG_PATH="direct")
    Dw, _, infow = _call(ctx, img, idx, h_loc=h_loc, skip=1, DEG_PATH="direct")
    assert (info["path"], infow["path"], infow["skipping"]) == (glf.DEG_DENSE, glf.DEG_WINDOWED, 1)
    _within("direct", "261x70 windowed", "D", Dw, ref.D, BD, g)
    assert np.array_equal(_bits(Dw), _bits(D))
    assert ref.pairs <= infow["entries_evaluated"] < info["entries_evaluated"]


# ---- the pixel formats ----------------------------------------------------------------------------------------------------------------------

PIX_W, PIX_H = 70, 45


def _pix_guide(fmt):
    """(image, kernel, h_val, reference module): pix_cases' pattern, with the 16-bit guide over the full range and the float guides
    holding negative values and magnitudes of 1e6 and 1e-3 in one image (h_val to match the large ones)."""
    img, kernel, h_val, mod = pix_cases.pix_case(fmt, PIX_W, PIX_H, 6)
    if fmt == "u16":
        img = img.copy()
        img[0, 0], img[PIX_H - 1, PIX_W - 1] = 0, 65535
    if fmt in ("f32", "rgbf32"):
        pat = pix_cases.pattern(PIX_H, PIX_W, 6, 3 if fmt == "rgbf32" else 1)
        img = (2.0e6 * (pat - 0.5)).astype(np.float32)
        img[10:30, 40:60] = (1.0e-3 * (pat[10:30, 40:60] - 0.5)).astype(np.float32)
        h_val = 2.0e6 * 30.0 / 255.0
        assert img.min() < -1e5 and img.max() > 1e5
    return img, kernel, h_val, mod


def _pix_idx(kind):
    if kind == "random":
        return _random_idx(PIX_W, PIX_H, 257, 12)
    r, c = np.array([3, 14, 27, 41]), np.array([2, 15, 28, 40, 55, 68])
    return (r[:, None] * PIX_W + c[None, :]).reshape(-1).astype(np.uint32)


@pytest.mark.parametrize("h_loc", [2.0, 40.0])
@pytest.mark.parametrize("kind", ["random", "grid"])
@pytest.mark.parametrize("fmt", pix_cases.FORMATS)
def test_pixel_formats_against_fp64(ctx, fmt, kind, h_loc):
    """k_degree_entrywise<G> on 70 x 45 (no multiple of EW_COLS) with p = 257 random and p = 24 grid samples, at h_loc 2 (radius 21: real
    windows) and 40, all rows and the shard [7, 31); value-weighted and weighted sums are refused."""
    img, kernel, h_val, mod = _pix_guide(fmt)
    idx = _pix_idx(kind)
    g = dref.gamma("pix", fmt=fmt)
    for shard in (None, (7, 31)):
        ref = _ref(("pix", fmt, kind, h_loc, shard), img, idx, h_loc, h_val, rows=shard, kern=mod.kernel)
        _, BD, _, _ = dref.bounds("pix", ref, fmt=fmt)
        D, _, info = _call(ctx, img, idx, kernel=kernel, h_loc=h_loc, h_val=h_val, rows=shard)
        r0, r1 = shard or (0, PIX_H)
        assert (info["path"], info["chunks"]) == (glf.DEG_ENTRYWISE, -(-(r1 - r0) // 16))
        assert info["entries_evaluated"] >= ref.pairs
        if h_loc == 2.0 and kind == "random" and shard is None:
            assert info["entries_evaluated"] < float(idx.size) * PIX_H * PIX_W      # real windows
        _within("pix " + fmt, "%s/h_loc %g/rows %s" % (kind, h_loc, shard), "D", D, ref.D, BD, g)
        D1, _, _ = _call(ctx, img, idx, kernel=kernel, h_loc=h_loc, h_val=h_val, rows=shard, skip=1)
        assert np.array_equal(_bits(D1), _bits(D))
    if h_loc == 40.0:
        _refused(ctx, glf.ERR_UNSUPPORTED, img, idx, kernel=kernel, h_val=h_val, ysum=True)
        _refused(ctx, glf.ERR_UNSUPPORTED, img, idx, kernel=kernel, h_val=h_val, plane=np.ones((PIX_H, PIX_W), dtype=np.float32))


@pytest.mark.parametrize("h_loc", [2.0, 40.0])
@pytest.mark.parametrize("ffmt,ifmt", [("f32", "u16"), ("rgbf32", "rgb8")])
def test_integer_valued_floats_give_the_integer_formats_bits(ctx, ffmt, ifmt, h_loc):
    img, ikernel, h_val, _ = pix_cases.pix_case(ifmt, PIX_W, PIX_H, 6)
    fkernel = glf.KERNEL_BILATERAL_F32 if ffmt == "f32" else glf.KERNEL_BILATERAL_RGBF32
    for kind in ("random", "grid"):
        idx = _pix_idx(kind)
        Di, _, _ = _call(ctx, img, idx, kernel=ikernel, h_loc=h_loc, h_val=h_val)
        Df, _, _ = _call(ctx, img.astype(np.float32), idx, kernel=fkernel, h_loc=h_loc, h_val=h_val)
        assert np.array_equal(_bits(Di), _bits(Df)), (ffmt, kind)


def test_nlm_against_the_oracle(ctx):
    w, h = 37, 29
    img, idx = glf.synth_image(w, h, seed=2), glf.Sampling(w, h, 20)
    assert idx.size == 20
    prm = orc.default_params(orc.NLM)
    D, _, info = _call(ctx, img, idx, kernel=glf.KERNEL_NLM, h_loc=prm.h_loc, h_val=prm.h_val)
    assert info["path"] == glf.DEG_NLM and info["entries_evaluated"] == 20.0 * w * h
    ref = dref.Reference()
    ref.D, ref.Uy, ref.Us, ref.Uabs, ref.smax, ref.rows, ref.width = orc.degree(img, idx, prm), np.zeros(20), np.zeros(20), np.zeros(20), 0.0, (0, h), w
    g, BD, _, _ = dref.bounds("nlm", ref, h_val=prm.h_val)
    _within("nlm", "37x29", "D", D, ref.D, BD, g)
    shard = (5, 20)
    ref.D, ref.rows = orc.degree(img, idx, prm, row0=shard[0], row1=shard[1]), shard
    g, BD, _, _ = dref.bounds("nlm", ref, h_val=prm.h_val)
    D, _, info = _call(ctx, img, idx, kernel=glf.KERNEL_NLM, h_loc=prm.h_loc, h_val=prm.h_val, rows=shard)
    _within("nlm", "37x29/rows 5-20", "D", D, ref.D, BD, g)


# ---- refusals and the old entry point -----------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(ctx):
    w, h, rows, cols, h_loc, idx = dref.shape("fives")
    img, _ = _guide("synth", w, h)
    ctx.set_tuning(DEG_PATH="grid")
    one = np.ones((h, w), dtype=np.float32)
    for rows_ in ((5, 5), (9, 4), (0, h + 1), (h, h + 2)):
        _refused(ctx, glf.ERR_INVALID, img, idx, rows=rows_)
    bad = idx.copy()
    bad[[3, 4]] = bad[[4, 3]]
    _refused(ctx, glf.ERR_INVALID, img, bad)
    bad = idx.copy()
    bad[-1] = w * h
    _refused(ctx, glf.ERR_INVALID, img, bad)
    _refused(ctx, glf.ERR_INVALID, img, idx, kernel=8)
    _refused(ctx, glf.ERR_INVALID, img, idx, kernel=-1)
    _refused(ctx, glf.ERR_UNSUPPORTED, img[:2, :].copy(), np.array([1, 5, 60], dtype=np.uint32), kernel=glf.KERNEL_NLM)
    nan = img.astype(np.float32)
    nan[7, 7] = np.nan
    _refused(ctx, glf.ERR_INVALID, nan, idx, kernel=glf.KERNEL_BILATERAL_F32)
    _refused(ctx, glf.ERR_INVALID, img, idx, plane=one, ysum=True)
    _refused(ctx, glf.ERR_UNSUPPORTED, img, _random_idx(w, h, 24, 3), plane=one)                           # not a grid
    _refused(ctx, glf.ERR_UNSUPPORTED, img, _random_idx(w, h, 24, 3), ysum=True)
    _refused(ctx, glf.ERR_UNSUPPORTED, img.astype(np.uint16), idx, kernel=glf.KERNEL_BILATERAL_U16, plane=one)   # not a grey kernel
    _refused(ctx, glf.ERR_UNSUPPORTED, img, idx, kernel=glf.KERNEL_NLM, plane=one)
    D, _, info = _call(ctx, img, idx, DEG_PATH="grid")                                                      # and the context still works
    assert info["path"] == glf.DEG_GRID


def test_agrees_with_compute_affinity_matrices(ctx):
    """glf_Degree_ex(all rows, skip 0) is glf_ComputeAffinityMatrices' degree, bit for bit: the grid form and a pixel format."""
    w, h, rows, cols, h_loc, idx = dref.shape("fives")
    img, _ = _guide("synth", w, h)
    D, _, info = _call(ctx, img, idx, DEG_PATH="grid")
    assert info["path"] == glf.DEG_GRID
    d_img = ctx.to_device(img)
    _, K_B = ctx.ComputeAffinityMatrices(d_img, idx, want_KA=False)
    assert np.array_equal(_bits(ctx.degree_of(K_B)), _bits(D))
    ctx.destroy(K_B)
    ctx.reset_tuning()
    img, kernel, h_val, _ = _pix_guide("u16")
    idx = _pix_idx("random")
    D, _, _ = _call(ctx, img, idx, kernel=kernel, h_val=h_val)
    d_img = _dev(ctx, img)
    _, K_B = ctx.ComputeAffinityMatrices(d_img, idx, want_KA=False, kernel=kernel, h_val=h_val)
    assert np.array_equal(_bits(ctx.degree_of(K_B)), _bits(D))
    ctx.destroy(K_B)
