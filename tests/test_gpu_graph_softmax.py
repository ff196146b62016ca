"""Softmax read-out on a graph handle (glf_graph_softmax / Graph.softmax, .soft_assign, .mean_field): the class probabilities, the
log-sum-exp and the entropy of up to 32 score planes ident_j s_j + Phi a_j (+ bias_j), formed in registers in one pass over Phi
(k_graph_softmax: k_graph_classify up to its scores, then a softmax epilogue) and never written.

Shapes: those of tests/test_gpu_graph_classify.py -- 61 x 47 at ld 32 / 64 / 128 / 256 and `tiny`, both storages; 509 x 515 in one
test, so that waves run their tile loop more than once. Every raw call writes into buffers pre-filled with a sentinel, so that
"untouched" and "every pixel written" are both asserted.

The scores have glf_graph_synthesize's bits (plus one f32 addition of the bias), so test 1 takes z = synthesize's output, adds the
bias in f32, and compares with the f64 softmax of those very numbers under the bounds of tests/test_softmax_ref.py (derived in
DESIGN.md, "Softmax read-out"): what is left is the epilogue's own arithmetic. Each case prints the largest error / bound.
"argmax_j p_j is classify's label wherever its margin is > 0" is asserted as: p at the label is the largest p (score_j < best gives
t_j < 0 and e_j <= 1 = e_label, exactly), and the label is numpy's argmax wherever the largest p is unique; a margin of a few ulps
leaves two classes with the same p, where an argmax is not defined.

Where a test compares with f64 on the handle's own Phi (6, 7), the scores differ from the f64 ones by err_j. With e = max_j err_j
and E = exp(2 beta e) - 1 (asserted <= 1/2): d ln p_j = beta (dz_j - sum_i p_i dz_i), so p_j moves by at most p_j E; lse is
1-Lipschitz in beta z under the maximum norm, so it moves by at most beta e; and with p'_j = p_j (1 + d_j), |d_j| <= E, sum_j p_j d_j = 0,
H' - H = -sum_j p_j d_j ln p_j - sum_j p_j ((1 + d_j) ln(1 + d_j) - d_j), at most E sum_j p_j |ln p_j| + E^2. These terms are added to
test 1's bounds, evaluated on the f64 scores.

tests/test_softmax_ref.py is an independent numpy reference that this file imports; it names no symbol of the library and therefore
passes with or without the feature. The tests of this file and of tests/test_graph_softmax_abi.py fail without it."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
from test_gpu_graph import SHAPES, _grey_graph, _opt, _phi64  # noqa: E402
from test_gpu_graph_classify import _bits, _coeffs, _handle, _halves, _ident_planes, _same  # noqa: E402
from test_gpu_graph_cluster import TWO_TONE_SEED, _two_tone  # noqa: E402
from test_gpu_graph_compact import LD_SHAPES, _pair  # noqa: E402
from test_softmax_ref import U, bounds, exact, fractions  # noqa: E402

ALL_SHAPES = LD_SHAPES + ["tiny"]
STORAGES = ["f32", "compact"]
SENTINEL = -77.0
KEYS = ("prob", "lse", "entropy")
BETAS = (0.25, 1.0, 8.0)


def _raw(g, a, ident=None, plane=None, planes=None, bias=None, beta=1.0, want=KEYS, k=None, nplanes=None):
    """glf_graph_softmax itself on sentinel-filled buffers -> (status, dict of all three buffers)."""
    a = None if a is None else np.ascontiguousarray(np.atleast_2d(np.asarray(a, dtype=np.float64)))
    k = a.shape[0] if k is None else k
    h, w = g.info["height"], g.info["width"]
    dev = g.ctx.device
    out = {"prob": torch.full((max(min(k, 32), 1), h, w), SENTINEL, dtype=torch.float32, device=dev),
           "lse": torch.full((h, w), SENTINEL, dtype=torch.float32, device=dev),
           "entropy": torch.full((h, w), SENTINEL, dtype=torch.float32, device=dev)}
    pl = np.full(max(k, 1), -1, dtype=np.int32) if plane is None else np.ascontiguousarray(plane, dtype=np.int32)
    idn = np.zeros(max(k, 1), dtype=np.float32) if ident is None else np.ascontiguousarray(ident, dtype=np.float32)
    bs = None if bias is None else np.ascontiguousarray(bias, dtype=np.float64)
    if nplanes is None:
        nplanes = 0 if planes is None else planes.shape[0]
    torch.cuda.synchronize()
    rc = glf._lib.glf_graph_softmax(g._g, C.c_int(k), glf._ptr(a), glf._ptr(idn), glf._ptr(pl), C.c_int(nplanes),
                                    C.c_void_p(planes.data_ptr()) if planes is not None else None, glf._ptr(bs), C.c_double(beta),
                                    *[C.c_void_p(out[key].data_ptr()) if key in want else None for key in KEYS])
    torch.cuda.synchronize()
    return rc, out


def _ok(g, *args, **kw):
    rc, out = _raw(g, *args, **kw)
    assert rc == glf.OK, (rc, glf._lib.glf_ctx_last_error(g.ctx._ctx).decode())
    return out


def _untouched(out, keys=KEYS):
    return all(bool(torch.all(out[key] == SENTINEL)) for key in keys)


def _np(x):
    return x.detach().cpu().numpy()


def _scores(g, a, ident, plane, planes, bias):
    """The library's own scores as f32 numpy [k, N]: synthesize's output, the bias added in f32."""
    z = _np(g.synthesize(a, ident, plane, planes)).reshape(a.shape[0], -1)
    if bias is not None:
        z = (z + np.asarray(bias, dtype=np.float64).astype(np.float32)[:, None]).astype(np.float32)
    return z


def _check_against(out, x, what, score_err=None, worst=None):
    """Test 1's comparison of one call's outputs with exact()'s dict x; score_err [N]: the largest error of a pixel's scores against
    the ones x was made from (tests 6 and 7), which widens the three bounds as the module text derives; None for the plain bounds.
    -> the three fractions."""
    k = x["p"].shape[0]
    p, lse, ent = (_np(out[key]).astype(np.float64) for key in KEYS)
    p = p.reshape(k, -1)
    if score_err is None:
        fr = fractions(p, lse.reshape(-1), ent.reshape(-1), x)
        bp = bounds(x)[0]
    else:
        E = np.expm1(2.0 * x["beta"] * score_err)
        assert float(E.max()) <= 0.5, (what, float(E.max()))
        bp, blse, bh = bounds(x)
        bp = bp + x["p"] * E
        blse = blse + x["beta"] * score_err
        plnp = -(x["p"] * np.log(np.where(x["p"] > 0, x["p"], 1.0))).sum(axis=0)
        bh = bh + E * plnp + E * E
        fr = (float((np.abs(p - x["p"]) / bp).max()), float((np.abs(lse.reshape(-1) - x["lse"]) / blse).max()),
              float((np.abs(ent.reshape(-1) - x["entropy"]) / bh).max()))
    print("%s: largest error / bound: p %.3f lse %.3f entropy %.3f" % (what, *fr))
    assert max(fr) <= 1.0, (what, fr)
    assert np.all(p >= 0) and np.all(p <= 1), what
    assert np.abs(p.sum(axis=0) - 1.0).max() <= (bp.sum(axis=0) + k * 2.0 ** -52).max(), what
    if worst is not None:
        for i in range(3):
            worst[i] = max(worst[i], fr[i])
    return fr


# ---- 1. against fp64 of the library's own scores ------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_against_f64_of_the_own_scores(shape, storage):
    rng = np.random.default_rng(200 + SHAPES[shape][5])
    worst = [0.0, 0.0, 0.0]
    with glf.Context(0) as ctx:
        g, phi, d_sig = _handle(ctx, shape, storage)
        m = g.info["m"]
        for k in (1, 2, 5, 31, 32):
            a = 3.0 * _coeffs(phi, m, k, rng)
            idn, pl = _ident_planes(k)
            bias = rng.normal(size=k)
            for ident, plane, planes, bs in ((None, None, None, None), (idn, pl, d_sig, bias)):
                z = _scores(g, a, ident, plane, planes, bs)
                assert np.isfinite(z).all()
                cls = g.classify(a, ident, plane, planes, bs, want=("label", "margin"))
                label, margin = _np(cls["label"]).reshape(-1), _np(cls["margin"]).reshape(-1)
                for beta in BETAS:
                    what = "%s %s k %d%s beta %g" % (shape, storage, k, " planes+bias" if bs is not None else "", beta)
                    out = _ok(g, a, ident, plane, planes, bs, beta)
                    _check_against(out, exact(z, beta), what, worst=worst)
                    p = _np(out["prob"]).reshape(k, -1)
                    clear = margin > 0
                    top = p.max(axis=0)
                    assert np.all(p[label, np.arange(p.shape[1])][clear] == top[clear]), what
                    unique = clear & ((p == top).sum(axis=0) == 1)
                    assert np.all(p.argmax(axis=0)[unique] == label[unique]), what
                    if k == 1:
                        assert bool(torch.all(out["prob"] == 1)) and not _bits(out["entropy"]).any(), what
                        _same(out["lse"].reshape(-1), (np.float32(beta) * z[0]).astype(np.float32) + np.float32(0.0), what + ": lse of one class")
        # the Python call is the raw call
        a = _coeffs(phi, m, 5, rng)
        idn, pl = _ident_planes(5)
        raw, got = _ok(g, a, idn, pl, d_sig, None, 2.0), g.softmax(a, idn, pl, d_sig, beta=2.0, want=KEYS)
        assert sorted(got) == sorted(KEYS) and all(got[key].dtype == torch.float32 for key in KEYS)
        assert sorted(g.softmax(a)) == ["prob"]
        assert tuple(got["prob"].shape) == (5, SHAPES[shape][1], SHAPES[shape][0]) and tuple(got["lse"].shape) == tuple(got["entropy"].shape) == tuple(got["prob"].shape[1:])
        for key in KEYS:
            _same(got[key], raw[key], "Graph.softmax %s" % key)
        g.close()
    print("%s %s: largest error / bound over all cases: p %.3f lse %.3f entropy %.3f" % (shape, storage, *worst))


# ---- 2. bit-for-bit contracts --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", STORAGES)
def test_bit_for_bit_contracts(storage):
    rng = np.random.default_rng(57)
    with glf.Context(0) as ctx:
        g, phi, d_sig = _handle(ctx, "ld64", storage)
        m, k = g.info["m"], 5
        a = _coeffs(phi, m, k, rng)
        ident, plane = _ident_planes(k)
        bias = rng.normal(size=k)
        base = _ok(g, a, ident, plane, d_sig, bias, 1.5)
        again = _ok(g, a, ident, plane, d_sig, bias, 1.5)
        for key in KEYS:
            _same(again[key], base[key], "second call: %s" % key)
        # any subset of the outputs: the bits of the full call, the other buffers untouched
        for want in (("prob",), ("lse",), ("entropy",), ("prob", "lse"), ("prob", "entropy"), ("lse", "entropy")):
            part = _ok(g, a, ident, plane, d_sig, bias, 1.5, want=want)
            for key in want:
                _same(part[key], base[key], "%s of %s" % (key, want))
            assert _untouched(part, [key for key in KEYS if key not in want]), want
        # a class that cannot matter: its e is an exact +0, and no other bit moves (slot 5 sits in the other half-wave's registers)
        a6 = np.concatenate([a, _coeffs(phi, m, 1, rng)])
        more = _ok(g, a6, np.append(ident, np.float32(1.0)), np.append(plane, np.int32(1)), d_sig, np.append(bias, -1e30), 1.5)
        assert not _bits(more["prob"][k]).any()
        _same(more["prob"][:k], base["prob"], "appended class: prob")
        _same(more["lse"], base["lse"], "appended class: lse")
        _same(more["entropy"], base["entropy"], "appended class: entropy")
        # scores halved, beta doubled: the same t, bit for bit
        half = _ok(g, a / 2, ident / np.float32(2), plane, d_sig, bias / 2, 3.0)
        _same(half["prob"], base["prob"], "scaled call: prob")
        _same(half["entropy"], base["entropy"], "scaled call: entropy")
        g.close()


@pytest.mark.parametrize("variant", ["plain", "scaled"])
@pytest.mark.parametrize("shape", ["ld64", "ld256"])
def test_compact_handle_is_its_f32_twin(shape, variant):
    rng = np.random.default_rng(43)
    with glf.Context(0) as ctx:
        gc, gt, _, d_sig, _, _ = _pair(ctx, shape, variant)
        a = _coeffs(_phi64(gt), gt.info["m"], 7, rng)
        ident, plane = _ident_planes(7)
        bias = rng.normal(size=7) * 0.1
        oc, ot = _ok(gc, a, ident, plane, d_sig, bias, 2.0), _ok(gt, a, ident, plane, d_sig, bias, 2.0)
        assert bool(torch.isfinite(ot["prob"]).all())
        for key in KEYS:
            _same(oc[key], ot[key], "%s %s compact against its twin: %s" % (shape, variant, key))
        gc.close()
        gt.close()


# ---- 3. specials ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["tiny", "ld32"])
@pytest.mark.parametrize("k", [6, 32])
def test_specials_follow_the_rule(shape, k):
    """All-zero coefficients, identity factor 1: score_j = fmaf(1, plane_j, +0), the plane's value. A pixel with a NaN score, a +inf
    score or nothing but -inf scores is NaN in every output; every other pixel is finite, with p = +0 exactly where its score is
    -inf, and within test 1's bounds of the f64 softmax of its finite scores."""
    w, h = SHAPES[shape][:2]
    n = w * h
    rng = np.random.default_rng(5 * k + n)
    planes = rng.integers(-2, 3, size=(k, n)).astype(np.float32)
    specials = np.array([np.nan, np.inf, -np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
    hit = rng.random(planes.shape) < (0.5 / k)
    planes[hit] = specials[rng.integers(0, specials.size, int(hit.sum()))]
    planes[:, 0] = np.nan                                                        # an all-NaN pixel
    planes[:, 1] = -np.inf                                                       # nothing above -inf
    planes[:, 2] = -np.inf
    planes[4, 2] = 1.5                                                           # one score above -inf: p = 1 there
    planes[:, 3] = 1.0
    planes[k - 1, 3] = np.inf                                                    # one +inf
    planes[:, 4] = 1.0
    planes[k - 1, 4] = np.nan                                                    # one NaN, in the other half-wave for k = 6
    planes[:, 5] = -1.0                                                          # a clean pixel between them
    planes[:, n - 1] = planes[:, 2]                                              # ... and in the last, partial tile
    bad = np.isnan(planes).any(axis=0) | np.isposinf(planes).any(axis=0) | np.isneginf(planes).all(axis=0)
    assert bad[[0, 1, 3, 4]].all() and not bad[[2, 5, n - 1]].any() and 0.05 < bad.mean() < 0.6
    with glf.Context(0) as ctx:
        g, _, _ = _grey_graph(ctx, shape)
        d_planes = torch.from_numpy(planes.reshape(k, h, w)).to(ctx.device)
        out = _ok(g, np.zeros((k, g.info["m"])), np.ones(k, dtype=np.float32), np.arange(k, dtype=np.int32), d_planes, None, 1.0)
        g.close()
    p, lse, ent = _np(out["prob"]).reshape(k, n), _np(out["lse"]).reshape(n), _np(out["entropy"]).reshape(n)
    assert np.isnan(p[:, bad]).all() and np.isnan(lse[bad]).all() and np.isnan(ent[bad]).all()
    good = ~bad
    assert np.isfinite(p[:, good]).all() and np.isfinite(lse[good]).all() and np.isfinite(ent[good]).all()
    gone = np.isneginf(planes) & good[None, :]
    assert gone.any() and not p[gone].view(np.uint32).any()                       # +0, the bit pattern
    assert p[4, 2] == 1 and p[4, n - 1] == 1 and lse[2] == np.float32(1.5) and not ent[[2]].view(np.uint32).any()
    x = exact(planes[:, good], 1.0)
    fr = fractions(p[:, good], lse[good], ent[good], x)
    print("specials %s k %d: %d NaN pixels of %d; the others' largest error / bound: p %.3f lse %.3f entropy %.3f" % (shape, k, int(bad.sum()), n, *fr))
    assert max(fr) <= 1.0


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched():
    rng = np.random.default_rng(10)
    with glf.Context(0) as ctx:
        g, phi, d_sig = _handle(ctx, "ld64", "f32")
        m, k = g.info["m"], 4
        h, w = g.info["height"], g.info["width"]
        a = _coeffs(phi, m, k, rng)
        ident, plane = np.ones(k, dtype=np.float32), np.array([0, 1, 2, -1], dtype=np.int32)
        bad_plane, low_plane, huge = plane.copy(), plane.copy(), a.copy()
        bad_plane[2] = 3                                                         # = nplanes
        low_plane[0] = -2
        huge[1, 3] = 1e60                                                        # finite in f64, not in f32
        a33 = _coeffs(phi, m, 33, rng)
        cases = {
            "k = 0": (dict(a=a, k=0), "k = 0"), "k = 33": (dict(a=a33, k=33), "k = 33"), "k = -1": (dict(a=a, k=-1), "k = -1"),
            "plane[j] = nplanes": (dict(a=a, ident=ident, plane=bad_plane, planes=d_sig), "plane[2]"),
            "plane[j] = -2": (dict(a=a, ident=ident, plane=low_plane, planes=d_sig), "plane[0]"),
            "planes without d_planes": (dict(a=a, ident=ident, plane=plane, planes=None, nplanes=3), "identity"),
            "NaN bias": (dict(a=a, bias=[0.0, np.nan, 0.0, 0.0]), "bias"), "Inf bias": (dict(a=a, bias=[0.0, 0.0, 0.0, -np.inf]), "bias"),
            "a bias beyond f32": (dict(a=a, bias=[1e60, 0.0, 0.0, 0.0]), "bias"),
            "a coefficient beyond f32": (dict(a=huge), "coefficient"), "h_a NULL": (dict(a=None, k=k), "h_a"),
            "no output": (dict(a=a, want=()), "no output"),
            "beta = 0": (dict(a=a, beta=0.0), "beta"), "beta < 0": (dict(a=a, beta=-1.0), "beta"), "beta NaN": (dict(a=a, beta=float("nan")), "beta"),
            "beta Inf": (dict(a=a, beta=float("inf")), "beta"), "beta beyond f32": (dict(a=a, beta=1e39), "beta"),
            "beta that underflows in f32": (dict(a=a, beta=1e-60), "beta"),
            "beta log2 e beyond f32": (dict(a=a, beta=3.0e38), "beta"),
        }
        last = lambda: glf._lib.glf_ctx_last_error(ctx._ctx).decode()
        for what, (kw, word) in cases.items():
            rc, out = _raw(g, **kw)
            assert rc == glf.ERR_INVALID, what
            assert "glf_graph_softmax" in last() and word in last(), (what, last())
            assert _untouched(out), what
        assert np.isfinite(np.float32(3.0e38)) and not np.isfinite(np.float32(3.0e38 * 1.4426950408889634))
        out = _ok(g, a)
        out2 = {key: out[key].clone() for key in KEYS}
        assert glf._lib.glf_graph_softmax(None, C.c_int(k), glf._ptr(a), None, glf._ptr(plane), 0, None, None, C.c_double(1.0),
                                          *[C.c_void_p(out2[key].data_ptr()) for key in KEYS]) == glf.ERR_INVALID
        torch.cuda.synchronize()
        for key in KEYS:
            _same(out2[key], out[key], "a NULL handle writes nothing")
        # the Python layer
        with pytest.raises(ValueError, match="32"):
            g.softmax(a33)
        with pytest.raises(ValueError):
            g.softmax(np.zeros((2, m + 1)))
        with pytest.raises(ValueError):
            g.softmax(a, want=("probs",))
        with pytest.raises(ValueError):
            g.softmax(a, want=())
        with pytest.raises(glf.GlfError):
            g.softmax(a, beta=0.0)
        with pytest.raises(ValueError, match="32"):
            g.soft_assign(np.zeros((33, 2)))
        with pytest.raises(ValueError):
            g.soft_assign(np.zeros((2, m + 1)))
        with pytest.raises(ValueError):
            g.soft_assign(np.zeros((2, 2)), temperature=0.0)
        with pytest.raises(ValueError):
            g.soft_assign(np.zeros((2, 2)), scale=np.ones(3))
        logits = torch.zeros((3, h, w), dtype=torch.float32, device=ctx.device)
        with pytest.raises(ValueError, match="32"):
            g.mean_field(torch.zeros((33, h, w), dtype=torch.float32, device=ctx.device))
        with pytest.raises(ValueError):
            g.mean_field(logits, compat=np.eye(2))
        with pytest.raises(ValueError):
            g.mean_field(logits, response=np.ones(m + 1))
        with pytest.raises(ValueError):
            g.mean_field(logits, init=torch.zeros((2, h, w), dtype=torch.float32, device=ctx.device))
        # nothing faulted, and the next valid call succeeds
        _check_against(_ok(g, a, ident, plane, d_sig), exact(_scores(g, a, ident, plane, d_sig, None), 1.0), "after the refusals")
        g.close()


# ---- 5. the tile loop ----------------------------------------------------------------------------------------------------------------

def test_tile_loop():
    """509 x 515 = 8192 tiles: every wave runs its tile loop more than once -- the prefetch under the MFMAs, fresh accumulators, a
    fresh best, S and A per tile. Test 1 at k = 32 with identity planes and biases, ld 64, the bounds evaluated in torch f64 on the device."""
    w, h, m, ld, k, beta = 509, 515, 40, 64, 32, 2.0
    n = w * h
    rng = np.random.default_rng(65)
    with glf.Context(0) as ctx:
        assert (n + 31) // 32 > 4 * 7 * ctx.device_info()["num_cus"]
        g = ctx.graph(ctx.to_device(glf.synth_image(w, h, seed=3)), glf.default_options(num_samples=300, num_eigvals=m, epsilon=0.1))
        assert (g.info["m"], g.info["ld"]) == (m, ld)
        a = 3.0 * _coeffs(np.array([float(g.phi[:, :m].abs().max())]), m, k, rng)
        planes = torch.from_numpy(rng.normal(size=(3, h, w)).astype(np.float32)).to(ctx.device)
        ident, plane = _ident_planes(k)
        bias = rng.normal(size=k)
        z = g.synthesize(a, ident, plane, planes) + torch.from_numpy(bias.astype(np.float32)).to(ctx.device)[:, None, None]   # one f32 addition
        out = _ok(g, a, ident, plane, planes, bias, beta)
        g.close()
        # tests/test_softmax_ref.py's exact() and bounds(), in torch f64
        z = z.double().reshape(k, n)
        best = z.max(dim=0).values
        t = beta * 1.4426950408889634074 * (z - best)
        e = torch.exp2(t)
        S = e.sum(dim=0)
        p, lnS = e / S, torch.log(S)
        wsum = (p * t.abs()).sum(dim=0)
        lse, ent = beta * best + lnS, lnS + np.log(2.0) * wsum
        assert float(t.min()) > -126.0                                           # (no clipped class: at = |t|)
        eps = 2 * U + 3 * np.log(2.0) * t.abs() * U
        eps_s = eps.max(dim=0).values + 16 * U
        so = 1.0 + 2.0 ** -10
        bp = p * (eps + eps_s + 3 * U) * so + 2.0 ** -126
        blse = (eps_s + 3 * U * lnS + 2 * U * (beta * best).abs() + U * lse.abs()) * so + 2.0 ** -120
        bh = (np.log(2.0) * (p * t.abs() * (eps + eps_s + 22 * U)).sum(dim=0) + eps_s + 2 * U * lnS + 3 * U * (lnS + np.log(2.0) * wsum)) * so + 2.0 ** -100
        got_p = out["prob"].double().reshape(k, n)
        fr = (float(((got_p - p).abs() / bp).max()), float(((out["lse"].double().reshape(n) - lse).abs() / blse).max()),
              float(((out["entropy"].double().reshape(n) - ent).abs() / bh).max()))
        print("509 x 515 k 32: largest error / bound: p %.3f lse %.3f entropy %.3f" % fr)
        assert all(f <= 1.0 for f in fr), fr                                      # (a NaN fails the comparison)
        assert float(got_p.min()) >= 0 and float(got_p.max()) <= 1
        assert float((got_p.sum(dim=0) - 1.0).abs().max()) <= float(bp.sum(dim=0).max()) + k * 2.0 ** -52


# ---- 6. soft memberships -------------------------------------------------------------------------------------------------------------

def _score_err(phi, ld, a, bias=None, logit=None):
    """err_j [k, N] of the library's scores against exact arithmetic on its own Phi and coefficients: synthesize's (ld + 4) u
    (|ident s| + |Phi| |a|), plus for a bias the rounding of fl32(bias) and of the addition, u |bias| + u (|bias| + |Phi| |a|)."""
    mag = np.abs(a) @ np.abs(phi).T + (0.0 if logit is None else np.abs(logit))
    err = (ld + 4) * U * mag
    if bias is not None:
        err = err + U * (2 * np.abs(bias)[:, None] + mag)
    return err


@pytest.mark.parametrize("storage", STORAGES)
def test_soft_assign_against_f64(storage):
    rng = np.random.default_rng(66)
    with glf.Context(0) as ctx:
        g, phi, _ = _handle(ctx, "ld64", storage)
        m, ld = g.info["m"], g.info["ld"]
        n = phi.shape[0]
        for dim in (1, m):
            for k in (2, 8):
                scale = rng.uniform(0.5, 2.0, size=dim) / np.abs(phi[:, :dim]).max()     # the embedded rows are of order one
                y = phi[:, :dim] * scale[None, :]
                cent = y[rng.integers(0, n, size=k)] + 0.05 * rng.normal(size=(k, dim))   # centres near rows of the embedding
                T = 0.5 * float(np.median(((y[:, None, :] - cent[None, :, :]) ** 2).sum(axis=2)))
                what = "soft_assign %s dim %d k %d" % (storage, dim, k)
                out = g.soft_assign(cent, scale, T, want=KEYS)
                assert tuple(out["prob"].shape) == (k, g.info["height"], g.info["width"])
                d64 = ((y[:, None, :] - cent[None, :, :]) ** 2).sum(axis=2).T                  # [k, N]
                a = np.zeros((k, m))
                a[:, :dim] = 2.0 * cent * scale[None, :] / T
                bias = -(cent * cent).sum(axis=1) / T
                err = _score_err(phi, ld, a, bias)
                extra = np.expm1(2.0 * err.max(axis=0))
                x = exact(-d64 / T, 1.0)                                         # (the row's own |y|^2 / T is common to the classes)
                own = (y * y).sum(axis=1) / T                                    # ... and the call's scores, hence its lse, are without it
                x["lse"], x["best"] = x["lse"] + own, x["best"] + own
                _check_against(out, x, what + " against f64 memberships", score_err=err.max(axis=0))
                assert sorted(g.soft_assign(cent, scale, T)) == ["prob"]
                # ... and against the route through distance planes: quadform, then torch.softmax; its planes carry quadform's own
                # bound (include/glf.h) into the softmax in the same way, and torch's f32 softmax a few roundings of its own
                R = np.zeros((m, dim))
                R[np.arange(dim), np.arange(dim)] = scale
                q = g.quadform(R, cent)
                theirs = _np(torch.softmax(-q / np.float32(T), dim=0)).reshape(k, n).astype(np.float64)
                xs = np.abs(y[:, None, :] - cent.astype(np.float32).astype(np.float64)[None, :, :])   # |x*_c| [N, k, dim]
                delta = (ld + 4) * U * np.abs(y)[:, None, :]
                ec = delta + U * (xs + delta)
                tr = U * np.abs(cent)[None, :, :]                                # fl32(t_k) against t_k
                qerr = ((2 * xs * (ec + tr) + ec * ec + tr * tr).sum(axis=2) + (dim + 1) * U * ((xs + ec) ** 2).sum(axis=2)).T + 2 * U * d64   # (+ the division by fl32(T))
                their_bound = x["p"] * (np.expm1(2.0 * qerr.max(axis=0) / T) + (k + 16) * U) + 2.0 ** -126
                ours = _np(out["prob"]).reshape(k, n).astype(np.float64)
                both = bounds(x)[0] + x["p"] * extra + their_bound
                worst = float((np.abs(ours - theirs) / both).max())
                print("%s against torch.softmax(-quadform / T): largest difference / summed bounds %.3f" % (what, worst))
                assert worst <= 1.0, what
        g.close()


# ---- 7. mean field, step by step -----------------------------------------------------------------------------------------------------

def _test_logits(w, h):
    """refine_logits' test logits: k = 3, one-hot halves plus sigma = 0.5 noise (rng 77); the third class is pure noise."""
    rng = np.random.default_rng(77)
    halves = _halves(w, h)
    logits = 0.5 * rng.normal(size=(3, w * h))
    logits[0] += halves == 0
    logits[1] += halves == 1
    return logits.astype(np.float32), halves


def _mean_field_step64(what, step, q_prev, wgt, phi, ld, logits, M, g, ident, beta):
    """One iteration's outputs against the f64 step from the previous Q [k, N]: c64 = (w Q_prev) Phi, a64 = M (g o c64), s64 = ident
    logit + Phi a64. The returned coefficients must lie within project_wide's own bound of a64 (include/glf.h: per entry
    ((GLF_GRAPH_NORMAL_CHAIN + 3) u + N 2^-51) sum_px |w Q Phi|, pushed through |M| and |g|; the host mixing is f64), so that an error
    of the host mixing cannot hide in the score error; the scores then differ from s64 by at most
    err_j = (ld + 4) u (|ident logit_j| + |Phi| |a_j|) + |Phi| |a_j - a64_j| (refine_logits' test expression)."""
    n = phi.shape[0]
    a = step["coeffs"]
    wq = q_prev * wgt[None, :]
    a64 = M @ (g[None, :] * (wq @ phi))
    cb = ((glf.GRAPH_NORMAL_CHAIN + 3) * U + n * 2.0 ** -51) * (np.abs(wq) @ np.abs(phi))
    ab = np.abs(M) @ (np.abs(g)[None, :] * cb) + 1e-12 * np.abs(a64)
    print("%s: max |a - a64| / max |a64| %.3e, largest |a - a64| / project_wide's bound %.3f" %
          (what, float(np.abs(a - a64).max() / np.abs(a64).max()), float((np.abs(a - a64) / ab).max())))
    assert np.all(np.abs(a - a64) <= ab), what
    l64 = ident * logits.astype(np.float64)
    s64 = l64 + a64 @ phi.T
    err = _score_err(phi, ld, a, logit=l64) + np.abs(a - a64) @ np.abs(phi).T
    return _check_against(step, exact(s64, beta), what, score_err=err.max(axis=0))


def test_mean_field_step_by_step():
    """Every iteration's Q, lse and entropy against an f64 step from the library's own previous Q, so that nothing accumulates
    (_mean_field_step64); then one step with every argument off its default -- a full compatibility matrix, a response that is not
    1 - lam, an identity factor of 0.5, a caller's weight -- against the same f64 step, and the weight paths bit for bit."""
    w, h = SHAPES["ld32"][:2]
    n, k, coupling, beta, steps = w * h, 3, 2.0, 1.5, 4
    logits, _ = _test_logits(w, h)
    with glf.Context(0) as ctx:
        g = ctx.graph(ctx.to_device(_two_tone(TWO_TONE_SEED)), _opt("ld32"))
        m, ld = g.info["m"], g.info["ld"]
        phi, lam = _phi64(g), g.eigenvalues
        d_logits = torch.from_numpy(logits.reshape(k, h, w)).to(ctx.device)
        wgt = np.ones(n)
        wgt[g.samples().astype(np.int64)] = 0.0
        q0 = g.mean_field(d_logits, coupling, beta=beta, max_iter=0, want=KEYS)
        assert q0["iterations"] == 0 and not q0["converged"] and not q0["coeffs"].any()
        _check_against(q0, exact(logits, beta), "mean_field: Q0 is the softmax of the logits")
        whole = g.mean_field(d_logits, coupling, beta=beta, max_iter=steps, tol=0.0, want=KEYS)
        assert whole["iterations"] == steps and not whole["converged"] and whole["changes"].shape == (steps,)
        prev = q0["prob"]
        for it in range(1, steps + 1):
            step = g.mean_field(d_logits, coupling, beta=beta, max_iter=1, tol=0.0, init=prev, want=KEYS)
            q_prev = _np(prev).reshape(k, n).astype(np.float64)
            _mean_field_step64("mean_field step %d" % it, step, q_prev, wgt, phi, ld, logits, coupling * np.eye(k), 1.0 - lam, 1.0, beta)
            prev = step["prob"]
        for key in KEYS:
            _same(prev if key == "prob" else step[key], whole[key], "the chained steps are the one call: %s" % key)
        np.testing.assert_array_equal(step["coeffs"], whole["coeffs"])
        # a caller's compatibility matrix that is the Potts one, and a stop by tol
        same = g.mean_field(d_logits, compat=coupling * np.eye(k), beta=beta, max_iter=steps, tol=0.0)
        _same(same["prob"], whole["prob"], "compat = coupling I")
        loose = g.mean_field(d_logits, coupling, beta=beta, max_iter=steps, tol=1e30)
        assert loose["iterations"] == 1 and loose["converged"]
        # every argument off its default, one step from Q0
        rng = np.random.default_rng(78)
        M = np.array([[1.5, -0.5, 0.25], [-0.75, 2.0, 0.0], [0.5, -0.25, 1.0]])
        resp = rng.uniform(0.2, 1.5, size=m) * np.where(np.arange(m) % 3 == 1, -1.0, 1.0)
        cw = rng.uniform(0.25, 2.0, size=n).astype(np.float32)
        d_cw = torch.from_numpy(cw.reshape(h, w)).to(ctx.device)
        q_prev = _np(q0["prob"]).reshape(k, n).astype(np.float64)
        step = g.mean_field(d_logits, compat=M, response=resp, weight=d_cw, ident=0.5, beta=beta, max_iter=1, tol=0.0, init=q0["prob"], want=KEYS)
        _mean_field_step64("mean_field, full compat, response, weight, ident 0.5", step, q_prev, cw.astype(np.float64) * wgt, phi, ld, logits,
                           M, resp, 0.5, beta)
        keep = g.mean_field(d_logits, compat=M, response=resp, weight=d_cw, exclude_samples=False, ident=0.5, beta=beta, max_iter=1, tol=0.0,
                            init=q0["prob"], want=KEYS)
        _mean_field_step64("mean_field, the same with the sample pixels kept", keep, q_prev, cw.astype(np.float64), phi, ld, logits, M, resp, 0.5, beta)
        assert not np.array_equal(keep["coeffs"], step["coeffs"])
        # the weight paths, bit for bit: the sample mask as the caller's weight, and a weight of ones under the mask
        d_mask = torch.from_numpy(wgt.astype(np.float32).reshape(h, w)).to(ctx.device)
        for what, kw in (("weight = the sample mask, exclude_samples off", dict(weight=d_mask, exclude_samples=False)),
                         ("weight = ones", dict(weight=torch.ones_like(d_mask)))):
            other = g.mean_field(d_logits, coupling, beta=beta, max_iter=steps, tol=0.0, want=KEYS, **kw)
            for key in KEYS:
                _same(other[key], whole[key], "%s: %s" % (what, key))
            np.testing.assert_array_equal(other["coeffs"], whole["coeffs"])
        g.close()


# ---- 8. mean field, end to end -------------------------------------------------------------------------------------------------------

def test_mean_field_end_to_end():
    """The basis made orthonormal off the sample pixels, then 8 mean-field steps at coupling 4 on refine_logits' test logits: the f64
    run must lift the agreement with the two halves by at least 0.05 over the raw logits' argmax (a condition on the inputs), and the
    library must give the f64 labels wherever the f64 top-two score gap exceeds 1e-3 (a chosen threshold, about 1000 times the f32
    score error; test 7 carries the derived bounds), with at most 1 % of the pixels left out."""
    w, h = SHAPES["ld32"][:2]
    n, k, coupling, steps = w * h, 3, 4.0, 8
    logits, halves = _test_logits(w, h)
    with glf.Context(0) as ctx:
        g = ctx.graph(ctx.to_device(_two_tone(TWO_TONE_SEED)), _opt("ld32"))
        samples = g.samples().astype(np.int64)
        wgt = np.ones(n, dtype=np.float32)
        wgt[samples] = 0.0
        d_w = torch.from_numpy(wgt.reshape(h, w)).to(ctx.device)
        G = g.normal_equations(d_w)[0]
        g.transform(glf.basis_orthonormal(G), g.eigenvalues)
        m = g.info["m"]
        phi = _phi64(g)
        d_logits = torch.from_numpy(logits.reshape(k, h, w)).to(ctx.device)
        out = g.mean_field(d_logits, coupling, response=np.ones(m), max_iter=steps, tol=0.0, want=("prob", "entropy"))
        assert out["iterations"] == steps
        label = _np(out["prob"]).reshape(k, n).argmax(axis=0)
        g.close()
    w64 = wgt.astype(np.float64)
    l64 = logits.astype(np.float64)
    q = exact(l64, 1.0)["p"]
    for _ in range(steps):
        s64 = l64 + (coupling * ((q * w64[None, :]) @ phi)) @ phi.T
        q = exact(s64, 1.0)["p"]
    srt = np.sort(s64, axis=0)
    decided = (srt[-1] - srt[-2]) > 1e-3
    left_out = 1.0 - float(decided.mean())
    label64 = s64.argmax(axis=0)
    outside = w64 > 0
    agree, agree64 = float((label == halves)[outside].mean()), float((label64 == halves)[outside].mean())
    raw = float((logits.argmax(axis=0) == halves)[outside].mean())
    wrong = int(np.count_nonzero((label != label64) & decided))
    print("mean_field end to end: agreement with the two halves outside the sample pixels %.4f (f64 %.4f; the raw logits' argmax %.4f); "
          "%.3f %% of the pixels left out, %d labels differ" % (agree, agree64, raw, 100.0 * left_out, wrong))
    assert agree64 >= raw + 0.05, "the inputs do not show the gain this test is about: f64 %.4f against raw %.4f" % (agree64, raw)
    assert left_out <= 0.01
    assert wrong == 0
    assert abs(agree - agree64) <= left_out + 1e-12
