"""Label read-out on a graph handle (glf_graph_classify / Graph.classify, .refine_logits, .propagate_labels): the winner, its score
and its margin over the runner-up of up to 32 score planes ident_j s_j + Phi a_j (+ bias_j), formed in registers in one pass over
Phi (k_graph_classify: k_graph_synthesize up to its store, then a top-two epilogue) and never written.

Shapes: those of tests/test_gpu_graph.py -- 61 x 47 = 2867 pixels (89 whole tiles and one of 19 pixels) at ld 32 / 64 / 128 / 256,
and `tiny` (160 pixels), both storages; 509 x 515 in one test, so that waves run their tile loop more than once. Every raw call
writes into buffers pre-filled with a sentinel, so that "untouched" and "every pixel written" are both asserted.

The scores have glf_graph_synthesize's bits, so most tests compare against synthesize on the same handle, bit for bit. A score of
-0 cannot be produced on the device (an accumulator starts at +0, and x + (+0) is +0 for both zeros): planes holding -0 are read
out as +0, which the expected arrays of test 2 state; tests/test_classify_ref.py covers true -0 scores on the rule itself.

The drivers (test 5) are compared with f64 on the handle's own Phi. A pixel is compared where the f64 margin exceeds
2 max_j err_j, err_j = (ld + 4) 2^-24 (|ident s_j| + |Phi| |a_j|) + |Phi| |a_j - a64_j|: the committed synthesize bound of each
competing score plus what the difference of the library's coefficients a from the f64 ones a64 (computed, not estimated) moves a
score by; a label can differ from the f64 one only where the margin is at most err_winner + err_other. The pixels left out must be
at most 1 % of the image.

No handle exists on a context with a communicator (glf_graph_build refuses it: tests/test_gpu_graph.py), so that refusal cannot be
reached through glf_graph_classify and is not repeated here."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
from test_gpu_graph import SHAPES, _grey_graph, _opt, _phi64  # noqa: E402
from test_gpu_graph_cluster import TWO_TONE_SEED, _two_tone  # noqa: E402
from test_gpu_graph_compact import LD_SHAPES, _pair  # noqa: E402

U = 2.0 ** -24
ALL_SHAPES = LD_SHAPES + ["tiny"]
STORAGES = ["f32", "compact"]
SENTINEL = -77
KEYS = ("label", "best", "margin")


def _handle(ctx, shape, storage):
    """(graph, its own Phi [N, m] in f64: Q on a compact handle, device planes [3, H, W])."""
    g, _, d_sig = _grey_graph(ctx, shape)
    if storage == "compact":
        g.compact()
        return g, g.dequantize().cpu().numpy()[:, :g.info["m"]].astype(np.float64), d_sig
    return g, _phi64(g), d_sig


def _coeffs(phi, m, k, rng):
    """a [k, m] at the scale that makes the scores Phi a of order one (the quadratic forms' _metric)."""
    return rng.normal(size=(k, m)) / (np.sqrt(m) * max(float(np.abs(phi).max()), 1e-30))


def _ident_planes(k):
    """Identity factors from {1, -0.5, 0.25} and a plane map over the three test planes with one class left without a plane."""
    plane = np.array([j % 3 for j in range(k)], dtype=np.int32)
    if k > 1:
        plane[k // 2] = -1
    return np.array([(1.0, -0.5, 0.25)[(j // 3) % 3] for j in range(k)], dtype=np.float32), plane


def _raw(g, a, ident=None, plane=None, planes=None, bias=None, want=KEYS, k=None, nplanes=None, out=None):
    """glf_graph_classify itself on sentinel-filled buffers -> (status, dict of all three buffers [H, W])."""
    a = None if a is None else np.ascontiguousarray(np.atleast_2d(np.asarray(a, dtype=np.float64)))
    k = a.shape[0] if k is None else k
    h, w = g.info["height"], g.info["width"]
    dev = g.ctx.device
    if out is None:
        out = {"label": torch.full((h, w), SENTINEL, dtype=torch.int32, device=dev),
               "best": torch.full((h, w), float(SENTINEL), dtype=torch.float32, device=dev),
               "margin": torch.full((h, w), float(SENTINEL), dtype=torch.float32, device=dev)}
    pl = np.full(max(k, 1), -1, dtype=np.int32) if plane is None else np.ascontiguousarray(plane, dtype=np.int32)
    idn = np.zeros(max(k, 1), dtype=np.float32) if ident is None else np.ascontiguousarray(ident, dtype=np.float32)
    bs = None if bias is None else np.ascontiguousarray(bias, dtype=np.float64)
    if nplanes is None:
        nplanes = 0 if planes is None else planes.shape[0]
    torch.cuda.synchronize()
    rc = glf._lib.glf_graph_classify(g._g, C.c_int(k), glf._ptr(a), glf._ptr(idn), glf._ptr(pl), C.c_int(nplanes),
                                     C.c_void_p(planes.data_ptr()) if planes is not None else None, glf._ptr(bs),
                                     *[C.c_void_p(out[key].data_ptr()) if key in want else None for key in KEYS])
    torch.cuda.synchronize()
    return rc, out


def _ok(g, *args, **kw):
    rc, out = _raw(g, *args, **kw)
    assert rc == glf.OK, (rc, glf._lib.glf_ctx_last_error(g.ctx._ctx).decode())
    return out


def _untouched(out, keys=KEYS):
    return all(bool(torch.all(out[key] == SENTINEL)) for key in keys)


def _bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view("u%d" % x.dtype.itemsize)


def _same(a, b, what):
    ia, ib = _bits(a), _bits(b)
    assert ia.dtype == ib.dtype and ia.shape == ib.shape, (what, ia.dtype, ib.dtype, ia.shape, ib.shape)
    bad = int(np.count_nonzero(ia != ib))
    assert bad == 0, "%s: %d of %d elements differ in bits" % (what, bad, ia.size)


def _lowest_argmax(y):
    """The lowest index among the largest entries along axis 0 (numpy's argmax returns the first occurrence)."""
    y = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
    return (y == y.max(axis=0)).argmax(axis=0).astype(np.int32)


def _against_synthesize(g, a, ident, plane, planes, what):
    """Test 1's comparison of one call with the handle's own synthesize; -> the outputs."""
    k = a.shape[0]
    y = g.synthesize(a, ident, plane, planes)
    assert bool(torch.isfinite(y).all())
    out = _ok(g, a, ident, plane, planes)
    top2 = torch.topk(y, min(2, k), 0)
    _same(out["best"], top2.values[0], what + ": best")
    _same(out["label"], _lowest_argmax(y), what + ": label")
    want = top2.values[0] - top2.values[1] if k > 1 else torch.full_like(y[0], float("inf"))
    _same(out["margin"], want, what + ": margin")
    return out


# ---- 1. bit for bit against glf_graph_synthesize -------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_bit_for_bit_against_synthesize(shape, storage):
    rng = np.random.default_rng(100 + SHAPES[shape][5])
    with glf.Context(0) as ctx:
        g, phi, d_sig = _handle(ctx, shape, storage)
        m = g.info["m"]
        for k in (1, 2, 5, 31, 32):
            a = _coeffs(phi, m, k, rng)
            out = _against_synthesize(g, a, None, None, None, "%s %s k %d" % (shape, storage, k))
            assert int(out["label"].min()) >= 0 and int(out["label"].max()) < k
            ident, plane = _ident_planes(k)
            _against_synthesize(g, a, ident, plane, d_sig, "%s %s k %d with identity planes" % (shape, storage, k))
        # the Python call is the raw call
        a = _coeffs(phi, m, 5, rng)
        ident, plane = _ident_planes(5)
        raw, got = _ok(g, a, ident, plane, d_sig), g.classify(a, ident, plane, d_sig, want=KEYS)
        assert sorted(got) == sorted(KEYS) and got["label"].dtype == torch.int32 and got["best"].dtype == got["margin"].dtype == torch.float32
        assert sorted(g.classify(a)) == ["label"]
        for key in KEYS:
            assert tuple(got[key].shape) == (SHAPES[shape][1], SHAPES[shape][0])
            _same(got[key], raw[key], "Graph.classify %s" % key)
        g.close()


@pytest.mark.parametrize("shape", ["ld64", "ld256"])
def test_compact_handle_is_its_f32_twin(shape):
    """The header's contract: on a compact handle the call returns what it returns on an f32 handle whose Phi is Q."""
    rng = np.random.default_rng(41)
    with glf.Context(0) as ctx:
        gc, gt, _, d_sig, _, _ = _pair(ctx, shape)
        phi = _phi64(gt)
        a = _coeffs(phi, gt.info["m"], 7, rng)
        ident, plane = _ident_planes(7)
        bias = rng.normal(size=7) * 0.1
        oc, ot = _ok(gc, a, ident, plane, d_sig, bias), _ok(gt, a, ident, plane, d_sig, bias)
        for key in KEYS:
            _same(oc[key], ot[key], "%s compact against its twin: %s" % (shape, key))
        gc.close()
        gt.close()


# ---- 2. ties and specials -------------------------------------------------------------------------------------------------------------

def _rule(scores):
    """(label, best, margin) [N] of f32 scores [k, N] by the rule text of include/glf.h, pixel by pixel."""
    k, n = scores.shape
    label, best, margin = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    ninf = np.float32(-np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for px in range(n):
            b, l = ninf, 0
            for j in range(k):
                if scores[j, px] > b:
                    b, l = scores[j, px], j
            s = ninf
            for j in range(k):
                if j != l and scores[j, px] > s:
                    s = scores[j, px]
            label[px], best[px], margin[px] = l, b, (np.float32(0.0) if s == b else np.float32(b - s))
    return label, best, margin


@pytest.mark.parametrize("storage", STORAGES)
def test_duplicated_classes_tie(storage):
    rng = np.random.default_rng(12)
    with glf.Context(0) as ctx:
        g, phi, _ = _handle(ctx, "ld64", storage)
        a = _coeffs(phi, g.info["m"], 8, rng)
        a[3], a[6] = a[1], a[2]                                                  # a pair within half-wave 0, and one across the halves
        out = _ok(g, a)
        label, margin = out["label"].cpu().numpy(), out["margin"].cpu().numpy()
        assert not np.isin(label, (3, 6)).any()
        pair = np.isin(label, (1, 2))
        print("duplicated classes win %d of %d pixels" % (int(pair.sum()), pair.size))
        assert (label == 1).any() and (label == 2).any()
        assert not _bits(margin[pair]).any()                                     # +0, the bit pattern
        assert np.all(margin[~pair] > 0)
        g.close()


@pytest.mark.parametrize("shape", ["tiny", "ld32"])
@pytest.mark.parametrize("k", [6, 32])
def test_specials_follow_the_rule(shape, k):
    """All-zero coefficients, identity factor 1: score_j = fmaf(1, plane_j, +0), the plane's value (-0 read as +0)."""
    w, h = SHAPES[shape][:2]
    n = w * h
    rng = np.random.default_rng(3 * k + n)
    planes = rng.integers(-2, 3, size=(k, n)).astype(np.float32)                  # small integers: exact ties everywhere
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
    hit = rng.random(planes.shape) < 0.25
    planes[hit] = specials[rng.integers(0, specials.size, int(hit.sum()))]
    planes[:, 0] = np.nan                                                        # an all-NaN pixel
    planes[:, 1] = np.nan
    planes[k - 1, 1] = -3.0                                                      # one finite score
    planes[:, 2] = -np.inf                                                       # nothing above -inf
    planes[:, 3] = -np.inf
    planes[4, 3] = 1.5                                                           # one score above -inf
    planes[:, 4] = 0.0
    planes[4, 4] = -0.0                                                          # zeros of both signs
    planes[:, 5] = -1.0
    planes[1, 5], planes[4, 5] = 2.0, 2.0                                        # a tie across the halves
    planes[:, 6] = np.inf                                                        # every class at +inf
    planes[:, n - 1] = planes[:, 5]                                              # ... and in the last, partial tile
    scores = planes + np.float32(0.0)                                            # x + (+0): -0 becomes +0, everything else itself
    want_label, want_best, want_margin = _rule(scores)
    assert want_label[0] == 0 and np.isneginf(want_best[0]) and want_label[1] == k - 1 and np.isposinf(want_margin[1])
    assert want_label[5] == 1 and want_margin[5] == 0 and want_label[6] == 0 and want_margin[6] == 0 and np.isposinf(want_margin[3])
    with glf.Context(0) as ctx:
        g, _, _ = _grey_graph(ctx, shape)
        d_planes = torch.from_numpy(planes.reshape(k, h, w)).to(ctx.device)
        out = _ok(g, np.zeros((k, g.info["m"])), np.ones(k, dtype=np.float32), np.arange(k, dtype=np.int32), d_planes)
        _same(out["label"].reshape(-1), want_label, "label")
        _same(out["best"].reshape(-1), want_best, "best")
        _same(out["margin"].reshape(-1), want_margin, "margin")
        assert not np.isnan(out["margin"].cpu().numpy()).any() and not np.isnan(out["best"].cpu().numpy()).any()
        g.close()


@pytest.mark.parametrize("storage", STORAGES)
def test_one_class(storage):
    rng = np.random.default_rng(1)
    with glf.Context(0) as ctx:
        g, phi, d_sig = _handle(ctx, "ld32", storage)
        a = _coeffs(phi, g.info["m"], 1, rng)
        for ident, plane, planes in ((None, None, None), (np.array([0.5], dtype=np.float32), np.array([2], dtype=np.int32), d_sig)):
            out = _ok(g, a, ident, plane, planes)
            assert not out["label"].any()
            _same(out["best"], g.synthesize(a, ident, plane, planes)[0], "best is y_0")
            assert bool(torch.all(out["margin"] == float("inf")))
        g.close()


# ---- 3. independence -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", STORAGES)
def test_independence(storage):
    rng = np.random.default_rng(23)
    with glf.Context(0) as ctx:
        g, phi, d_sig = _handle(ctx, "ld64", storage)
        m, k = g.info["m"], 5
        a = _coeffs(phi, m, k, rng)
        ident, plane = _ident_planes(k)
        y = g.synthesize(a, ident, plane, d_sig)
        assert not bool((y == 0).any())                                          # no signed zeros among the scores
        base = _ok(g, a, ident, plane, d_sig)
        # two calls, the same bits
        again = _ok(g, a, ident, plane, d_sig)
        for key in KEYS:
            _same(again[key], base[key], "second call: %s" % key)
        # exact zeros as the bias: the NULL call
        zero = _ok(g, a, ident, plane, d_sig, np.zeros(k))
        for key in KEYS:
            _same(zero[key], base[key], "zero bias: %s" % key)
        # label alone: the same bits, the other two buffers untouched
        alone = _ok(g, a, ident, plane, d_sig, want=("label",))
        _same(alone["label"], base["label"], "label alone")
        assert _untouched(alone, ("best", "margin"))
        only_margin = _ok(g, a, ident, plane, d_sig, want=("margin",))
        _same(only_margin["margin"], base["margin"], "margin alone")
        assert _untouched(only_margin, ("label", "best"))
        # a class that cannot win changes no label and no best, and no finite margin
        a6 = np.concatenate([a, _coeffs(phi, m, 1, rng)])
        more = _ok(g, a6, np.append(ident, np.float32(1.0)), np.append(plane, np.int32(1)), d_sig, np.array([0.0] * k + [-1e30]))
        _same(more["label"], base["label"], "appended class: label")
        _same(more["best"], base["best"], "appended class: best")
        finite = torch.isfinite(base["margin"])
        assert bool(finite.all())
        _same(more["margin"][finite], base["margin"][finite], "appended class: margin")
        # a permutation of the classes permutes the labels wherever the margin is positive
        perm = np.array([3, 0, 4, 1, 2])
        moved = _ok(g, a[perm], ident[perm], plane[perm], d_sig)                 # slot s holds class perm[s]
        clear = (base["margin"] > 0).cpu().numpy()
        assert clear.all()
        np.testing.assert_array_equal(perm[moved["label"].cpu().numpy()][clear], base["label"].cpu().numpy()[clear])
        _same(moved["best"], base["best"], "permuted classes: best")
        _same(moved["margin"], base["margin"], "permuted classes: margin")
        # the same bias on every class: fl(y + c) is monotone in y, so a label can move only where the rounding closes the gap
        c = 0.75
        top2 = torch.topk(y, 2, 0).values
        gap, room = (top2[0] - top2[1]).double(), 4.0 * U * (top2[0].abs().double() + c)
        print("smallest margin %.3e against %.3e of rounding room" % (float(gap.min()), float(room.max())))
        assert bool((gap > room).all())                                          # checked from y, not assumed
        shifted = _ok(g, a, ident, plane, d_sig, np.full(k, c))
        _same(shifted["label"], base["label"], "common bias: label")
        _same(shifted["best"], (y + np.float32(c)).max(0).values, "common bias: best is one f32 addition")
        g.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched():
    rng = np.random.default_rng(9)
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
        }
        last = lambda: glf._lib.glf_ctx_last_error(ctx._ctx).decode()
        for what, (kw, word) in cases.items():
            rc, out = _raw(g, **kw)
            assert rc == glf.ERR_INVALID, what
            assert "glf_graph_classify" in last() and word in last(), (what, last())
            assert _untouched(out), what
        rc, out = _raw(g, a)
        assert rc == glf.OK
        out2 = {key: out[key].clone() for key in KEYS}
        assert glf._lib.glf_graph_classify(None, C.c_int(k), glf._ptr(a), None, glf._ptr(plane), 0, None, None,
                                           *[C.c_void_p(out2[key].data_ptr()) for key in KEYS]) == glf.ERR_INVALID
        torch.cuda.synchronize()
        for key in KEYS:
            _same(out2[key], out[key], "a NULL handle writes nothing")
        # the Python layer
        with pytest.raises(ValueError, match="32"):
            g.classify(a33)
        with pytest.raises(ValueError):
            g.classify(np.zeros((2, m + 1)))
        with pytest.raises(ValueError):
            g.classify(a, want=("labels",))
        with pytest.raises(ValueError, match="32"):
            g.refine_logits(torch.zeros((33, h, w), dtype=torch.float32, device=ctx.device))
        seeds = torch.full((h, w), -1, dtype=torch.int32, device=ctx.device)
        seeds[3, 4], seeds[9, 30] = 0, 1
        with pytest.raises(ValueError, match="32"):
            g.propagate_labels(seeds, 33)
        with pytest.raises(ValueError, match="no seed"):
            g.propagate_labels(seeds, 3)
        seeds[5, 5] = 2
        with pytest.raises(ValueError):
            g.propagate_labels(seeds, 2)                                         # a seed value of k
        seeds[5, 5] = -2
        with pytest.raises(ValueError):
            g.propagate_labels(seeds, 2)
        # nothing faulted, and the next valid call succeeds
        _against_synthesize(g, a, ident, plane, d_sig, "after the refusals")
        g.close()


# ---- 5. the drivers against f64 on the handle's own Phi ------------------------------------------------------------------------------

def _top2_64(s):
    """(lowest-index argmax, margin) of f64 scores [k, N]."""
    label = (s == s.max(axis=0)).argmax(axis=0)
    srt = np.sort(s, axis=0)
    return label, srt[-1] - srt[-2]


def _compare_with_f64(what, label, s64, err, skip=None):
    """The module text's rule; -> (share left out, the mask of compared pixels)."""
    label64, margin64 = _top2_64(s64)
    decided = margin64 > 2.0 * err.max(axis=0)
    left_out = 1.0 - float(decided.mean())
    wrong = int(np.count_nonzero((label != label64) & decided))
    print("%s: %.3f %% of the pixels left out (margin64 <= 2 max err), smallest compared margin %.3e, largest err %.3e, %d labels differ" %
          (what, 100.0 * left_out, float(margin64[decided].min()), float(err.max()), wrong))
    assert left_out <= 0.01, (what, left_out)
    assert wrong == 0, (what, wrong)
    return left_out, label64


def _halves(w, h):
    return np.tile((np.arange(w) >= w // 2).astype(np.int64), h)


def test_propagate_labels_against_f64():
    w, h = SHAPES["ld32"][:2]
    n, k, ridge = w * h, 2, 1e-3
    with glf.Context(0) as ctx:
        g = ctx.graph(ctx.to_device(_two_tone(TWO_TONE_SEED)), _opt("ld32"))
        m, ld = g.info["m"], g.info["ld"]
        assert (m, ld) == (8, 32)
        phi, lam = _phi64(g), g.eigenvalues
        seeds = np.full((h, w), -1, dtype=np.int32)                              # two short scribbles per half, 20 pixels
        seeds[10, 5:10], seeds[35, 15:20] = 0, 0
        seeds[12, 40:45], seeds[30, 50:55] = 1, 1
        assert int((seeds >= 0).sum()) == 20
        out = g.propagate_labels(torch.from_numpy(seeds).to(ctx.device), k, ridge=ridge, want=KEYS)
        a = out["coeffs"]
        assert a.shape == (k, m) and out["label"].dtype == torch.int32 and tuple(out["label"].shape) == (h, w)
        label = out["label"].cpu().numpy().reshape(-1)
        # the read-out is synthesize's, bit for bit
        y = g.synthesize(a)
        _same(out["label"], _lowest_argmax(y), "propagate_labels: label")
        _same(out["best"], y.max(0).values, "propagate_labels: best")
        samples = g.samples().astype(np.int64)
        g.close()
    # f64: weighted normal equations, solve, Phi a, lowest-index argmax
    sd = seeds.reshape(-1)
    wgt = (sd >= 0).astype(np.float64)
    onehot = np.stack([(sd == j).astype(np.float64) for j in range(k)])
    G64 = phi.T @ (wgt[:, None] * phi)
    b64 = (onehot * wgt) @ phi
    pen = (ridge + 0.0 * lam) * (np.trace(G64) / m)
    a64 = np.linalg.solve(G64 + np.diag(pen), b64.T).T
    s64 = a64 @ phi.T
    err = (ld + 4) * U * (np.abs(a) @ np.abs(phi).T) + np.abs(a - a64) @ np.abs(phi).T
    print("propagate_labels: max |a - a64| / max |a64| %.3e" % (float(np.abs(a - a64).max()) / float(np.abs(a64).max())))
    left_out, label64 = _compare_with_f64("propagate_labels", label, s64, err)
    outside = np.ones(n, dtype=bool)
    outside[samples] = False
    halves = _halves(w, h)
    agree, agree64 = float((label == halves)[outside].mean()), float((label64 == halves)[outside].mean())
    print("propagate_labels: agreement with the two halves outside the sample pixels %.4f (f64 %.4f)" % (agree, agree64))
    assert abs(agree - agree64) <= left_out + 1e-12


def test_refine_logits_against_f64_and_apply():
    w, h = SHAPES["ld32"][:2]
    n, k = w * h, 3
    rng = np.random.default_rng(77)
    halves = _halves(w, h)
    logits = 0.5 * rng.normal(size=(k, n))
    logits[0] += halves == 0
    logits[1] += halves == 1                                                     # the third class is pure noise
    logits = logits.astype(np.float32)
    with glf.Context(0) as ctx:
        g = ctx.graph(ctx.to_device(_two_tone(TWO_TONE_SEED)), _opt("ld32"))
        m, ld = g.info["m"], g.info["ld"]
        phi, lam = _phi64(g), g.eigenvalues
        d_logits = torch.from_numpy(logits.reshape(k, h, w)).to(ctx.device)
        out = g.refine_logits(d_logits, want=KEYS)
        label = out["label"].cpu().numpy().reshape(-1)
        # Graph.apply on the wide route and the lowest-index argmax: the same coefficients, the same arithmetic, the same bits
        z = g.apply(d_logits, (1.0 - lam)[None], ident=1.0, wide=True)[0]
        _same(out["label"], _lowest_argmax(z), "refine_logits against apply: label")
        top2 = torch.topk(z, 2, 0).values
        _same(out["best"], top2[0], "refine_logits against apply: best")
        _same(out["margin"], top2[0] - top2[1], "refine_logits against apply: margin")
        assert sorted(g.refine_logits(d_logits)) == ["label", "margin"]
        a = (1.0 - lam)[None, :] * g.project_wide(d_logits)                      # the library's coefficients
        samples = g.samples().astype(np.int64)
        g.close()
    l64 = logits.astype(np.float64)
    a64 = (1.0 - lam)[None, :] * (l64 @ phi)
    s64 = l64 + a64 @ phi.T
    err = (ld + 4) * U * (np.abs(l64) + np.abs(a) @ np.abs(phi).T) + np.abs(a - a64) @ np.abs(phi).T
    left_out, label64 = _compare_with_f64("refine_logits", label, s64, err)
    outside = np.ones(n, dtype=bool)
    outside[samples] = False
    agree, agree64 = float((label == halves)[outside].mean()), float((label64 == halves)[outside].mean())
    raw = float((logits.argmax(axis=0) == halves)[outside].mean())
    print("refine_logits: agreement with the two halves outside the sample pixels %.4f (f64 %.4f; the raw logits' argmax %.4f)" % (agree, agree64, raw))
    assert abs(agree - agree64) <= left_out + 1e-12


# ---- 6. the tile loop ----------------------------------------------------------------------------------------------------------------

def test_tile_loop():
    """509 x 515 = 8192 tiles: more than the resident waves take at once, so every wave runs its tile loop more than once -- the
    prefetch under the MFMAs, fresh accumulators and a fresh top two per tile. Test 1 at k = 32 with identity planes, ld 64."""
    w, h, m, ld, k = 509, 515, 40, 64, 32
    n = w * h
    rng = np.random.default_rng(64)
    with glf.Context(0) as ctx:
        assert (n + 31) // 32 > 4 * 7 * ctx.device_info()["num_cus"]
        g = ctx.graph(ctx.to_device(glf.synth_image(w, h, seed=3)), glf.default_options(num_samples=300, num_eigvals=m, epsilon=0.1))
        assert (g.info["m"], g.info["ld"]) == (m, ld)
        a = _coeffs(np.array([float(g.phi[:, :m].abs().max())]), m, k, rng)
        planes = torch.from_numpy(rng.normal(size=(3, h, w)).astype(np.float32)).to(ctx.device)
        ident, plane = _ident_planes(k)
        out = _against_synthesize(g, a, ident, plane, planes, "509 x 515 k 32")
        counts = np.bincount(out["label"].cpu().numpy().reshape(-1), minlength=k)
        print("509 x 515: classes that win somewhere %d of %d" % (int((counts > 0).sum()), k))
        g.close()
