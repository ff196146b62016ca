"""Blend read-out on a graph handle (glf_graph_blend / Graph.blend, .apply_local, .gather, .fit_piecewise): a bank of nout * nlevels
<= 32 score planes ident_s s + Phi a_s, slot s = o nlevels + b, formed in registers in one pass over Phi (k_graph_blend:
k_graph_classify up to its scores) and read out per pixel by a level map -- the plane of an integer level, the pinned linear blend of
the two neighbouring planes between two levels -- and never written.

Shapes: those of tests/test_gpu_graph.py -- 61 x 47 = 2867 pixels (89 whole tiles and one of 19 pixels) at ld 32 / 64 / 128 / 256,
and `tiny` (160 pixels), both storages; 509 x 515 in one test, so that waves run their tile loop more than once. Every raw call
writes into buffers pre-filled with a sentinel, so that "untouched" and "every pixel written" are both asserted.

The scores have glf_graph_synthesize's bits, so tests 1, 2 and 4 compare with the handle's own synthesize of the same nout * nlevels
coefficient rows, bit for bit: at integer levels the matching plane itself, elsewhere tests/blend_ref.py's emulation of the epilogue
applied to those planes (tests/test_blend_ref.py checks that emulation against a restatement in rationals, and that the comparison
rejects seeded defects). Test 3 compares with f64 on the handle's own Phi under the bound of include/glf.h ("Blend
read-out"): the same f32 level gives the same i and f exactly, so with u = 2^-24 and e_s = (ld + 4) u (|ident_s s| + |Phi| |a_s|),
  |out - out*| <= (1 - f) e_lo + f e_hi + 2 u (1 + u) ((1 - f) (|z*_lo| + e_lo) + f (|z*_hi| + e_hi)).

tests/test_blend_ref.py names no symbol of the library and passes with or without the feature; this file and
tests/test_graph_blend_abi.py fail without it."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import blend_ref as br  # noqa: E402
import glf  # noqa: E402
from test_gpu_graph import SHAPES, _opt, _phi64  # noqa: E402
from test_gpu_graph_classify import _coeffs, _handle, _ident_planes  # noqa: E402
from test_gpu_graph_cluster import TWO_TONE_SEED, _two_tone  # noqa: E402
from test_gpu_graph_compact import LD_SHAPES, _pair  # noqa: E402

U = 2.0 ** -24
ALL_SHAPES = LD_SHAPES + ["tiny"]
STORAGES = ["f32", "compact"]
CASES = [(1, 2), (1, 32), (4, 8), (16, 2), (3, 10)]
SENTINEL = -77.0


def _raw(g, a, level, nout, nlevels, ident=None, plane=None, planes=None, nplanes=None, null=()):
    """glf_graph_blend itself on a sentinel-filled buffer -> (status, the buffer [max(nout, 1), H, W]). a: [nout * nlevels, m] or None;
    null: which of "level", "out", "plane" are passed as NULL."""
    a = None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, np.shape(a)[-1]))
    h, w = g.info["height"], g.info["width"]
    slots = min(max(nout * nlevels, 1), 64)                                      # (a refused call reads no entry)
    out = torch.full((max(min(nout, 32), 1), h, w), SENTINEL, dtype=torch.float32, device=g.ctx.device)
    pl = np.full(slots, -1, dtype=np.int32) if plane is None else np.ascontiguousarray(plane, dtype=np.int32)
    idn = None if ident is None else np.ascontiguousarray(ident, dtype=np.float32)
    if nplanes is None:
        nplanes = 0 if planes is None else planes.shape[0]
    torch.cuda.synchronize()
    rc = glf._lib.glf_graph_blend(g._g, C.c_int(nout), C.c_int(nlevels), glf._ptr(a), glf._ptr(idn), None if "plane" in null else glf._ptr(pl),
                                  C.c_int(nplanes), C.c_void_p(planes.data_ptr()) if planes is not None else None,
                                  None if "level" in null else C.c_void_p(level.data_ptr()), None if "out" in null else C.c_void_p(out.data_ptr()))
    torch.cuda.synchronize()
    return rc, out


def _ok(g, *args, **kw):
    rc, out = _raw(g, *args, **kw)
    assert rc == glf.OK, (rc, glf._lib.glf_ctx_last_error(g.ctx._ctx).decode())
    assert not bool((out == SENTINEL).any())                                     # every pixel of every output was written
    return out


def _same(a, b, what):
    """Bit for bit, for two float32 tensors / arrays of one shape."""
    a = torch.as_tensor(a).detach().cpu().contiguous()
    b = torch.as_tensor(b).detach().cpu().contiguous()
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    bad = int((a.view(torch.int32) != b.view(torch.int32)).sum())
    assert bad == 0, "%s: %d of %d elements differ in bits" % (what, bad, a.numel())


def _dev_level(g, level):
    return torch.from_numpy(np.ascontiguousarray(level, dtype=np.float32).reshape(g.info["height"], g.info["width"])).to(g.ctx.device)


def _bank(g, phi, nout, nlevels, rng, with_planes):
    """(a [slots, m], ident, plane): a bank at the scale that makes the scores of order one; the identity terms of the classify tests
    (factors from {1, -0.5, 0.25}, the three test planes, one slot without a plane) or none."""
    slots = nout * nlevels
    a = _coeffs(phi, g.info["m"], slots, rng)
    ident, plane = _ident_planes(slots) if with_planes else (None, None)
    return a, ident, plane


# ---- 1. integer levels: the matching plane of synthesize, bit for bit ---------------------------------------------------------------

@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_integer_levels_are_synthesize(shape, storage):
    rng = np.random.default_rng(300 + SHAPES[shape][5])
    with glf.Context(0) as ctx:
        g, phi, d_sig = _handle(ctx, shape, storage)
        h, w = g.info["height"], g.info["width"]
        for nout, nlevels in CASES:
            for with_planes in (False, True):
                what = "%s %s (%d, %d)%s" % (shape, storage, nout, nlevels, " planes" if with_planes else "")
                a, ident, plane = _bank(g, phi, nout, nlevels, rng, with_planes)
                planes = d_sig if with_planes else None
                y = g.synthesize(a, ident, plane, planes).view(nout, nlevels, h, w)
                assert bool(torch.isfinite(y).all())
                for b in range(nlevels):
                    out = _ok(g, a, torch.full((h, w), float(b), dtype=torch.float32, device=ctx.device), nout, nlevels, ident, plane, planes)
                    _same(out, y[:, b], "%s constant level %d" % (what, b))
                idx = rng.integers(0, nlevels, size=(h, w))
                idx[0, 0], idx[-1, -1] = nlevels - 1, 0                          # both ends of the bank, whatever the draw
                idx = torch.from_numpy(idx).to(ctx.device)
                out = _ok(g, a, idx.to(torch.float32), nout, nlevels, ident, plane, planes)
                _same(out, torch.gather(y, 1, idx[None, None].expand(nout, 1, h, w))[:, 0], what + " random integer map")
        # the Python call is the raw call
        a, ident, plane = _bank(g, phi, 4, 8, rng, True)
        level = _dev_level(g, br.special_levels(8, h * w, rng))
        raw = _ok(g, a, level, 4, 8, ident, plane, d_sig)
        got = g.blend(a.reshape(4, 8, -1), level, ident.reshape(4, 8), plane.reshape(4, 8), d_sig)
        assert got.dtype == torch.float32 and tuple(got.shape) == (4, h, w)
        _same(got, raw, "Graph.blend")
        one = g.blend(a[:8], level)
        assert tuple(one.shape) == (1, h, w)
        _same(one, _ok(g, a[:8], level, 1, 8), "Graph.blend, one output from [nlevels, m]")
        g.close()


# ---- 2. fractional levels: blend_ref on synthesize's planes, bit for bit ------------------------------------------------------------

def _against_ref(g, a, ident, plane, planes, level, nout, nlevels, what):
    y = g.synthesize(a, ident, plane, planes).reshape(nout * nlevels, -1).cpu().numpy()
    assert np.isfinite(y).all()
    out = _ok(g, a, _dev_level(g, level), nout, nlevels, ident, plane, planes)
    want = br.emulate(y, level, nout, nlevels)[0]
    _same(out.reshape(nout, -1), want, what)
    return out


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_fractional_levels_are_the_pinned_lerp(shape, storage):
    rng = np.random.default_rng(400 + SHAPES[shape][5])
    with glf.Context(0) as ctx:
        g, phi, d_sig = _handle(ctx, shape, storage)
        n = g.info["height"] * g.info["width"]
        for nout, nlevels in CASES:
            level = br.special_levels(nlevels, n, rng)
            for with_planes in (False, True):
                a, ident, plane = _bank(g, phi, nout, nlevels, rng, with_planes)
                _against_ref(g, a, ident, plane, d_sig if with_planes else None, level, nout, nlevels,
                             "%s %s (%d, %d)%s" % (shape, storage, nout, nlevels, " planes" if with_planes else ""))
        g.close()


def test_tile_loop():
    """509 x 515 = 8192 tiles: every wave runs its tile loop more than once -- the level loaded per tile, the prefetch under the
    MFMAs, the wave's image reused for the transposed scores and then for the next tile. Test 2 at (4, 8) with identity planes, ld 64."""
    w, h, m, ld, nout, nlevels = 509, 515, 40, 64, 4, 8
    rng = np.random.default_rng(75)
    with glf.Context(0) as ctx:
        assert (w * h + 31) // 32 > 4 * 7 * ctx.device_info()["num_cus"]
        g = ctx.graph(ctx.to_device(glf.synth_image(w, h, seed=3)), glf.default_options(num_samples=300, num_eigvals=m, epsilon=0.1))
        assert (g.info["m"], g.info["ld"]) == (m, ld)
        a = _coeffs(np.array([float(g.phi[:, :m].abs().max())]), m, nout * nlevels, rng)
        planes = torch.from_numpy(rng.normal(size=(3, h, w)).astype(np.float32)).to(ctx.device)
        ident, plane = _ident_planes(nout * nlevels)
        _against_ref(g, a, ident, plane, planes, br.special_levels(nlevels, w * h, rng), nout, nlevels, "509 x 515 (4, 8) planes")
        g.close()


# ---- 3. against fp64 on the handle's own Phi, every pixel ---------------------------------------------------------------------------

@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_against_f64_every_pixel(shape, storage):
    rng = np.random.default_rng(500 + SHAPES[shape][5])
    worst = 0.0
    with glf.Context(0) as ctx:
        g, phi, d_sig = _handle(ctx, shape, storage)
        ld, n = g.info["ld"], g.info["height"] * g.info["width"]
        s = d_sig.reshape(3, -1).cpu().numpy().astype(np.float64)
        for nout, nlevels in CASES:
            a, ident, plane = _bank(g, phi, nout, nlevels, rng, True)
            level = br.special_levels(nlevels, n, rng)
            out = _ok(g, a, _dev_level(g, level), nout, nlevels, ident, plane, d_sig).reshape(nout, n).cpu().numpy().astype(np.float64)
            idt = np.where(plane[:, None] >= 0, ident.astype(np.float64)[:, None] * s[np.maximum(plane, 0)], 0.0)     # [slots, N]
            z = idt + a @ phi.T
            e = (ld + 4) * U * (np.abs(idt) + np.abs(a) @ np.abs(phi).T)
            i, f = br.index_rule(level, nlevels)
            f = f.astype(np.float64)
            px = np.arange(n)
            for o in range(nout):
                lo = o * nlevels + i
                z_lo, z_hi, e_lo, e_hi = z[lo, px], z[lo + 1, px], e[lo, px], e[lo + 1, px]
                want = (1 - f) * z_lo + f * z_hi
                bound = (1 - f) * e_lo + f * e_hi + 2 * U * (1 + U) * ((1 - f) * (np.abs(z_lo) + e_lo) + f * (np.abs(z_hi) + e_hi))
                frac = float((np.abs(out[o] - want) / bound).max())
                worst = max(worst, frac)
                assert frac <= 1.0, ("%s %s (%d, %d) output %d" % (shape, storage, nout, nlevels, o), frac)
        g.close()
    print("blend against f64, %s %s (ld %d): largest error / bound %.3f" % (shape, storage, SHAPES[shape][5], worst))


# ---- 4. independence -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", STORAGES)
def test_independence(storage):
    rng = np.random.default_rng(58)
    with glf.Context(0) as ctx:
        g, phi, d_sig = _handle(ctx, "ld64", storage)
        h, w, m = g.info["height"], g.info["width"], g.info["m"]
        n = h * w
        nout, nlevels = 4, 8
        a, ident, plane = _bank(g, phi, nout, nlevels, rng, True)
        lev = br.special_levels(nlevels, n, rng)
        level = _dev_level(g, lev)
        base = _ok(g, a, level, nout, nlevels, ident, plane, d_sig)
        _same(_ok(g, a, level, nout, nlevels, ident, plane, d_sig), base, "second call")
        # an output's plane depends neither on nout nor on the outputs beside it (nor on its slots)
        rows = lambda outs: np.concatenate([np.arange(o * nlevels, (o + 1) * nlevels) for o in outs])
        for outs in ([0], [3], [2, 0], [3, 1, 2]):
            r = rows(outs)
            part = _ok(g, a[r], level, len(outs), nlevels, ident[r], plane[r], d_sig)
            for k, o in enumerate(outs):
                _same(part[k], base[o], "output %d alone / among %s" % (o, outs))
        # levels appended above the map's maximum change no bit (the top level is then read with f = 0 instead of f = 1)
        inside = np.clip(np.where(np.isnan(lev), 0.0, lev), -1.0, float(nlevels - 1)).astype(np.float32)
        assert inside.max() == nlevels - 1
        d_inside = _dev_level(g, inside)
        two = rows([1, 2])
        short = _ok(g, a[two], d_inside, 2, nlevels, ident[two], plane[two], d_sig)
        extra, ei, ep = _bank(g, phi, 2, 3, rng, True)
        longer = lambda x, ex: np.concatenate([x[two][:nlevels], ex[:3], x[two][nlevels:], ex[3:]])
        _same(_ok(g, longer(a, extra), d_inside, 2, nlevels + 3, longer(ident, ei), longer(plane, ep), d_sig), short, "three levels appended")
        # a slot that overflows reaches no pixel that does not take it with a weight other than zero
        j = 3
        big_a, big_i, big_p = a[:nlevels].copy(), ident[:nlevels].copy(), plane[:nlevels].copy()
        big_a[j], big_i[j], big_p[j] = 1e30, 1e37, 2                            # plane 2 is >= 900 everywhere: the score is 1e37 * 900 + ..
        assert not bool(torch.isfinite(g.synthesize(big_a, big_i, big_p, d_sig)[j]).any())
        clean = _ok(g, a[:nlevels], level, 1, nlevels, ident[:nlevels], plane[:nlevels], d_sig)[0].reshape(-1).cpu().numpy()
        dirty = _ok(g, big_a, level, 1, nlevels, big_i, big_p, d_sig)[0].reshape(-1).cpu().numpy()
        tc = np.clip(np.where(np.isnan(lev), 0.0, lev), 0.0, nlevels - 1.0)
        near = (tc > j - 1) & (tc < j + 1)
        assert near.any() and (tc == j - 1).any() and (tc == j + 1).any()
        assert np.array_equal(clean[~near].view(np.uint32), dirty[~near].view(np.uint32))
        assert not np.isfinite(dirty[near]).any() and np.isfinite(clean).all()
        # out= is written in place
        buf = torch.full((nout, h, w), SENTINEL, dtype=torch.float32, device=ctx.device)
        got = g.blend(a.reshape(nout, nlevels, m), level, ident.reshape(nout, nlevels), plane.reshape(nout, nlevels), d_sig, out=buf)
        assert got.data_ptr() == buf.data_ptr()
        _same(buf, base, "out=")
        # more outputs than 32 // nlevels: groups, and no output depends on its group
        many = np.concatenate([a, a[rows([2, 0, 1])]]).reshape(7, nlevels, m)
        mi, mp = np.concatenate([ident, ident[rows([2, 0, 1])]]).reshape(7, nlevels), np.concatenate([plane, plane[rows([2, 0, 1])]]).reshape(7, nlevels)
        grouped = g.blend(many, level, mi, mp, d_sig)
        _same(grouped[:4], base, "seven outputs: the first group")
        _same(grouped[4:], base[[2, 0, 1]], "seven outputs: the second group")
        g.close()


@pytest.mark.parametrize("variant", ["plain", "scaled"])
@pytest.mark.parametrize("shape", ["ld64", "ld256"])
def test_compact_handle_is_its_f32_twin(shape, variant):
    rng = np.random.default_rng(44)
    with glf.Context(0) as ctx:
        gc, gt, _, d_sig, _, _ = _pair(ctx, shape, variant)
        nout, nlevels = 4, 8
        a, ident, plane = _bank(gt, _phi64(gt), nout, nlevels, rng, True)
        level = _dev_level(gt, br.special_levels(nlevels, gt.info["height"] * gt.info["width"], rng))
        oc, ot = _ok(gc, a, level, nout, nlevels, ident, plane, d_sig), _ok(gt, a, level, nout, nlevels, ident, plane, d_sig)
        assert bool(torch.isfinite(ot).all())
        _same(oc, ot, "%s %s compact against its twin" % (shape, variant))
        gc.close()
        gt.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_output_untouched():
    rng = np.random.default_rng(11)
    with glf.Context(0) as ctx:
        g, phi, d_sig = _handle(ctx, "ld64", "f32")
        h, w, m = g.info["height"], g.info["width"], g.info["m"]
        nout, nlevels = 2, 3
        a = _coeffs(phi, m, 6, rng)
        ident, plane = np.ones(6, dtype=np.float32), np.array([0, 1, 2, -1, 0, 1], dtype=np.int32)
        level = torch.zeros((h, w), dtype=torch.float32, device=ctx.device)
        bad_plane, low_plane, huge = plane.copy(), plane.copy(), a.copy()
        bad_plane[2] = 3                                                         # = nplanes
        low_plane[4] = -2
        huge[1, 3] = 1e60                                                        # finite in f64, not in f32
        a33 = _coeffs(phi, m, 33, rng)
        cases = {
            "nout = 0": (dict(a=a, nout=0, nlevels=3), "nout = 0"), "nout = -1": (dict(a=a, nout=-1, nlevels=3), "nout = -1"),
            "nlevels = 1": (dict(a=a, nout=2, nlevels=1), "nlevels = 1"), "nlevels = 0": (dict(a=a, nout=2, nlevels=0), "nlevels = 0"),
            "33 slots": (dict(a=a33, nout=3, nlevels=11), "nout * nlevels"), "1 x 33": (dict(a=a33, nout=1, nlevels=33), "nlevels = 33"),
            "an int overflow": (dict(a=a, nout=2 ** 16, nlevels=2 ** 16), "nout * nlevels"),
            "h_a NULL": (dict(a=None, nout=2, nlevels=3), "h_a"), "plane NULL": (dict(a=a, nout=2, nlevels=3, null=("plane",)), "plane"),
            "nplanes < 0": (dict(a=a, nout=2, nlevels=3, nplanes=-1), "nplanes"),
            "plane[s] = nplanes": (dict(a=a, nout=2, nlevels=3, ident=ident, plane=bad_plane, planes=d_sig), "plane[2]"),
            "plane[s] = -2": (dict(a=a, nout=2, nlevels=3, ident=ident, plane=low_plane, planes=d_sig), "plane[4]"),
            "planes without d_planes": (dict(a=a, nout=2, nlevels=3, ident=ident, plane=plane, planes=None, nplanes=3), "identity"),
            "planes without ident": (dict(a=a, nout=2, nlevels=3, ident=None, plane=plane, planes=d_sig), "identity"),
            "a coefficient beyond f32": (dict(a=huge, nout=2, nlevels=3), "coefficient"),
            "a NaN coefficient": (dict(a=np.where(np.arange(m) == 1, np.nan, a), nout=2, nlevels=3), "coefficient"),
            "d_level NULL": (dict(a=a, nout=2, nlevels=3, null=("level",)), "d_level"),
        }
        last = lambda: glf._lib.glf_ctx_last_error(ctx._ctx).decode()
        for what, (kw, word) in cases.items():
            rc, out = _raw(g, level=level, **kw)
            assert rc == glf.ERR_INVALID, what
            assert "glf_graph_blend" in last() and word in last(), (what, last())
            assert bool((out == SENTINEL).all()), what
        rc, _ = _raw(g, a, level, 2, 3, null=("out",))
        assert rc == glf.ERR_INVALID and "glf_graph_blend" in last() and "d_out" in last()
        out = _ok(g, a, level, 2, 3)
        out2 = out.clone()
        assert glf._lib.glf_graph_blend(None, C.c_int(2), C.c_int(3), glf._ptr(a), None, glf._ptr(plane), 0, None, C.c_void_p(level.data_ptr()),
                                        C.c_void_p(out2.data_ptr())) == glf.ERR_INVALID
        torch.cuda.synchronize()
        _same(out2, out, "a NULL handle writes nothing")
        # the Python layer
        with pytest.raises(ValueError, match="32"):
            g.blend(np.zeros((1, 33, m)), level)
        with pytest.raises(ValueError):
            g.blend(np.zeros((1, m)), level)                                     # one level
        with pytest.raises(ValueError):
            g.blend(np.zeros((2, 3, m + 1)), level)
        with pytest.raises(ValueError):
            g.blend(np.zeros((2, 3, m)), level[:-1])
        with pytest.raises(ValueError):
            g.blend(np.zeros((2, 3, m)), level, ident=np.ones((2, 4)))
        with pytest.raises(ValueError):
            g.blend(np.zeros((2, 3, m)), level, out=torch.zeros((3, h, w), dtype=torch.float32, device=ctx.device))
        with pytest.raises(glf.GlfError):
            g.blend(np.zeros((2, 3, m)), level, ident=1.0, plane=0)              # identity terms without planes
        with pytest.raises(ValueError, match="32"):
            g.apply_local(d_sig, level, np.ones((33, m)))
        with pytest.raises(ValueError):
            g.apply_local(d_sig, level, np.ones((1, m)))
        labels = torch.zeros((h, w), dtype=torch.int32, device=ctx.device)
        with pytest.raises(ValueError, match="32"):
            g.gather(np.zeros((33, m)), labels)
        with pytest.raises(ValueError):
            g.gather(np.zeros((1, m)), labels)
        with pytest.raises(ValueError):
            g.fit_piecewise(d_sig, labels, 1)
        with pytest.raises(ValueError, match="32"):
            g.fit_piecewise(d_sig, labels, 33)
        # nothing faulted, and the next valid call succeeds
        _against_ref(g, a, ident, plane, d_sig, br.special_levels(3, h * w, rng), 2, 3, "after the refusals")
        g.close()


# ---- 6. the drivers ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", STORAGES)
def test_apply_local_is_its_chained_calls_and_apply_at_integer_levels(storage):
    rng = np.random.default_rng(59)
    with glf.Context(0) as ctx:
        g, phi, d_sig = _handle(ctx, "ld64", storage)
        h, w, m = g.info["height"], g.info["width"], g.info["m"]
        lam = g.eigenvalues
        B = 5
        weights = np.exp(-np.array([0.0, 0.5, 2.0, 8.0, 32.0])[:, None] * lam[None, :])
        ident = np.array([1.0, 0.5, 0.25, 0.0, -0.5], dtype=np.float32)
        level = _dev_level(g, br.special_levels(B, h * w, rng))
        got = g.apply_local(d_sig, level, weights, ident)
        assert tuple(got.shape) == (3, h, w) and got.dtype == torch.float32
        c = g.project_wide(d_sig)
        chained = g.blend(weights[None, :, :] * c[:, None, :], level, ident[None, :], np.arange(3, dtype=np.int32)[:, None], d_sig)
        _same(got, chained, "apply_local against project_wide, the host scaling and blend")
        whole = g.apply(d_sig, weights, ident, wide=True)                        # [B, 3, H, W]
        for b in range(B):
            flat = g.apply_local(d_sig, torch.full((h, w), float(b), dtype=torch.float32, device=ctx.device), weights, ident)
            _same(flat, whole[b], "apply_local at the constant level %d against apply" % b)
        # a float ident, and more planes than 32 // B: groups of planes
        seven = torch.cat([d_sig, d_sig.flip(0), d_sig[:1]])
        wide = g.apply_local(seven, level, weights)
        one = g.apply_local(d_sig, level, weights, 1.0)
        _same(wide[:3], one, "seven planes: the first three")
        _same(wide[3:6], one.flip(0), "seven planes: the next three")
        _same(wide[6], one[0], "seven planes: the last")
        g.close()


def test_apply_local_smooths_where_the_level_says():
    """The two-tone image as the plane, a bank whose level 0 is the input itself (weights 0, ident 1) and whose other levels smooth
    (ident 0, the projection damped by (1 - lam)^q on the basis made orthonormal), level 0 on the left half and B - 1 on the right: the
    left half comes back exactly, the right half is apply's top response, and its sample variance over the flat right half is below
    the input's."""
    w, h = SHAPES["ld32"][:2]
    with glf.Context(0) as ctx:
        img = _two_tone(TWO_TONE_SEED)
        g = ctx.graph(ctx.to_device(img), _opt("ld32"))
        g.orthonormalize("ritz")
        lam = g.eigenvalues
        plane = torch.from_numpy(img.astype(np.float32)[None]).to(ctx.device)
        assert not bool(torch.signbit(plane).any())                              # no -0: fmaf(1, s, +0) is s
        powers = np.array([0.0, 1.0, 2.0, 4.0])
        weights = (1.0 - lam)[None, :] ** powers[:, None]
        weights[0] = 0.0
        ident = np.array([1.0, 0.0, 0.0, 0.0], dtype=np.float32)
        B = weights.shape[0]
        left = torch.arange(w, device=ctx.device) < w // 2
        level = torch.where(left, 0.0, float(B - 1))[None, :].expand(h, w).contiguous().to(torch.float32)
        out = g.apply_local(plane, level, weights, ident)[0]
        _same(out[:, :w // 2], plane[0][:, :w // 2], "level 0 under weights 0 and ident 1: the input plane")
        top = g.apply(plane, weights, ident, wide=True)[B - 1, 0]
        _same(out[:, w // 2:], top[:, w // 2:], "level B - 1: apply's response B - 1")
        var_in, var_out = float(plane[0][:, w // 2:].double().var()), float(out[:, w // 2:].double().var())
        print("apply_local on the two-tone image: sample variance over the right half %.3f in, %.3e out (its mean %.2f in, %.3f out)" %
              (var_in, var_out, float(plane[0][:, w // 2:].double().mean()), float(out[:, w // 2:].double().mean())))
        assert var_out < var_in
        g.close()


def test_gather_is_synthesize_gathered():
    rng = np.random.default_rng(60)
    with glf.Context(0) as ctx:
        g, phi, _ = _handle(ctx, "ld64", "f32")
        h, w, m = g.info["height"], g.info["width"], g.info["m"]
        for k in (2, 5, 32):
            labels = g.segment(k, seed=3, max_iter=5)[0]
            a = _coeffs(phi, m, k, rng)
            y = g.synthesize(a)
            want = torch.gather(y, 0, labels.long()[None])[0]
            got = g.gather(a, labels)
            assert tuple(got.shape) == (h, w)
            _same(got, want, "gather, k = %d" % k)
        g.close()


def test_fit_piecewise_is_its_chained_calls():
    """On the two-tone image with the two halves as labels: the driver equals normal_equations under the weight (labels == j),
    fit_coeffs and gather, bit for bit; a label without pixels keeps zero coefficients. The RMS error against the noiseless tones is
    printed next to Graph.fit's (measured, not asserted: the handle's basis is not orthonormal)."""
    w, h = SHAPES["ld32"][:2]
    with glf.Context(0) as ctx:
        img = _two_tone(TWO_TONE_SEED)
        g = ctx.graph(ctx.to_device(img), _opt("ld32"))
        m = g.info["m"]
        assert m == 8
        plane = torch.from_numpy(img.astype(np.float32)[None]).to(ctx.device)
        cols = torch.arange(w, device=ctx.device)
        labels = (cols >= w // 2).to(torch.int32)[None, :].expand(h, w).contiguous()
        wgt = torch.from_numpy(np.random.default_rng(61).uniform(0.5, 2.0, size=(h, w)).astype(np.float32)).to(ctx.device)
        for weight, smooth, ridge in ((None, 0.0, 0.0), (wgt, 0.5, 1e-3)):
            out, a = g.fit_piecewise(plane, labels, 2, weight, smooth, ridge)
            assert tuple(out.shape) == (1, h, w) and a.shape == (1, 2, m)
            want_a = np.zeros_like(a)
            for j in range(2):
                wj = (labels == j).to(torch.float32) * (1.0 if weight is None else weight)
                G, b = g.normal_equations(wj, plane)
                want_a[:, j] = glf.fit_coeffs(G, b, (ridge + smooth * g.eigenvalues) * (np.trace(G) / m))
            np.testing.assert_array_equal(a, want_a)
            _same(out[0], g.gather(want_a[0], labels), "fit_piecewise against its chained calls")
        out, a = g.fit_piecewise(plane, labels, 2)
        out3, a3 = g.fit_piecewise(plane, labels, 3)                             # label 2 has no pixel: its system is refused
        assert not a3[:, 2].any()
        np.testing.assert_array_equal(a3[:, :2], a)
        _same(out3, out, "an empty third segment")
        tones = torch.where(cols < w // 2, 60.0, 190.0)[None, :].expand(h, w).double()
        rms = lambda x: float(((x.double() - tones) ** 2).mean().sqrt())
        print("two-tone image, m = 8: RMS error against the noiseless tones: fit_piecewise %.3f, fit %.3f, the input %.3f" %
              (rms(out[0]), rms(g.fit(plane)[0]), rms(plane[0])))
        # the same with the mid-grey 125 taken off plane and tones (the basis holds no constant; +-65 is a step it can carry)
        centred, tones = (plane - 125.0).contiguous(), tones - 125.0
        print("... with 125 subtracted from both: fit_piecewise %.3f, fit %.3f, the input %.3f" %
              (rms(g.fit_piecewise(centred, labels, 2)[0][0]), rms(g.fit(centred)[0]), rms(centred[0])))
        g.close()
