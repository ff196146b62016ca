"""The spectral edge map of a graph handle (glf_graph_edges / Graph.edges, .boundary, .samples): per pixel and direction
sum_{c < dim} (fl32(scale_c) (Phi[nb][c] - Phi[px][c]))^2 for the E, S, SE and SW neighbours (k_graph_edges, the handle's stencil
kernel: strips of 62 image columns and blocks of 16 image rows, one per wave).

Shapes: those of tests/test_gpu_graph.py -- 61 x 47 (one strip, three row blocks, the last of 15 rows) at ld 32 / 64 / 128 / 256, so
one to four column chunks -- `tiny` (16 x 10: a strip wider than the image), and 509 x 515 once (nine strips, the last of 13
columns, 33 row blocks, the last of 3 rows), and 1021 x 1031 once, checked on the device: more units than resident waves, so that
some waves walk a second unit. Both storages. Where it helps the handle's Phi is overwritten with pseudo-random
values: distinct rows make any wrong neighbour visible.

The reference is tests/edges_ref.py: (a) the pinned arithmetic emulated bit for bit, (b) the float64 map with the bound
|q - q*| <= gamma(dim + 4) q* + dim 2^-149 ("Spectral edge map"), both checked on the CPU by tests/test_edges_ref.py,
seeded defects included."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import edges_ref as er  # noqa: E402
import glf  # noqa: E402
from test_gpu_graph import SHAPES, _dev, _grey_graph, _opt  # noqa: E402
from test_gpu_graph_cluster import TWO_TONE_SEED, _two_tone  # noqa: E402
from test_gpu_graph_compact import LD_SHAPES, _pair, _same  # noqa: E402
from test_gpu_graph_quad import _handle  # noqa: E402

ALL_SHAPES = LD_SHAPES + ["tiny"]
STORAGES = ["f32", "compact"]
SENTINEL = -77.0
ALL_DIRS = ("E", "S", "SE", "SW")


def _random_handle(ctx, shape, storage, seed):
    """(graph whose Phi[:, :m] is pseudo-random, with another magnitude per column, its own Phi float32 [N, ld]: Q on a compact
    handle)."""
    g, _, _ = _grey_graph(ctx, shape)
    m = g.info["m"]
    rng = np.random.default_rng(seed)
    vals = rng.normal(size=(g.phi.shape[0], m)) * 2.0 ** rng.integers(-6, 7, m)
    g.phi[:, :m] = _dev(ctx, vals.astype(np.float32))
    torch.cuda.synchronize()
    if storage == "compact":
        g.compact()
    return g, g.dequantize().cpu().numpy()


def _mask(h, w, seed):
    return (np.random.default_rng(seed).uniform(size=(h, w)) >= 0.25).astype(np.uint8)


def _edges(g, scale, dim, valid=None, dirs=ALL_DIRS):
    """glf_graph_edges itself, with the samples left in, into a buffer of four planes and a tail prefilled with a sentinel that no
    output can equal (outputs are >= 0): numpy [len(dirs), H, W] in the order of dirs. Every pixel of every requested plane must
    have been written, and nothing behind them. scale None: the Python default, 1 - lam."""
    ctx, (h, w), m = g.ctx, (g.info["height"], g.info["width"]), g.info["m"]
    n = h * w
    dirs = tuple(dirs)
    order = sorted(dirs, key=lambda d: glf.EDGE_DIRS[d])
    sc = np.ascontiguousarray((1.0 - g.eigenvalues if scale is None else np.asarray(scale, dtype=np.float64))[:dim])
    assert sc.shape == (dim,) and dim <= m
    buf = torch.full((4 * n + 64,), SENTINEL, dtype=torch.float32, device=ctx.device)
    dv = None if valid is None else _dev(ctx, np.ascontiguousarray(valid, dtype=np.uint8))
    torch.cuda.synchronize()
    rc = glf._lib.glf_graph_edges(g._g, C.c_uint(sum(glf.EDGE_DIRS[d] for d in dirs)), C.c_uint(dim), glf._ptr(sc),
                                  C.c_void_p(dv.data_ptr()) if dv is not None else None, C.c_void_p(buf.data_ptr()))
    assert rc == glf.OK, glf._lib.glf_ctx_last_error(ctx._ctx).decode()
    got = buf.cpu().numpy()
    planes, tail = got[:len(order) * n].reshape(len(order), h, w), got[len(order) * n:]
    assert not np.any(planes == np.float32(SENTINEL)), "a pixel of a requested plane was not written"
    assert np.all(tail == np.float32(SENTINEL)), "something was written behind the requested planes"
    return planes[[order.index(d) for d in dirs]].copy()


def _scale(m, seed):
    return np.random.default_rng(seed).uniform(0.5, 2.0, m)


def _assert_within(got, q, bound, what):
    err = np.abs(got.astype(np.float64) - q)
    frac = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: max |q - q*| / bound %.3f (max err %.3e)" % (what, frac, float(err.max())))
    assert np.isfinite(got).all() and np.all(err <= bound), (what, frac)
    return frac


# ---- 1. bit for bit against the emulation --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_bits_against_the_emulation(shape, storage):
    w, h = SHAPES[shape][:2]
    with glf.Context(0) as ctx:
        g, phi = _random_handle(ctx, shape, storage, 11)
        m = g.info["m"]
        scale = _scale(m, 12)
        for dim in sorted({1, min(5, m), m}):
            for valid in (None, _mask(h, w, 13)):
                got = _edges(g, scale, dim, valid)
                want, subnormal = er.emulate(phi, scale, dim, h, w, valid)
                assert not subnormal                                              # the one place where a flushing device could differ
                _same(got, want, "%s %s dim %d %s" % (shape, storage, dim, "masked" if valid is not None else "unmasked"))
        g.close()


def test_many_strips_and_row_blocks():
    """509 x 515 at ld 64: bit for bit against the emulation and within the bound of the float64 map, every pixel, masked."""
    w, h, m = 509, 515, 40
    with glf.Context(0) as ctx:
        g = ctx.graph(ctx.to_device(glf.synth_image(w, h, seed=3)), glf.default_options(num_samples=300, num_eigvals=m, epsilon=0.1))
        assert (g.info["m"], g.info["ld"]) == (m, 64)
        rng = np.random.default_rng(21)
        g.phi[:, :m] = _dev(ctx, rng.normal(size=(w * h, m)).astype(np.float32))
        torch.cuda.synchronize()
        phi = g.phi.cpu().numpy()
        scale, valid = _scale(m, 22), _mask(h, w, 23)
        got = _edges(g, scale, m, valid)
        g.close()
    want, subnormal = er.emulate(phi, scale, m, h, w, valid)
    assert not subnormal
    _same(got, want, "509 x 515")
    q, bound, _ = er.exact(phi, scale, m, h, w, valid)
    _assert_within(got, q, bound, "509 x 515 dim %d" % m)


def test_more_units_than_resident_waves():
    """1021 x 1031 at ld 64: 17 strips x 65 row blocks = 1105 units for the 4 x CUs waves that are resident at that ld (one workgroup
    per CU: profiles/graph_edges_kernel_resources.txt), so some waves walk a second unit -- the loads of its first row issued under the
    last row of the first, the ring reused. On the device, in torch: dim = 1 bit for bit (one subtraction, one multiplication, and
    fmaf(x, x, 0) is the exact square rounded once), dim = m within the bound of the float64 map, every pixel, masked."""
    w, h, m = 1021, 1031, 40
    units = -(-w // 62) * -(-h // 16)
    with glf.Context(0) as ctx:
        assert units > 4 * ctx.device_info()["num_cus"]
        g = ctx.graph(ctx.to_device(glf.synth_image(w, h, seed=3)), glf.default_options(num_samples=300, num_eigvals=m, epsilon=0.1))
        assert (g.info["m"], g.info["ld"]) == (m, 64)
        gen = torch.Generator(device=ctx.device)
        gen.manual_seed(71)
        g.phi[:, :m] = torch.randn((w * h, m), generator=gen, device=ctx.device)
        valid = torch.rand((h, w), generator=gen, device=ctx.device) >= 0.25
        scale = _scale(m, 72)
        s32 = torch.from_numpy(scale.astype(np.float32)).to(ctx.device)
        torch.cuda.synchronize()
        v8 = valid.to(torch.uint8).contiguous()
        sc = np.ascontiguousarray(scale, dtype=np.float64)
        runs = []
        for dim in (1, m):                                                       # the call itself, into planes prefilled with the sentinel
            buf = torch.full((4, h, w), SENTINEL, dtype=torch.float32, device=ctx.device)
            torch.cuda.synchronize()
            assert glf._lib.glf_graph_edges(g._g, C.c_uint(15), C.c_uint(dim), glf._ptr(sc), C.c_void_p(v8.data_ptr()), C.c_void_p(buf.data_ptr())) == glf.OK
            assert not bool((buf == SENTINEL).any()), "a pixel was not written"
            runs.append(buf)
        one, got = runs
        phi = g.phi.view(h, w, -1)[:, :, :m]
        worst = 0.0
        for k, name in enumerate(er.DIRS):
            dr, dc = er.OFFSETS[name]
            own = (slice(0, h - dr), slice(0, w - 1) if dc == 1 else slice(1, w) if dc == -1 else slice(0, w))
            nb = (slice(dr, h), slice(1, w) if dc == 1 else slice(0, w - 1) if dc == -1 else slice(0, w))
            live = valid[own] & valid[nb]
            d = phi[nb] - phi[own]                                               # f32: one subtraction
            x0 = d[:, :, 0] * s32[0]                                             # f32: one multiplication
            want1 = torch.zeros((h, w), dtype=torch.float32, device=ctx.device)
            want1[own] = torch.where(live, (x0.double() ** 2).float(), torch.zeros_like(x0))
            _same(one[k], want1, "%s dim 1" % name)
            q = torch.zeros((h, w), dtype=torch.float64, device=ctx.device)
            d64 = phi[nb].double() - phi[own].double()                           # exact
            q[own] = torch.where(live, ((d64 * s32.double()) ** 2).sum(-1), torch.zeros_like(x0, dtype=torch.float64))
            bound = (er.gamma(m + 4) + (m + 4) * 2.0 ** -52) * q + m * 2.0 ** -149
            err = (got[k].double() - q).abs()
            assert bool(torch.all(err <= bound)) and bool(torch.isfinite(got[k]).all()), name
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert not bool((got[k].view(torch.int32)[q == 0] != 0).any())      # +0 by bits wherever the edge is not live
        g.close()
    print("%d units: max |q - q*| / bound %.3f" % (units, worst))


# ---- 2. against fp64, every pixel ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_edges_against_fp64(shape, storage):
    """On the handle's own Phi (the extended eigenvectors: neighbouring rows nearly equal, the differences cancel) and the default
    response 1 - lam, and on pseudo-random rows."""
    w, h = SHAPES[shape][:2]
    worst = 0.0
    with glf.Context(0) as ctx:
        g, _ = _handle(ctx, shape, storage)
        m = g.info["m"]
        phi = g.dequantize().cpu().numpy()
        resp = 1.0 - g.eigenvalues
        for dim in sorted({1, min(5, m), m}):                                    # (ld256: m = 200)
            for valid in (None, _mask(h, w, 31)):
                got = _edges(g, None, dim, valid)
                assert got.shape == (4, h, w) and got.dtype == np.float32
                q, bound, _ = er.exact(phi, resp, dim, h, w, valid)
                worst = max(worst, _assert_within(got, q, bound, "%s %s dim %d" % (shape, storage, dim)))
        g.close()
        g, phi = _random_handle(ctx, shape, storage, 32)
        scale = _scale(m, 33)
        q, bound, _ = er.exact(phi, scale, m, h, w)
        worst = max(worst, _assert_within(_edges(g, scale, m), q, bound, "%s %s random rows" % (shape, storage)))
        g.close()
    print("%s %s: largest fraction of the bound %.3f" % (shape, storage, worst))


# ---- 3. structure, bit for bit -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_structure(shape):
    w, h = SHAPES[shape][:2]
    n = w * h
    lib = glf._lib
    with glf.Context(0) as ctx:
        g, phi = _random_handle(ctx, shape, "f32", 41)
        m = g.info["m"]
        scale, valid = _scale(m, 42), _mask(h, w, 43)
        full = _edges(g, scale, m, valid)
        _same(_edges(g, scale, m, valid), full, "two calls")
        # a plane does not depend on dirs, and Graph.edges returns the planes in the order asked for
        dvalid = _dev(ctx, valid)
        for dirs in (("E",), ("S",), ("SE",), ("SW",), ("E", "SW"), ("SW", "S"), ("S", "SE", "SW"), ("SW", "SE", "S", "E")):
            want = full[[er.DIRS.index(d) for d in dirs]]
            _same(_edges(g, scale, m, valid, dirs), want, "dirs %s" % (dirs,))
            _same(g.edges(dirs, response=scale, dim=m, valid=dvalid, exclude_samples=False), want, "Graph.edges, dirs %s" % (dirs,))
        _same(g.edges("SE", response=scale, dim=m, valid=dvalid, exclude_samples=False), full[2:3], "Graph.edges, one name")
        # both Python calls return with the library's stream drained, the reordered planes and the torch-formed boundary included:
        # the caller's stream does not wait for that stream by itself
        g.edges(("SW", "E"), response=scale, dim=m, valid=dvalid)
        assert ctx.stream.query()
        g.boundary(response=scale, dim=m, valid=dvalid)
        assert ctx.stream.query()
        _same(_edges(g, 2.0 * scale, m, valid), np.float32(4.0) * full, "the scale times 2")
        # every border, masked or out-of-image value is +0 by bits, and everything else is not
        _, _, live = er.exact(phi, scale, m, h, w, valid)
        assert not full.view(np.uint32)[~live].any() and np.all(full[live] > 0)
        unmasked = _edges(g, scale, m)
        _same(unmasked[live], full[live], "the mask does not change a live edge")
        assert not unmasked[0][:, -1].view(np.uint32).any() and not unmasked[2][:, -1].view(np.uint32).any()
        assert not unmasked[3][:, 0].view(np.uint32).any() and not unmasked[1:, -1, :].view(np.uint32).any()
        # zero-scale columns, appended or interleaved, change nothing
        if m >= 4:
            dim = m - 2
            short = _edges(g, scale, dim, valid)
            z = scale.copy()
            z[dim:] = 0.0
            _same(_edges(g, z, m, valid), short, "zero scales appended")
            z = scale.copy()
            z[[1, m // 2]] = 0.0
            keep = [c for c in range(m) if c not in (1, m // 2)]
            want, _ = er.emulate(np.ascontiguousarray(phi[:, keep]), scale[keep], m - 2, h, w, valid)
            _same(_edges(g, z, m, valid), want, "zero scales interleaved")
        # the raw call: the sentinel survives behind the requested planes
        buf = torch.full((4 * n + 64,), SENTINEL, dtype=torch.float32, device=ctx.device)
        sc = np.ascontiguousarray(scale, dtype=np.float64)
        dv = _dev(ctx, valid)
        torch.cuda.synchronize()
        rc = lib.glf_graph_edges(g._g, C.c_uint(glf.EDGE_DIRS["S"] | glf.EDGE_DIRS["SW"]), C.c_uint(m), glf._ptr(sc), C.c_void_p(dv.data_ptr()),
                                 C.c_void_p(buf.data_ptr()))
        assert rc == glf.OK
        _same(buf[:2 * n].view(2, h, w), full[[1, 3]], "the raw call")
        assert bool(torch.all(buf[2 * n:] == SENTINEL))
        # scale NULL = ones
        rc = lib.glf_graph_edges(g._g, C.c_uint(1), C.c_uint(m), None, None, C.c_void_p(buf.data_ptr()))
        assert rc == glf.OK
        _same(buf[:n].view(1, h, w), _edges(g, np.ones(m), m, None, ("E",)), "scale NULL")
        g.close()


@pytest.mark.parametrize("variant", ["plain", "scaled"])
@pytest.mark.parametrize("shape", LD_SHAPES)
def test_compact_equals_its_f32_twin(shape, variant):
    w, h = SHAPES[shape][:2]
    with glf.Context(0) as ctx:
        gc, gt, _, _, _, e = _pair(ctx, shape, variant)
        m = gc.info["m"]
        q = gt.phi.cpu().numpy()
        colmax = np.maximum(np.abs(q[:, :m]).max(axis=0), 1e-300)
        scale = _scale(m, 51) / colmax                                           # every column of Q at order one, whatever its scale
        for dim in sorted({1, min(5, m), m}):
            for valid in (None, _mask(h, w, 52)):
                a, b = _edges(gc, scale, dim, valid), _edges(gt, scale, dim, valid)
                _same(a, b, "%s %s dim %d" % (shape, variant, dim))
                assert np.any(a > 0)
        want, _ = er.emulate(q, scale, m, h, w)
        _same(_edges(gc, scale, m), want, "%s %s against the emulation on Q" % (shape, variant))
        if variant == "scaled":
            assert len(set(e[:m].tolist())) >= 3
        gc.close()
        gt.close()


def test_refusals_leave_the_output_untouched():
    lib = glf._lib
    with glf.Context(0) as ctx:
        g, _ = _handle(ctx, "ld64", "f32")
        m, n = g.info["m"], SHAPES["ld64"][0] * SHAPES["ld64"][1]
        out = torch.full((4, n), SENTINEL, dtype=torch.float32, device=ctx.device)
        torch.cuda.synchronize()
        O = C.c_void_p(out.data_ptr())
        ones = np.ones(m)
        with_nan, with_inf, too_big = ones.copy(), ones.copy(), ones.copy()
        with_nan[3] = np.nan
        with_inf[m - 1] = -np.inf
        too_big[0] = 1e39                                                         # finite in f64, not in f32
        cases = {"dirs = 0": (0, m, ones, "dirs"), "dirs = 16": (16, m, ones, "dirs"), "dim = 0": (15, 0, ones, "dim"),
                 "dim = m + 1": (15, m + 1, ones, "dim"), "NaN in scale": (15, m, with_nan, "finite"), "Inf in scale": (1, m, with_inf, "finite"),
                 "a scale beyond f32": (15, m, too_big, "finite")}
        for what, (dirs, dim, sc, word) in cases.items():
            assert lib.glf_graph_edges(g._g, C.c_uint(dirs), C.c_uint(dim), glf._ptr(sc), None, O) == glf.ERR_INVALID, what
            assert word in lib.glf_ctx_last_error(ctx._ctx).decode(), (what, lib.glf_ctx_last_error(ctx._ctx).decode())
        assert lib.glf_graph_edges(g._g, C.c_uint(15), C.c_uint(m), glf._ptr(ones), None, None) == glf.ERR_INVALID
        assert "d_out" in lib.glf_ctx_last_error(ctx._ctx).decode()
        assert lib.glf_graph_edges(None, C.c_uint(15), C.c_uint(m), glf._ptr(ones), None, O) == glf.ERR_INVALID
        assert lib.glf_graph_samples(None, glf._ptr(np.zeros(4, dtype=np.uint32))) == glf.ERR_INVALID
        assert lib.glf_graph_samples(g._g, None) == glf.ERR_INVALID
        assert "h_idx" in lib.glf_ctx_last_error(ctx._ctx).decode()
        torch.cuda.synchronize()
        assert bool(torch.all(out == SENTINEL))
        for bad in (dict(dirs=()), dict(dirs=("E", "N")), dict(dirs=("E", "E")), dict(dim=0), dict(dim=m + 1), dict(response=np.ones(m + 1)),
                    dict(valid=torch.zeros((3, 3), device=ctx.device))):
            with pytest.raises(ValueError):
                g.edges(**bad)
        # nothing faulted, and the next valid call succeeds
        assert g.edges().shape == (4, SHAPES["ld64"][1], SHAPES["ld64"][0])
        # a compact handle refuses by the folded value scale_0 2^e_0: 2^e_0 < 1 brings 1e39 back into f32, and 4e38 2^-e_0 folds to 4e38
        g.compact()
        e0 = int(g.column_exponents()[0])
        assert e0 < -4
        folded = ones.copy()
        folded[0] = 1e39
        assert lib.glf_graph_edges(g._g, C.c_uint(15), C.c_uint(m), glf._ptr(folded), None, O) == glf.OK
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        folded[0] = 4e38 * 2.0 ** -e0
        assert lib.glf_graph_edges(g._g, C.c_uint(15), C.c_uint(m), glf._ptr(folded), None, O) == glf.ERR_INVALID
        assert "folded" in lib.glf_ctx_last_error(ctx._ctx).decode()
        torch.cuda.synchronize()
        assert bool(torch.all(out == SENTINEL))
        g.close()


# ---- 4. samples() --------------------------------------------------------------------------------------------------------------------

def test_samples_are_the_samplers():
    w, h, ns = SHAPES["ld32"][:3]
    img = glf.synth_image(w, h, seed=3)
    with glf.Context(0) as ctx:
        for random, want in ((False, glf.Sampling(w, h, ns)), (True, glf.RandomSampling(w, h, ns, seed=5))):
            opt = _opt("ld32", sampling=glf.SAMPLING_RANDOM, sampling_seed=5) if random else _opt("ld32")
            with ctx.graph(ctx.to_device(img), opt) as g:
                s = g.samples()
                assert s.dtype == np.uint32 and s.shape == (g.info["p"],) and np.all(np.diff(s.astype(np.int64)) > 0)
                np.testing.assert_array_equal(s, want)
                g.compact()
                np.testing.assert_array_equal(g.samples(), want)


# ---- 5. what the feature is for ------------------------------------------------------------------------------------------------------

def _boundary_rows(e_plane, live_e, w):
    """(rows whose boundary edge is live, the fraction of them whose strongest E edge is the boundary, median boundary / median
    interior edge)."""
    b = w // 2 - 1                                                               # the edge between columns W // 2 - 1 and W // 2
    rows = np.flatnonzero(live_e[:, b])
    hit = float(np.mean(np.argmax(e_plane[rows], axis=1) == b))
    interior = live_e.copy()
    interior[:, b] = False
    return rows, hit, float(np.median(e_plane[rows, b]) / np.median(e_plane[interior]))


def test_the_tone_boundary_is_the_strongest_edge():
    """The two-tone image of the cluster tests at ld 32, m = dim = 8, the E plane without the sample pixels: in every image row the
    strongest edge is the tone boundary, and the median boundary edge is at least 50 times the median interior edge -- on the
    float64 map of the handle's own Phi, then on the library's map. With the sample pixels left in, the rows that contain one fail."""
    w, h = SHAPES["ld32"][:2]
    with glf.Context(0) as ctx:
        g = ctx.graph(ctx.to_device(_two_tone(TWO_TONE_SEED)), _opt("ld32"))
        m = g.info["m"]
        phi = g.phi.cpu().numpy()
        valid = np.ones(h * w, dtype=np.uint8)
        valid[g.samples()] = 0
        got = g.edges(("E",), dim=m).cpu().numpy()[0]
        with_samples = g.edges(("E",), dim=m, exclude_samples=False).cpu().numpy()[0]
        resp = 1.0 - g.eigenvalues
        g.close()
    q, _, live = er.exact(phi, resp, m, h, w, valid.reshape(h, w))
    for what, plane in (("f64 on the handle's Phi", q[0]), ("library", got.astype(np.float64))):
        rows, hit, ratio = _boundary_rows(plane, live[0], w)
        print("%s: %d rows with a live boundary edge, argmax is the boundary in %.3f of them, median boundary / interior %.1f" % (what, rows.size, hit, ratio))
        assert rows.size >= h // 2 and hit == 1.0 and ratio >= 50.0, what
    _, _, live_all = er.exact(phi, resp, m, h, w)
    rows, hit, ratio = _boundary_rows(with_samples.astype(np.float64), live_all[0], w)
    print("with the sample pixels: argmax is the boundary in %.3f of %d rows, median boundary / interior %.1f" % (hit, rows.size, ratio))
    assert hit < 1.0


# ---- 6. boundary() -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", ["ld64", "tiny"])
def test_boundary_against_its_restatement(shape, storage):
    w, h = SHAPES[shape][:2]
    with glf.Context(0) as ctx:
        g, _ = _handle(ctx, shape, storage)
        n = w * h
        for exclude, user in ((True, None), (False, _mask(h, w, 61)), (True, _mask(h, w, 62))):
            valid = np.ones(n, dtype=np.uint8) if user is None else user.reshape(-1).copy()
            if exclude:
                valid[g.samples()] = 0
            dv = None if user is None else _dev(ctx, user)
            planes = g.edges(valid=dv, exclude_samples=exclude).cpu().numpy()
            got = g.boundary(valid=dv, exclude_samples=exclude)
            assert tuple(got.shape) == (h, w) and got.dtype == torch.float32
            got = got.cpu().numpy()
            _, _, live = er.exact(np.zeros((n, 1), dtype=np.float32), [1.0], 1, h, w, valid.reshape(h, w))
            assert not planes.view(np.uint32)[~live].any()
            want, count = er.boundary(planes, live, dtype=np.float64)
            assert np.all(np.abs(got - want) <= 8 * er.U * want)                  # seven additions and one division, an ulp each
            assert not got.view(np.uint32)[count == 0].any()
            assert (count.max() == 8 or shape == "tiny") and count.min() < count.max() <= 8 and np.all(got >= 0)
        g.close()
