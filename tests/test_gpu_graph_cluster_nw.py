"""Spectral segmentation under unit-length rows and per-pixel weights: glf_graph_cluster_step_ex (k_graph_cluster's weight and normalise modes:
the embedding e(px) = rinv(px) scale o Phi[px][:dim], rinv = 1 / |scale o Phi[px][:dim]| formed in f32, and a weight plane in the
update), the driver glf_graph_segment_ex and Graph.cluster_step_ex / Graph.segment(normalize=, weight=) on top.

Shapes: those of tests/test_gpu_graph.py, as in tests/test_gpu_graph_cluster.py, whose decided / undecided scheme and helpers are used.
All references are torch f64 on the handle's own Phi. With u = 2^-24 and e the f64 embedding:
  score_j(px) = |c_j|^2 - 2 e . c_j
  normalize = 0: E_j = (CW + 4) u (|c_j|^2 + 2 sum_k |e_k| |c_jk|)            the plain step's bound
  normalize = 1: E_j = (3 CW / 2 + 12) u (|c_j|^2 + 2 sum_k |e_k| |c_jk|)     the dot-product chain, (CW + 4) u, and on the term bounded
                 by sum |e| |c| the half-row chain of the squared length, one add, the square root, the reciprocal and the final fma on
                 rinv: at most (CW / 2 + 8) u relative
Condition on the inputs, asserted from the f64 reference alone: at most 1 % of the pixels undecided. Two families of cases cannot meet it
by construction and are checked on their own: dim = 1 under normalize = 1 puts every row at +-1 (or 0), so that whole halves of the image
are decided or undecided together -- the cap is lifted, the decided / undecided checks stay and the reference embedding is asserted to be
+-1 / 0; a scale that is 0 on every used column embeds every pixel at the origin (rinv = 0 under normalize), and the label must then be
the argmin of fl32(|c_j|^2), the lowest index winning (test_zero_scale_labels_the_smallest_centroid).
Sums, given the kernel's own labels: |sums_j - sums64_j| <= ((CHAIN + CW / 2 + 10) u + N 2^-52) sum_{px in j} w rinv |phi_c|,
|mass_j - mass64_j| <= N 2^-52 sum_{px in j} w; counts and changed are exact."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
from test_gpu_graph import SHAPES, _grey_graph, _opt  # noqa: E402
from test_gpu_graph_cluster import CHAIN, KS, SENTINEL, U, _check_labels, _cw, _dims, _flat, _phi, _scale  # noqa: E402


def _embed64(phi, dim, scale, normalize):
    """(e [N, dim], rinv [N]) in f64 on phi's device."""
    r = phi[:, :dim] * (torch.ones(dim, dtype=torch.float64) if scale is None else torch.from_numpy(np.asarray(scale, dtype=np.float64))).to(phi.device)[None]
    if not normalize:
        return r, torch.ones(phi.shape[0], dtype=torch.float64, device=phi.device)
    n = (r * r).sum(dim=1).sqrt()
    rinv = torch.where(n > 0, 1.0 / n, torch.zeros_like(n))
    return r * rinv[:, None], rinv


def _scores(phi, cent, scale, cw, normalize):
    """(score [N, k], E [N, k]) in f64 on phi's device."""
    e = _embed64(phi, cent.shape[1], scale, normalize)[0]
    c = torch.from_numpy(cent).to(phi.device)
    c2 = (c * c).sum(dim=1)
    factor = (1.5 * cw + 12) if normalize else (cw + 4)
    return c2[None] - 2.0 * (e @ c.T), factor * U * (c2[None] + 2.0 * (e.abs() @ c.abs().T))


def _centroids(phi, k, dim, scale, normalize, rng):
    """The embedded rows of k distinct random pixels, each entry times (1 + 0.1 N(0, 1))."""
    px = rng.choice(phi.shape[0], size=k, replace=False)
    e = _embed64(phi[torch.from_numpy(px).to(phi.device)], dim, scale, normalize)[0].cpu().numpy()
    return e * (1.0 + 0.1 * rng.normal(size=e.shape))


def _weights(ctx, h, w, rng):
    """A random plane in [0, 2) of which about a tenth is exactly 0 -> (device float32 [h, w], f64 [N] on the CPU)."""
    x = rng.uniform(0.0, 2.0, (h, w)).astype(np.float32)
    x[rng.uniform(size=(h, w)) < 0.1] = 0.0
    return torch.from_numpy(x).to(ctx.device), torch.from_numpy(x.reshape(-1).astype(np.float64))


def _check_sums(phi, lab, k, dim, scale, normalize, w64, sums, counts, mass, cw, what):
    """sums [k, dim], counts [k] and mass [k] of a step against f64 on the labels the step wrote (lab: int64 [N], w64: f64 [N] or None,
    both on phi's device)."""
    n = phi.shape[0]
    rinv = _embed64(phi, dim, scale, normalize)[1]
    wt = torch.ones(n, dtype=torch.float64, device=phi.device) if w64 is None else w64
    onehot = (lab[:, None] == torch.arange(k, device=phi.device)[None]).double()
    coef = (wt * rinv)[:, None]
    want = (onehot.T @ (coef * phi[:, :dim])).cpu().numpy()
    bound = ((CHAIN + cw / 2 + 10) * U + n * 2.0 ** -52) * (onehot.T @ (coef * phi[:, :dim].abs())).cpu().numpy()
    mass64 = (onehot.T @ wt).cpu().numpy()
    bc = np.bincount(lab.cpu().numpy(), minlength=k)
    assert counts.dtype == np.uint64 and counts.shape == (k,) and sums.shape == (k, dim) and mass.dtype == np.float64 and mass.shape == (k,)
    np.testing.assert_array_equal(counts.astype(np.int64), bc, err_msg=what)
    assert int(counts.sum()) == n, what
    err, merr = np.abs(sums - want), np.abs(mass - mass64)
    print("%s: max |sums - sums64| / bound %.3f, max |mass - mass64| / sum w %.2e" %
          (what, float((err / np.maximum(bound, 1e-300)).max()), float((merr / np.maximum(mass64, 1e-300)).max())))
    assert np.all(err <= bound), what
    assert np.all(merr <= n * 2.0 ** -52 * mass64), what
    if w64 is None:
        np.testing.assert_array_equal(mass, counts.astype(np.float64), err_msg=what)


# ---- 1. labels against fp64 ---------------------------------------------------------------------------------------------------------

# The centroid seed, chosen as CENT_SEED of tests/test_gpu_graph_cluster.py is: the first of 101, 102, ... for which every case of
# every shape keeps the condition on the inputs (at most 1 % of the pixels undecided) from the f64 reference alone. Tried: 101 (tiny, k 32,
# dim 4 under a scale: 2 of 160 pixels, and 1 % of 160 is 1.6), 102 (ld128, k 32, dim 1, normalize 0: 253 of 2867 pixels between two of
# 32 centroids on a line), 103 (no case over the cap; of 101 .. 110, 104, 105, 107 and 109 hold it too).
CENT_SEED = 103


def _label_case(phi, shape, k, dim, normalize, scaled, seed=None):
    """(scale, centroids) of one case, from a random stream of its own (the weights do not enter the assignment)."""
    rng = np.random.default_rng([CENT_SEED if seed is None else seed, list(SHAPES).index(shape), k, dim, normalize, scaled])
    scale = _scale(dim, rng) if scaled else None
    return scale, _centroids(phi, k, dim, scale, normalize, rng)


def _label_cases(m):
    """(k, dim, normalize, scaled) of check 1, without the cases whose used columns are all scaled by 0 (dim = 1 under a scale that
    holds one 0: test_zero_scale_labels_the_smallest_centroid)."""
    return [c for c in itertools.product(KS, _dims(m), (0, 1), (0, 1)) if not (c[1] == 1 and c[3])]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_labels_against_fp64(shape):
    width, h, _, _, m, ld = SHAPES[shape]
    rng = np.random.default_rng(11)
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, shape)[0]
        phi = _phi(g, "cpu")
        over = []
        for k, dim, normalize, scaled in _label_cases(m):
            scale, cent = _label_case(phi, shape, k, dim, normalize, scaled)
            S, E = _scores(phi, cent, scale, _cw(ld), normalize)
            for weighted in (0, 1):
                weight = _weights(ctx, h, width, rng)[0] if weighted else None
                labels, sums, counts, mass, changed = g.cluster_step_ex(cent, scale, normalize=bool(normalize), weight=weight)
                assert labels.dtype == torch.int32 and tuple(labels.shape) == (h, width) and changed == 0
                lab = _flat(labels).cpu()
                what = "%s k %d dim %d normalize %d scale %s weight %s" % (shape, k, dim, normalize, "random" if scaled else "none",
                                                                          "random" if weighted else "none")
                signs = bool(normalize) and dim == 1                              # every row at +-1: decided or not by halves
                _check_labels(lab, S, E, what, cap=not signs, over=over)
                if signs:
                    e = _embed64(phi, dim, scale, 1)[0]
                    assert bool((((e.abs() - 1.0).abs() <= 2.0 ** -52) | (e == 0.0)).all()), what
        g.close()
    assert not over, over                                                         # the condition on the inputs: at most 1 % undecided


@pytest.mark.parametrize("shape", ["ld32", "ld128", "tiny"])
def test_zero_scale_labels_the_smallest_centroid(shape):
    """A scale that is 0 on every used column: e = 0 (under normalize rinv = 0), every score is fl32(|c_j|^2) exactly on both sides, and
    every pixel takes the argmin, the lowest index winning the tie between two equal centroids; the sums are then exactly 0."""
    width, h, _, _, m, ld = SHAPES[shape]
    n = width * h
    rng = np.random.default_rng(12)
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, shape)[0]
        weight = _weights(ctx, h, width, rng)[0]
        for k, dim, normalize in itertools.product(KS, (1, min(m, 7)), (0, 1)):
            cent = rng.normal(size=(k, dim))
            if k > 2:
                cent[k - 1] = cent[1]                                             # twins: the higher index never wins
            c2 = (cent ** 2).sum(axis=1).astype(np.float32)
            want = int(np.argmin(c2))                                             # (numpy's argmin takes the first of equals)
            for wt in (None, weight):
                labels, sums, counts, mass, _ = g.cluster_step_ex(cent, np.zeros(dim), normalize=bool(normalize), weight=wt)
                what = (shape, k, dim, normalize, wt is not None)
                assert bool((labels == want).all()), what
                assert counts[want] == n and int(counts.sum()) == n, what
                if normalize:
                    assert not sums.any(), what                                   # t = w rinv = 0
                if wt is None:
                    assert mass[want] == n, what
        g.close()


# ---- 2. sums, mass, counts and changed, given the kernel's own labels -----------------------------------------------------------------

@pytest.mark.parametrize("shape", list(SHAPES))
def test_sums_mass_counts_and_changed(shape):
    width, h, _, _, m, ld = SHAPES[shape]
    rng = np.random.default_rng(202)
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, shape)[0]
        phi = _phi(g, "cpu")
        for k, dim, normalize, weighted in itertools.product(KS, _dims(m), (0, 1), (0, 1)):
            scale = _scale(dim, rng) if (k + dim) % 2 and dim > 1 else None
            cent = _centroids(phi, k, dim, scale, normalize, rng)
            weight, w64 = _weights(ctx, h, width, rng) if weighted else (None, None)
            kw = dict(normalize=bool(normalize), weight=weight)
            what = "%s k %d dim %d normalize %d weighted %d" % (shape, k, dim, normalize, weighted)
            labels, sums, counts, mass, changed = g.cluster_step_ex(cent, scale, **kw)
            assert changed == 0                                                   # no prev
            lab = _flat(labels).cpu()
            _check_sums(phi, lab, k, dim, scale, normalize, w64, sums, counts, mass, _cw(ld), what)
            prev = torch.from_numpy(rng.integers(0, k, size=(h, width)).astype(np.int32)).to(ctx.device)
            moved = int(np.count_nonzero(prev.cpu().numpy().reshape(-1) != lab.numpy()))   # pixels, whatever their weight
            l2, s2, c2, m2, ch2 = g.cluster_step_ex(cent, scale, prev=prev, **kw)          # a separate buffer
            assert ch2 == moved, what
            inplace = prev.clone()
            l3, s3, c3, m3, ch3 = g.cluster_step_ex(cent, scale, prev=inplace, labels=inplace, **kw)   # prev is labels
            assert l3 is inplace and ch3 == moved, what
            for l, s, c, ms in ((l2, s2, c2, m2), (l3, s3, c3, m3)):
                assert torch.equal(l, labels), what
                np.testing.assert_array_equal(s.view(np.int64), sums.view(np.int64), err_msg=what)
                np.testing.assert_array_equal(c, counts, err_msg=what)
                np.testing.assert_array_equal(ms.view(np.int64), mass.view(np.int64), err_msg=what)
        g.close()


# ---- 3. exact properties --------------------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _raw_step(g, emb, cent, scale, prev, labels, k=None, dim=None, sums=True, counts=True, mass=True, changed=True):
    """glf_graph_cluster_step_ex itself on device pointers (ints or None) -> (status, sums, counts, mass, changed)."""
    kk, dd = (cent.shape if cent is not None else (2, 2))
    k, dim = kk if k is None else k, dd if dim is None else dim
    s, c, ms, ch = np.zeros((max(k, 1), max(dim, 1))), np.zeros(max(k, 1), dtype=np.uint64), np.zeros(max(k, 1)), C.c_uint64(12345)
    torch.cuda.synchronize()
    rc = glf._lib.glf_graph_cluster_step_ex(g._g, C.byref(emb) if emb is not None else None, C.c_uint(k), C.c_uint(dim), glf._ptr(cent),
                                            glf._ptr(scale), prev, labels, glf._ptr(s) if sums else None, glf._ptr(c) if counts else None,
                                            glf._ptr(ms) if mass else None, C.byref(ch) if changed else None)
    return rc, s, c, ms, int(ch.value)


@pytest.mark.parametrize("shape", ["ld32", "ld64", "ld256"])
def test_exact_properties(shape):
    width, h, _, _, m, ld = SHAPES[shape]
    n = width * h
    rng = np.random.default_rng(303)
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, shape)[0]
        phi = _phi(g, "cpu")
        dim = min(m, 64)
        weight, w64 = _weights(ctx, h, width, rng)
        ones = torch.ones((h, width), dtype=torch.float32, device=ctx.device)
        for k in (1, 5, 31):
            scale = _scale(dim, rng)
            prev = torch.from_numpy(rng.integers(0, k, size=(h, width)).astype(np.int32)).to(ctx.device)
            # a plain embedding: the bits of glf_graph_cluster_step, through Python and with emb NULL
            cent = _centroids(phi, k, dim, scale, 0, rng)
            l0, s0, c0, ch0 = g.cluster_step(cent, scale, prev=prev)
            l1, s1, c1, m1, ch1 = g.cluster_step_ex(cent, scale, prev=prev)
            buf = torch.full((n,), SENTINEL, dtype=torch.int32, device=ctx.device)
            rc, s2, c2, m2, ch2 = _raw_step(g, None, cent, scale, C.c_void_p(prev.data_ptr()), C.c_void_p(buf.data_ptr()))
            assert rc == glf.OK and torch.equal(l0, l1) and torch.equal(l0.reshape(-1), buf) and ch0 == ch1 == ch2
            for s, c, ms in ((s1, c1, m1), (s2, c2, m2)):
                np.testing.assert_array_equal(_bits(s), _bits(s0))
                np.testing.assert_array_equal(c, c0)
                np.testing.assert_array_equal(ms, c0.astype(np.float64))
            # weight = 1 without normalize: the weight mode, the plain step's labels (and, the operand being 1 and both instances
            # running one tile per wave at this size, its sums)
            l3, s3, c3, m3, ch3 = g.cluster_step_ex(cent, scale, prev=prev, weight=ones)
            assert torch.equal(l3, l0) and ch3 == ch0
            np.testing.assert_array_equal(_bits(s3), _bits(s0))
            np.testing.assert_array_equal(c3, c0)
            np.testing.assert_array_equal(m3, c0.astype(np.float64))
            for normalize in (False, True):
                cent = _centroids(phi, k, dim, scale, normalize, rng)
                la, sa, ca, ma, _ = g.cluster_step_ex(cent, scale, normalize=normalize, weight=weight)
                # two calls give the same bits
                lb, sb, cb, mb, _ = g.cluster_step_ex(cent, scale, normalize=normalize, weight=weight)
                assert torch.equal(la, lb)
                np.testing.assert_array_equal(_bits(sa), _bits(sb))
                np.testing.assert_array_equal(_bits(ma), _bits(mb))
                np.testing.assert_array_equal(ca, cb)
                # weights x 2: the same labels, sums and mass exactly doubled
                lc, sc, cc, mc, _ = g.cluster_step_ex(cent, scale, normalize=normalize, weight=weight * 2.0)
                assert torch.equal(la, lc)
                np.testing.assert_array_equal(_bits(sc), _bits(2.0 * sa))
                np.testing.assert_array_equal(_bits(mc), _bits(2.0 * ma))
                np.testing.assert_array_equal(ca, cc)
                # the weights do not enter the assignment
                ld_, sd, cd, md, _ = g.cluster_step_ex(cent, scale, normalize=normalize)
                assert torch.equal(la, ld_)
                np.testing.assert_array_equal(ca, cd)
                # a far centroid: no label moves, no bit of the other sums changes
                far = np.zeros(dim)
                far[int(np.flatnonzero(scale)[0])] = 1e3 * max(1.0, float(_embed64(phi, dim, scale, normalize)[0].norm(dim=1).max()))
                le, se, ce, me, _ = g.cluster_step_ex(np.concatenate([cent, far[None]]), scale, normalize=normalize, weight=weight)
                assert torch.equal(la, le), (shape, k, normalize)
                np.testing.assert_array_equal(_bits(se[:k]), _bits(sa))
                np.testing.assert_array_equal(_bits(me[:k]), _bits(ma))
                np.testing.assert_array_equal(ce[:k], ca)
                assert ce[k] == 0 and me[k] == 0 and not se[k].any()
                # a pixel of weight 0 is labelled, and the reference without those pixels gives the same sums and mass
                lab = _flat(la).cpu()
                assert int((w64 == 0).sum()) > 0 and int(lab.min()) >= 0 and int(lab.max()) < k
                keep = w64 > 0
                onehot = (lab[keep][:, None] == torch.arange(k)[None]).double()
                rinv = _embed64(phi, dim, scale, normalize)[1][keep]
                coef = (w64[keep] * rinv)[:, None]
                want = (onehot.T @ (coef * phi[keep, :dim])).numpy()
                bound = ((CHAIN + _cw(ld) / 2 + 10) * U + n * 2.0 ** -52) * (onehot.T @ (coef * phi[keep, :dim].abs())).numpy()
                assert np.all(np.abs(sa - want) <= bound)
                mass64 = (onehot.T @ w64[keep]).numpy()
                assert np.all(np.abs(ma - mass64) <= n * 2.0 ** -52 * mass64)
            # scale x 2 under normalize: the same embedding, so the same labels; rinv, and with it the sums, exactly halved
            cent = _centroids(phi, k, dim, scale, 1, rng)
            la, sa, ca, ma, _ = g.cluster_step_ex(cent, scale, normalize=True, weight=weight)
            lf, sf, cf, mf, _ = g.cluster_step_ex(cent, 2.0 * scale, normalize=True, weight=weight)
            assert torch.equal(la, lf)
            np.testing.assert_array_equal(_bits(sf), _bits(0.5 * sa))
            np.testing.assert_array_equal(_bits(mf), _bits(ma))
            np.testing.assert_array_equal(ca, cf)
        g.close()


# ---- 4. the grid-strided loop -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,ld", [(8, 32), (200, 256)])
def test_cluster_step_ex_many_tiles_per_wave(m, ld):
    """509 x 515 = 8191 tiles of 32 pixels and one of 23, more than a resident grid has waves: every wave runs its tile loop several
    times, whole chains are flushed into f64 and the next tile's loads, weights included, fly under the MFMAs. Both flags on, k = 32.
    Reference and the checks of 1 and 2 in torch f64 on the device."""
    width, h = 509, 515
    n = width * h
    rng = np.random.default_rng(ld)
    with glf.Context(0) as ctx:
        assert (n + 31) // 32 > 4 * 7 * ctx.device_info()["num_cus"]
        g = ctx.graph(ctx.to_device(glf.synth_image(width, h, seed=3)), glf.default_options(num_samples=300, num_eigvals=m, epsilon=0.1))
        assert (g.info["p"], g.info["m"], g.info["ld"]) == (324, m, ld)
        phi = _phi(g)
        k, dim = 32, min(m, 64)
        weight, w64 = _weights(ctx, h, width, rng)
        for scale in (None, _scale(dim, rng)):
            cent = _centroids(phi, k, dim, scale, 1, rng)
            what = "509 x 515 ld %d scale %s" % (ld, "none" if scale is None else "random")
            prev = torch.from_numpy(rng.integers(0, k, size=(h, width)).astype(np.int32)).to(ctx.device)
            labels, sums, counts, mass, changed = g.cluster_step_ex(cent, scale, prev=prev, normalize=True, weight=weight)
            lab = _flat(labels)
            S, E = _scores(phi, cent, scale, _cw(ld), 1)
            _check_labels(lab, S, E, what)
            _check_sums(phi, lab, k, dim, scale, 1, w64.to(phi.device), sums, counts, mass, _cw(ld), what)
            assert changed == int((prev != labels).sum()), what
        g.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_labels_untouched():
    width, h, _, _, m, ld = SHAPES["ld32"]
    n = width * h
    rng = np.random.default_rng(606)
    lib = glf._lib
    size = C.sizeof(glf.ClusterEmbed)
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, "ld32")[0]
        phi = _phi(g, "cpu")
        cent = _centroids(phi, 5, m, None, 1, rng)
        weight = _weights(ctx, h, width, rng)[0]
        buf = torch.full((n,), SENTINEL, dtype=torch.int32, device=ctx.device)
        L = C.c_void_p(buf.data_ptr())

        def bad(x, v):
            y = np.array(x, dtype=np.float64)
            y.reshape(-1)[3] = v
            return y

        ones = np.ones(m)
        good = glf.ClusterEmbed(size, 1, weight.data_ptr())
        cases = {
            "struct_size + 8": dict(emb=glf.ClusterEmbed(size + 8, 1, None)), "struct_size 0": dict(emb=glf.ClusterEmbed(0, 0, None)),
            "normalize 2": dict(emb=glf.ClusterEmbed(size, 2, None)), "normalize -1": dict(emb=glf.ClusterEmbed(size, -1, weight.data_ptr())),
            "mass NULL": dict(mass=False), "mass NULL, emb NULL": dict(emb=None, mass=False),
            "cent NULL": dict(cent=None, k=5, dim=m), "labels NULL": dict(labels=None), "sums NULL": dict(sums=False),
            "counts NULL": dict(counts=False), "changed NULL": dict(changed=False), "k = 0": dict(k=0), "k = 33": dict(cent=np.zeros((33, m))),
            "dim = 0": dict(dim=0), "dim = m + 1": dict(cent=np.zeros((5, m + 1))), "dim = 65": dict(cent=np.zeros((5, 65))),
            "NaN centroid": dict(cent=bad(cent, np.nan)), "Inf centroid": dict(cent=bad(cent, np.inf)),
            "-Inf centroid": dict(cent=bad(cent, -np.inf)), "NaN scale": dict(scale=bad(ones, np.nan)), "Inf scale": dict(scale=bad(ones, np.inf)),
        }
        for what, kw in cases.items():
            args = dict(emb=good, cent=cent, scale=None, prev=None, labels=L)
            args.update(kw)
            rc = _raw_step(g, args.pop("emb"), args.pop("cent"), args.pop("scale"), args.pop("prev"), args.pop("labels"), **args)[0]
            assert rc == glf.ERR_INVALID, what
            assert bool((buf == SENTINEL).all()), what
        rc = lib.glf_graph_cluster_step_ex(None, C.byref(good), C.c_uint(5), C.c_uint(m), glf._ptr(cent), None, None, L, glf._ptr(np.zeros((5, m))),
                                           glf._ptr(np.zeros(5, dtype=np.uint64)), glf._ptr(np.zeros(5)), C.byref(C.c_uint64()))
        assert rc == glf.ERR_INVALID                                              # a NULL handle
        # the driver
        h_cent = np.ascontiguousarray(cent[:2, :2])
        st = glf.SegmentStats()
        h_mass = np.full(2, 12345.0)

        def seg(k=2, dim=2, init=1, osize=C.sizeof(glf.SegmentOptions), scale=None, handle=g._g, labels=L, c=h_cent, opt=True, emb=good):
            o = glf.SegmentOptions(osize, k, dim, 50, 4096, init, 1, scale.ctypes.data if scale is not None else None)
            torch.cuda.synchronize()
            return lib.glf_graph_segment_ex(handle, C.byref(o) if opt else None, C.byref(emb) if emb is not None else None, labels, glf._ptr(c),
                                            C.byref(st), glf._ptr(h_mass))

        for what, kw in {"struct_size + 8": dict(osize=C.sizeof(glf.SegmentOptions) + 8), "struct_size 0": dict(osize=0), "k = 0": dict(k=0),
                         "k = 33": dict(k=33), "dim = 0": dict(dim=0), "dim = m + 1": dict(dim=m + 1), "init = 2": dict(init=2),
                         "init = -1": dict(init=-1), "NaN centroid": dict(c=np.array([[np.nan, 1.0], [2.0, 3.0]])),
                         "Inf centroid": dict(c=np.array([[0.0, 1.0], [2.0, np.inf]])), "NaN scale": dict(scale=np.array([1.0, np.nan])),
                         "opt NULL": dict(opt=False), "labels NULL": dict(labels=None), "cent NULL": dict(c=None), "handle NULL": dict(handle=None),
                         "emb struct_size": dict(emb=glf.ClusterEmbed(size - 4, 1, None)), "emb normalize 2": dict(emb=glf.ClusterEmbed(size, 2, None)),
                         "k = 33, emb NULL": dict(k=33, emb=None)}.items():
            assert seg(**kw) == glf.ERR_INVALID, what
            assert bool((buf == SENTINEL).all()), what
            assert bool((h_mass == 12345.0).all()), what
        # a sample whose weights are all 0, or hold a negative one, cannot be seeded: refused before any label is written
        for fill in (0.0, -1.0):
            wbad = torch.full((h, width), fill, dtype=torch.float32, device=ctx.device)
            assert seg(init=0, emb=glf.ClusterEmbed(size, 1, wbad.data_ptr())) == glf.ERR_INVALID, fill
            assert bool((buf == SENTINEL).all()), fill
        with pytest.raises(glf.GlfError) as e:
            g.segment(33, normalize=True)
        assert e.value.status == glf.ERR_INVALID
        with pytest.raises(glf.GlfError):
            g.cluster_step_ex(np.zeros((2, m + 1)), normalize=True)
        with pytest.raises(ValueError):
            g.cluster_step_ex(cent, weight=torch.zeros((h, width + 1), dtype=torch.float32, device=ctx.device))
        with pytest.raises(AssertionError):
            g.cluster_step_ex(cent, weight=torch.zeros((h, width), dtype=torch.float64, device=ctx.device))
        with pytest.raises(ValueError):
            g.segment(2, weight=torch.zeros((h + 1, width), dtype=torch.float32, device=ctx.device))
        # nothing faulted: the next valid calls succeed
        assert seg(init=0, c=np.full((2, 2), np.nan)) == glf.OK and st.iterations >= 1 and float(h_mass.sum()) > 0
        labels = g.cluster_step_ex(cent, normalize=True, weight=weight)[0]
        assert int(labels.min()) >= 0 and int(labels.max()) < 5
        g.close()


# ---- 6. the driver --------------------------------------------------------------------------------------------------------------------

# The noise seed of the four-quadrant image. (c)'s input condition -- no pixel of any iteration of the f64 Lloyd run with unit rows is
# undecided -- is asserted below on the handle's own Phi. Tried: 100 (holds: 5 iterations, no pixel undecided; so do 101 .. 107).
QUAD_SEED = 100
QUAD_TONES = (40.0, 100.0, 160.0, 220.0)                                          # top left, top right, bottom left, bottom right


def _quadrants(seed):
    """(image uint8 [47, 61], the quadrant of every pixel int64 [N], the centre pixel of each quadrant)."""
    w, h = SHAPES["ld32"][:2]
    q = (np.arange(h)[:, None] >= h // 2) * 2 + (np.arange(w)[None] >= w // 2)
    img = np.asarray(QUAD_TONES)[q] + np.random.default_rng(seed).uniform(-12, 12, (h, w))
    centres = [(h // 4) * w + w // 4, (h // 4) * w + w // 2 + (w - w // 2) // 2, (h // 2 + (h - h // 2) // 2) * w + w // 4,
               (h // 2 + (h - h // 2) // 2) * w + w // 2 + (w - w // 2) // 2]
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), torch.from_numpy(q.reshape(-1).astype(np.int64)), centres


def _agreement(lab, quad, k=4):
    """The largest fraction of pixels on which a relabelling of lab agrees with quad."""
    return max(float((torch.tensor(p)[lab] == quad).double().mean()) for p in itertools.permutations(range(k)))


def _lloyd64(phi, c0, normalize, iters=None, cw=32, w64=None, max_iter=50):
    """Lloyd's iteration in f64 on the embedded rows (the driver's convergence rule when iters is None) ->
    (labels, centroids, iterations, the undecided pixels of every iteration)."""
    e = _embed64(phi, c0.shape[1], None, normalize)[0]
    wt = torch.ones(phi.shape[0], dtype=torch.float64) if w64 is None else w64
    c, lab, und, it = c0.copy(), None, [], 0
    while it < (max_iter if iters is None else iters):
        S, E = _scores(phi, c, None, cw, normalize)
        new = S.argmin(dim=1)
        ar = torch.arange(S.shape[0])
        low = S - E
        low[ar, new] = float("inf")
        und.append(int((~(S[ar, new] + E[ar, new] < low.min(dim=1).values)).sum()))
        done = iters is None and lab is not None and bool((new == lab).all())
        lab = new
        it += 1
        for j in range(c.shape[0]):
            mj = wt * (lab == j)
            if float(mj.sum()) > 0:
                c[j] = ((mj[:, None] * e).sum(dim=0) / mj.sum()).numpy()
        if done:
            break
    return lab, c, it, und


def _python_lloyd(g, c0, max_iter=50, **kw):
    """The driver restated on cluster_step_ex + glf.cluster_update_w."""
    labels, sums, counts, mass, changed = g.cluster_step_ex(c0, **kw)
    cent, it, converged = glf.cluster_update_w(sums, mass, None, c0), 1, 0
    while it < max_iter and not converged:
        labels, sums, counts, mass, changed = g.cluster_step_ex(cent, prev=labels, labels=labels, **kw)
        converged = int(changed == 0)
        it += 1
        cent = glf.cluster_update_w(sums, mass, None, cent)
    return labels, cent, it, converged, changed, counts, mass


def test_segment_driver_finds_the_quadrants():
    """Four flat quadrants under noise, m = dim = 8, epsilon = 0.1: the rows of the loosely converged Phi differ in length so much that
    k-means on the raw rows never finds the quadrants, and on the unit-length rows it does. Without glf_graph_segment_ex there is no
    normalize argument: this test fails without the feature."""
    w, h = SHAPES["ld32"][:2]
    n, k, dim = w * h, 4, 8
    img, quad, centres = _quadrants(QUAD_SEED)
    with glf.Context(0) as ctx:
        g = ctx.graph(ctx.to_device(img), _opt("ld32"))
        phi = _phi(g, "cpu")
        e1 = _embed64(phi, dim, None, 1)[0]
        c0 = e1[centres].numpy().copy()                                           # unit rows
        c0_raw = phi[centres, :dim].numpy().copy()
        # (a) the driver is the loop
        labels, cent, st = g.segment(k, dim, init=c0, normalize=True)
        pl, pc, pit, pconv, pchanged, pcounts, pmass = _python_lloyd(g, c0, normalize=True)
        assert st["iterations"] == pit and st["converged"] == pconv == 1 and st["changed_last"] == pchanged == 0
        assert torch.equal(labels, pl)
        np.testing.assert_array_equal(st["counts"], pcounts)
        np.testing.assert_array_equal(st["mass"], pmass)
        np.testing.assert_array_equal(st["mass"], st["counts"].astype(np.float64))   # no weight plane: the mass is the count
        assert float(np.abs(cent - pc).max()) <= 1e-12 * float(np.abs(pc).max())
        assert labels.dtype == torch.int32 and tuple(labels.shape) == (h, w) and st["counts"].sum() == n
        # (b) a fixed point: one more step moves nothing
        l2, _, _, _, moved = g.cluster_step_ex(cent, prev=labels, normalize=True)
        assert moved == 0 and torch.equal(l2, labels)
        # (c) the same number of f64 Lloyd iterations in torch, with unit rows; the input condition: nobody undecided, ever
        lab64, c64, _, und = _lloyd64(phi, c0, 1, iters=st["iterations"])
        print("four quadrants seed %d: %d iterations, undecided per iteration %s" % (QUAD_SEED, st["iterations"], und))
        assert not any(und), und
        assert torch.equal(_flat(labels).cpu(), lab64)
        # (d) from the f64 reference alone: unit rows find the quadrants, raw rows do not; and the kernel's labels do
        unit = _agreement(lab64, quad)
        raw = _agreement(_lloyd64(phi, c0_raw, 0)[0], quad)
        print("agreement with the quadrants: unit rows %.4f, raw rows %.4f" % (unit, raw))
        assert unit >= 0.9 and raw <= 0.6, (unit, raw)
        assert _agreement(_flat(labels).cpu(), quad) >= 0.9
        # (e) weights: 1 on the left half, 0 on the right; k = 2 from the two left quadrants' centres: both centroids are means of left
        # pixels only, and the right half adds no mass
        left = (torch.arange(n) % w < w // 2)
        wplane = left.reshape(h, w).float().to(ctx.device)
        c2 = c0[[0, 2]]
        lw, cw_, sw = g.segment(2, dim, init=c2, normalize=True, weight=wplane)
        lab = _flat(lw).cpu()
        assert sw["converged"] == 1 and int(sw["counts"].sum()) == n
        for j in range(2):
            members = left & (lab == j)
            assert sw["mass"][j] == float(members.sum()) and sw["counts"][j] == int((lab == j).sum())
            assert int(members.sum()) > 0
            want = e1[members].mean(dim=0).numpy()
            bound = ((CHAIN + 32 / 2 + 10) * U + n * 2.0 ** -52) * e1[members].abs().mean(dim=0).numpy() + 4 * 2.0 ** -53 * np.abs(want)
            assert np.all(np.abs(cw_[j] - want) <= bound), (j, float(np.abs(cw_[j] - want).max()))
        assert float(sw["mass"].sum()) == float(left.sum())
        l64w, _, _, undw = _lloyd64(phi, c2, 1, iters=sw["iterations"], w64=left.double())
        print("weighted run: %d iterations, undecided per iteration %s" % (sw["iterations"], undw))
        if not any(undw):                                                         # (where the f64 run is decided, it gives the same labels)
            assert torch.equal(lab, l64w)
        # (f) seeding: reproducible, and the documented rule (the sample's rows normalised in f64, column by column, and its weights)
        wrand = _weights(ctx, h, w, np.random.default_rng(7))
        for sample_rows, wt in ((4096, None), (500, None), (500, wrand)):
            kw = dict(normalize=True, weight=None if wt is None else wt[0])
            la, ca, sa = g.segment(k, dim, seed=7, sample_rows=sample_rows, **kw)
            lb, cb, sb = g.segment(k, dim, seed=7, sample_rows=sample_rows, **kw)
            assert torch.equal(la, lb) and sa["iterations"] == sb["iterations"]
            np.testing.assert_array_equal(ca, cb)
            np.testing.assert_array_equal(sa["mass"], sb["mass"])
            ns = min(sample_rows, n)
            idx = [(i * n) // ns for i in range(ns)]
            rows = phi[idx, :dim].numpy().copy()
            n2 = np.zeros(ns)
            for c in range(dim):
                n2 += rows[:, c] * rows[:, c]
            rows *= np.where(n2 > 0, 1.0 / np.sqrt(np.where(n2 > 0, n2, 1.0)), 0.0)[:, None]
            init = glf.cluster_seed_w(rows, None if wt is None else wt[1].numpy()[idx], k, seed=7)
            lc, cc, sc = g.segment(k, dim, init=init, **kw)
            assert torch.equal(la, lc) and sa["iterations"] == sc["iterations"]
            np.testing.assert_array_equal(ca, cc)
        # the default segment is untouched: no mass in its dict, the plain driver's labels through the _ex entry with a plain embedding
        lp, cp, sp = g.segment(k, dim, init=c0_raw)
        assert "mass" not in sp
        buf = torch.empty((h, w), dtype=torch.int32, device=ctx.device)
        hc, st2, hm = c0_raw.copy(), glf.SegmentStats(), np.zeros(k)
        o = glf.SegmentOptions(C.sizeof(glf.SegmentOptions), k, dim, 50, 4096, 1, 1, None)
        torch.cuda.synchronize()
        assert glf._lib.glf_graph_segment_ex(g._g, C.byref(o), None, C.c_void_p(buf.data_ptr()), glf._ptr(hc), C.byref(st2), glf._ptr(hm)) == glf.OK
        assert torch.equal(buf, lp) and st2.iterations == sp["iterations"]
        np.testing.assert_array_equal(hc, cp)
        np.testing.assert_array_equal(hm, sp["counts"].astype(np.float64))
        g.close()


# ---- 7. one driver behind both entry points ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["tiny", "ld64"])
def test_plain_embedding_through_segment_ex_is_segment(shape):
    """glf_graph_segment is the reference; glf_graph_segment_ex with emb NULL, and with an embed struct of normalize = 0 and no weight,
    gives the same labels, the same centroid bits, the same stats, and mass == counts -- seeded (the sample of rows and k-means++ are
    shared too) and from given centroids."""
    width, h, _, _, m, ld = SHAPES[shape]
    n, k, dim = width * h, min(m, 5), min(m, 64)
    size = C.sizeof(glf.ClusterEmbed)
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, shape)[0]
        given = _centroids(_phi(g, "cpu"), k, dim, None, 0, np.random.default_rng(17))
        for init, sample_rows in ((0, 4096), (0, 100), (1, 4096)):
            o = glf.SegmentOptions(C.sizeof(glf.SegmentOptions), k, dim, 50, sample_rows, init, 7, None)

            def run(entry, *emb):
                labels = torch.full((h, width), SENTINEL, dtype=torch.int32, device=ctx.device)
                cent, st, mass = given.copy(), glf.SegmentStats(), np.full(k, -1.0)
                torch.cuda.synchronize()
                rc = entry(g._g, C.byref(o), *emb, C.c_void_p(labels.data_ptr()), glf._ptr(cent), C.byref(st), *((glf._ptr(mass),) if emb else ()))
                assert rc == glf.OK, (shape, init, sample_rows)
                return labels, cent, (int(st.iterations), int(st.converged), int(st.changed_last), list(st.counts)), mass

            l0, c0, s0, _ = run(glf._lib.glf_graph_segment)
            assert s0[0] >= 1 and sum(s0[3]) == n and int(l0.min()) >= 0 and int(l0.max()) < k
            for emb in (None, C.byref(glf.ClusterEmbed(size, 0, None))):
                l1, c1, s1, m1 = run(glf._lib.glf_graph_segment_ex, emb)
                assert torch.equal(l1, l0) and s1 == s0, (shape, init, sample_rows)
                np.testing.assert_array_equal(_bits(c1), _bits(c0))
                np.testing.assert_array_equal(m1, np.asarray(s0[3][:k], dtype=np.float64))
        g.close()
