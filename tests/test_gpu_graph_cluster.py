"""Spectral segmentation on a graph handle: glf_graph_cluster_step (k_graph_cluster: one Lloyd iteration of k-means over the embedded
rows e(px) = scale o Phi[px][:dim] in one pass over Phi -- scores and argmin on v_mfma_f32_32x32x2_f32, the per-label sums on the same
instruction with the pixels as the contraction index), the driver glf_graph_segment and Graph.cluster_step / Graph.segment on top.

Shapes: those of tests/test_gpu_graph.py. 61 x 47 = 2867 pixels is a multiple neither of 32 nor of any chain length, so the last staged
tile and the last chain are partial, at ld 32 / 64 / 128 / 256 (ld >= 64: only the first CW = 64 columns are read); `tiny` is 160
pixels with m = 4: fewer tiles than two workgroups have waves. 509 x 515 has more tiles than a resident grid has waves.

All references are torch f64 on the handle's own Phi. With u = 2^-24:
  score_j(px) = |c_j|^2 - 2 sum_k phi_k scale_k c_jk
  E_j(px) = (CW + 4) u (|c_j|^2 + 2 sum_k |phi_k| |scale_k c_jk|)     one score's f32 error: the rounding of the operand and of the
                                                                       bias, a CW-term chain, the final fma (as _synth_want)
A pixel is decided when its best f64 score plus its E is below every other score minus that score's E. A decided pixel must carry the
f64 label; an undecided one a label whose f64 score is within E_best + E_label of the best. Condition on the inputs, asserted from the
f64 reference alone: at most 1 % of the pixels are undecided. One case of the list cannot meet it by construction and is checked more
strictly instead: dim = 1 under a scale that holds one 0 embeds every pixel and every centroid at 0, all scores are exactly 0 on both
sides, and the tie rule then requires label 0 everywhere.
Sums, given the kernel's own labels: |sums_j - sums64_j| <= ((CHAIN + 1) u + N 2^-52) sum_{px in j} |phi| column by column (exact
products, an f32 chain of CHAIN terms, the f64 tails of both sides); counts and changed are exact."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
from test_gpu_graph import SHAPES, _grey_graph, _opt  # noqa: E402

U = 2.0 ** -24
CHAIN = glf.GRAPH_NORMAL_CHAIN
KS = (1, 2, 5, 32)
SENTINEL = -77


def _cw(ld):
    return 32 if ld < 64 else 64


def _dims(m):
    return sorted({1, min(m, 64)} | ({7} if m >= 7 else set()))


def _scale(dim, rng):
    """A random scale in [0.5, 2) that holds one 0."""
    s = rng.uniform(0.5, 2.0, dim)
    s[rng.integers(0, dim)] = 0.0
    return s


def _centroids(phi, k, dim, scale, rng):
    """The embedded rows of k distinct random pixels, each entry times (1 + 0.1 N(0, 1)). phi: torch f64 [N, >= dim]."""
    px = rng.choice(phi.shape[0], size=k, replace=False)
    e = phi[torch.from_numpy(px).to(phi.device), :dim].cpu().numpy() * (np.ones(dim) if scale is None else scale)[None]
    return e * (1.0 + 0.1 * rng.normal(size=e.shape))


def _scores(phi, cent, scale, cw):
    """(score [N, k], E [N, k]) in f64 on phi's device."""
    k, dim = cent.shape
    s = np.ones(dim) if scale is None else scale
    a = torch.from_numpy(s[None] * cent).to(phi.device)
    c2 = torch.from_numpy((cent ** 2).sum(axis=1)).to(phi.device)
    p = phi[:, :dim]
    return c2[None] - 2.0 * (p @ a.T), (cw + 4) * U * (c2[None] + 2.0 * (p.abs() @ a.abs().T))


def _check_labels(lab, S, E, what, cap=True, over=None):
    """lab: int64 [N] on S's device. Returns the number of undecided pixels. over: a list that collects the cases whose inputs break
    the cap, for one assertion over all of them, instead of stopping at the first."""
    n, k = S.shape
    ar = torch.arange(n, device=S.device)
    assert int(lab.min()) >= 0 and int(lab.max()) < k, what
    best = S.argmin(dim=1)
    sb, eb = S[ar, best], E[ar, best]
    low = S - E
    low[ar, best] = float("inf")
    decided = sb + eb < low.min(dim=1).values
    und = int((~decided).sum())
    print("%s: %d of %d pixels undecided" % (what, und, n))
    if cap and over is not None and und > 0.01 * n:
        over.append((what, und))
    elif cap:
        assert und <= 0.01 * n, (what, und)                                       # the condition on the inputs
    assert bool((lab[decided] == best[decided]).all()), what
    gap = S[ar, lab] - sb
    assert bool((gap <= eb + E[ar, lab]).all()), (what, float((gap - eb - E[ar, lab]).max()))
    return und


def _check_sums(phi, lab, k, dim, sums, counts, what):
    """sums [k, dim] and counts [k] of a step against f64 on the labels the step wrote (lab: int64 [N] on phi's device)."""
    n = phi.shape[0]
    onehot = (lab[:, None] == torch.arange(k, device=phi.device)[None]).double()
    want = (onehot.T @ phi[:, :dim]).cpu().numpy()
    bound = ((CHAIN + 1) * U + n * 2.0 ** -52) * (onehot.T @ phi[:, :dim].abs()).cpu().numpy()
    bc = np.bincount(lab.cpu().numpy(), minlength=k)
    assert counts.dtype == np.uint64 and counts.shape == (k,) and sums.shape == (k, dim)
    np.testing.assert_array_equal(counts.astype(np.int64), bc, err_msg=what)
    assert int(counts.sum()) == n, what
    err = np.abs(sums - want)
    print("%s: max |sums - sums64| / bound %.3f" % (what, float((err / np.maximum(bound, 1e-300)).max())))
    assert np.all(err <= bound), what


def _phi(g, device=None):
    p = g.phi[:, :g.info["m"]].double()
    return p if device is None else p.to(device)


def _flat(labels):
    return labels.reshape(-1).long()


# ---- 1. labels against fp64 ---------------------------------------------------------------------------------------------------------

# The centroid seed. 101, the first one tried, broke the condition on the inputs from the f64 reference alone: of 32 one-dimensional
# centroids two lay so close that 75 of ld128's 2867 pixels (42 of ld32's) fell between them within E. As two centroids approach each
# other the undecided zone around their midpoint, E / |c_j - c_j'| wide, grows without bound, so with 32 centroids on a line a draw can
# exceed 1 %; 20 of the 30 seeds 101 .. 130 keep every case of every shape inside the cap, 103 is the first of them.
CENT_SEED = 103


def _label_case(phi, shape, k, dim, scaled):
    """(scale, centroids) of one case, from a random stream of its own."""
    rng = np.random.default_rng([CENT_SEED, list(SHAPES).index(shape), k, dim, scaled])
    scale = _scale(dim, rng) if scaled else None
    return scale, _centroids(phi, k, dim, scale, rng)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_labels_against_fp64(shape):
    m, ld = SHAPES[shape][4:]
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, shape)[0]
        phi = _phi(g, "cpu")
        over = []
        for k in KS:
            for dim in _dims(m):
                for scaled in (0, 1):
                    scale, cent = _label_case(phi, shape, k, dim, scaled)
                    labels, sums, counts, changed = g.cluster_step(cent, scale)
                    assert labels.dtype == torch.int32 and tuple(labels.shape) == (SHAPES[shape][1], SHAPES[shape][0]) and changed == 0
                    lab = _flat(labels).cpu()
                    S, E = _scores(phi, cent, scale, _cw(ld))
                    what = "%s k %d dim %d scale %s" % (shape, k, dim, "none" if scale is None else "random")
                    flat = scale is not None and dim == 1                         # the whole embedding is 0: all scores tie exactly
                    _check_labels(lab, S, E, what, cap=not flat, over=over)
                    if flat:
                        assert not S.any() and not lab.any(), what
        g.close()
    assert not over, over                                                         # the condition on the inputs: at most 1 % undecided


# ---- 2. sums, counts and changed, given the kernel's own labels --------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(SHAPES))
def test_sums_counts_and_changed(shape):
    width, h, _, _, m, ld = SHAPES[shape]
    n = width * h
    rng = np.random.default_rng(202)
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, shape)[0]
        phi = _phi(g, "cpu")
        for k in KS:
            for dim in _dims(m):
                scale = _scale(dim, rng) if (k + dim) % 2 else None
                cent = _centroids(phi, k, dim, scale, rng)
                what = "%s k %d dim %d" % (shape, k, dim)
                labels, sums, counts, changed = g.cluster_step(cent, scale)
                assert changed == 0                                               # no prev
                lab = _flat(labels).cpu()
                _check_sums(phi, lab, k, dim, sums, counts, what)
                prev = torch.from_numpy(rng.integers(0, k, size=(h, width)).astype(np.int32)).to(ctx.device)
                moved = int(np.count_nonzero(prev.cpu().numpy().reshape(-1) != lab.numpy()))
                l2, s2, c2, ch2 = g.cluster_step(cent, scale, prev=prev)          # a separate buffer
                assert ch2 == moved, what
                inplace = prev.clone()
                l3, s3, c3, ch3 = g.cluster_step(cent, scale, prev=inplace, labels=inplace)   # prev is labels
                assert l3 is inplace and ch3 == moved, what
                for l, s, c in ((l2, s2, c2), (l3, s3, c3)):
                    assert torch.equal(l, labels), what
                    np.testing.assert_array_equal(s.view(np.int64), sums.view(np.int64), err_msg=what)
                    np.testing.assert_array_equal(c, counts, err_msg=what)
                if k == 1:
                    assert moved == 0
        g.close()


# ---- 3. ties and edges --------------------------------------------------------------------------------------------------------------

def _raw_step(g, cent, scale, prev, labels, k=None, dim=None, sums=True, counts=True, changed=True):
    """glf_graph_cluster_step itself on device pointers (ints or None) -> (status, sums, counts, changed)."""
    kk, dd = (cent.shape if cent is not None else (2, 2))
    k, dim = kk if k is None else k, dd if dim is None else dim
    s, c, ch = np.zeros((max(k, 1), max(dim, 1))), np.zeros(max(k, 1), dtype=np.uint64), C.c_uint64(12345)
    torch.cuda.synchronize()
    rc = glf._lib.glf_graph_cluster_step(g._g, C.c_uint(k), C.c_uint(dim), glf._ptr(cent), glf._ptr(scale), prev, labels,
                                         glf._ptr(s) if sums else None, glf._ptr(c) if counts else None, C.byref(ch) if changed else None)
    return rc, s, c, int(ch.value)


@pytest.mark.parametrize("shape", ["ld32", "ld256", "tiny"])
def test_ties_and_edges(shape):
    width, h, _, _, m, ld = SHAPES[shape]
    n = width * h
    rng = np.random.default_rng(303)
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, shape)[0]
        phi = _phi(g, "cpu")
        dim = min(m, 64)
        # two identical centroids j < j': the higher index never wins
        for k, j, jj in ((2, 0, 1), (5, 1, 3), (32, 4, 31), (32, 30, 31)):
            cent = _centroids(phi, k, dim, None, rng)
            cent[jj] = cent[j]
            labels, sums, counts, _ = g.cluster_step(cent)
            lab = _flat(labels).cpu()
            assert not bool((lab == jj).any()) and counts[jj] == 0 and not sums[jj].any(), (shape, k, j, jj)
            _check_sums(phi, lab, k, dim, sums, counts, "%s twins %d %d of %d" % (shape, j, jj, k))
        # k = 1: every label is 0, the sums are the column sums of Phi
        cent = _centroids(phi, 1, dim, None, rng)
        labels, sums, counts, _ = g.cluster_step(cent)
        assert not bool(labels.any()) and counts.tolist() == [n]
        _check_sums(phi, _flat(labels).cpu(), 1, dim, sums, counts, "%s k 1" % shape)
        col = phi[:, :dim].sum(dim=0).numpy()
        assert np.all(np.abs(sums[0] - col) <= ((CHAIN + 1) * U + n * 2.0 ** -52) * phi[:, :dim].abs().sum(dim=0).numpy())
        # a label buffer of N + 64 ints keeps its tail
        cent = _centroids(phi, 5, dim, None, rng)
        buf = torch.full((n + 64,), SENTINEL, dtype=torch.int32, device=ctx.device)
        rc, sums, counts, _ = _raw_step(g, cent, None, None, C.c_void_p(buf.data_ptr()))
        assert rc == glf.OK
        assert bool((buf[n:] == SENTINEL).all()) and int(buf[:n].min()) >= 0 and int(buf[:n].max()) < 5
        assert torch.equal(buf[:n].reshape(h, width), g.cluster_step(cent)[0])
        g.close()


# ---- 4. independence and repeatability ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["ld32", "ld64", "ld256"])
def test_repeatable_and_independent_of_a_far_centroid(shape):
    m, ld = SHAPES[shape][4:]
    rng = np.random.default_rng(404)
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, shape)[0]
        phi = _phi(g, "cpu")
        dim = min(m, 64)
        scale = _scale(dim, rng)
        far = np.zeros(dim)
        live = int(np.flatnonzero(scale)[0])
        far[live] = 1e3 * float((phi[:, :dim] * torch.from_numpy(scale)[None]).norm(dim=1).max())   # 1e3 times farther than any row
        for k in (1, 5, 31):
            cent = _centroids(phi, k, dim, scale, rng)
            l1, s1, c1, _ = g.cluster_step(cent, scale)
            l2, s2, c2, _ = g.cluster_step(cent, scale)
            assert torch.equal(l1, l2)
            np.testing.assert_array_equal(s1.view(np.int64), s2.view(np.int64))
            np.testing.assert_array_equal(c1, c2)
            l3, s3, c3, _ = g.cluster_step(np.concatenate([cent, far[None]]), scale)
            assert torch.equal(l1, l3), (shape, k)
            np.testing.assert_array_equal(s3[:k].view(np.int64), s1.view(np.int64))
            np.testing.assert_array_equal(c3[:k], c1)
            assert c3[k] == 0 and not s3[k].any()
        g.close()


# ---- 5. the grid-strided loop -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,ld", [(8, 32), (200, 256)])
def test_cluster_step_many_tiles_per_wave(m, ld):
    """509 x 515 = 8191 tiles of 32 pixels and one of 23, more than a resident grid has waves (at most 4 waves x 7 workgroups a CU at
    the smallest LDS footprint of the project's kernels; this one holds 39 to 45 KB a workgroup, so fewer): every wave runs its tile
    loop several times, whole chains are flushed into f64 and the next tile's loads fly under the MFMAs. At ld 256 only 64 of the 256
    columns are read. Reference and the checks of 1 and 2 in torch f64 on the device."""
    width, h = 509, 515
    n = width * h
    rng = np.random.default_rng(ld)
    with glf.Context(0) as ctx:
        assert (n + 31) // 32 > 4 * 7 * ctx.device_info()["num_cus"]
        assert glf.Sampling(width, h, 300).size == 324
        g = ctx.graph(ctx.to_device(glf.synth_image(width, h, seed=3)), glf.default_options(num_samples=300, num_eigvals=m, epsilon=0.1))
        assert (g.info["p"], g.info["m"], g.info["ld"]) == (324, m, ld)
        phi = _phi(g)
        k, dim = 32, min(m, 64)
        for scale in (None, _scale(dim, rng)):
            cent = _centroids(phi, k, dim, scale, rng)
            what = "509 x 515 ld %d scale %s" % (ld, "none" if scale is None else "random")
            prev = torch.from_numpy(rng.integers(0, k, size=(h, width)).astype(np.int32)).to(ctx.device)
            labels, sums, counts, changed = g.cluster_step(cent, scale, prev=prev)
            lab = _flat(labels)
            S, E = _scores(phi, cent, scale, _cw(ld))
            _check_labels(lab, S, E, what)
            _check_sums(phi, lab, k, dim, sums, counts, what)
            assert changed == int((prev != labels).sum()), what
        g.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_labels_untouched():
    width, h, _, _, m, ld = SHAPES["ld32"]
    n = width * h
    rng = np.random.default_rng(606)
    lib = glf._lib
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, "ld32")[0]
        phi = _phi(g, "cpu")
        cent = _centroids(phi, 5, m, None, rng)
        buf = torch.full((n,), SENTINEL, dtype=torch.int32, device=ctx.device)
        L = C.c_void_p(buf.data_ptr())

        def bad(x, v):
            y = np.array(x, dtype=np.float64)
            y.reshape(-1)[3] = v
            return y

        ones = np.ones(m)
        cases = {
            "cent NULL": dict(cent=None, k=5, dim=m), "labels NULL": dict(labels=None), "sums NULL": dict(sums=False),
            "counts NULL": dict(counts=False), "changed NULL": dict(changed=False), "k = 0": dict(k=0), "k = 33": dict(cent=np.zeros((33, m))),
            "dim = 0": dict(dim=0), "dim = m + 1": dict(cent=np.zeros((5, m + 1))), "dim = 65": dict(cent=np.zeros((5, 65))),
            "NaN centroid": dict(cent=bad(cent, np.nan)), "Inf centroid": dict(cent=bad(cent, np.inf)),
            "-Inf centroid": dict(cent=bad(cent, -np.inf)), "NaN scale": dict(scale=bad(ones, np.nan)), "Inf scale": dict(scale=bad(ones, np.inf)),
        }
        for what, kw in cases.items():
            args = dict(cent=cent, scale=None, prev=None, labels=L)
            args.update(kw)
            rc = _raw_step(g, args.pop("cent"), args.pop("scale"), args.pop("prev"), args.pop("labels"), **args)[0]
            assert rc == glf.ERR_INVALID, what
            assert bool((buf == SENTINEL).all()), what
        rc = lib.glf_graph_cluster_step(None, C.c_uint(5), C.c_uint(m), glf._ptr(cent), None, None, L, glf._ptr(np.zeros((5, m))),
                                        glf._ptr(np.zeros(5, dtype=np.uint64)), C.byref(C.c_uint64()))
        assert rc == glf.ERR_INVALID                                              # a NULL handle
        # the driver
        h_cent = np.ascontiguousarray(cent[:2, :2])
        st = glf.SegmentStats()

        def seg(k=2, dim=2, init=1, size=C.sizeof(glf.SegmentOptions), scale=None, handle=g._g, labels=L, c=h_cent, opt=True):
            o = glf.SegmentOptions(size, k, dim, 50, 4096, init, 1, scale.ctypes.data if scale is not None else None)
            torch.cuda.synchronize()
            return lib.glf_graph_segment(handle, C.byref(o) if opt else None, labels, glf._ptr(c), C.byref(st))

        for what, kw in {"struct_size + 8": dict(size=C.sizeof(glf.SegmentOptions) + 8), "struct_size 0": dict(size=0), "k = 0": dict(k=0),
                         "k = 33": dict(k=33), "dim = 0": dict(dim=0), "dim = m + 1": dict(dim=m + 1), "init = 2": dict(init=2),
                         "init = -1": dict(init=-1), "NaN centroid": dict(c=np.array([[np.nan, 1.0], [2.0, 3.0]])),
                         "Inf centroid": dict(c=np.array([[0.0, 1.0], [2.0, np.inf]])), "NaN scale": dict(scale=np.array([1.0, np.nan])),
                         "opt NULL": dict(opt=False), "labels NULL": dict(labels=None), "cent NULL": dict(c=None), "handle NULL": dict(handle=None)}.items():
            assert seg(**kw) == glf.ERR_INVALID, what
            assert bool((buf == SENTINEL).all()), what
        with pytest.raises(glf.GlfError) as e:
            g.segment(33)
        assert e.value.status == glf.ERR_INVALID
        with pytest.raises(glf.GlfError):
            g.cluster_step(np.zeros((2, m + 1)))
        with pytest.raises(ValueError):
            g.cluster_step(cent, prev=torch.zeros((h, width + 1), dtype=torch.int32, device=ctx.device))
        with pytest.raises(ValueError):
            g.cluster_step(cent, scale=np.ones(m + 1))
        with pytest.raises(AssertionError):
            g.cluster_step(cent, labels=torch.zeros((h, width), dtype=torch.int64, device=ctx.device))
        with pytest.raises(ValueError):
            g.segment(2, init=np.zeros((3, 2)))
        # nothing faulted: the next valid calls succeed, and a seeded init is not read for finiteness
        assert seg(init=0, c=np.full((2, 2), np.nan)) == glf.OK and st.iterations >= 1
        labels = g.cluster_step(cent)[0]
        assert int(labels.min()) >= 0 and int(labels.max()) < 5
        g.close()


# ---- 7. the driver --------------------------------------------------------------------------------------------------------------------

TWO_TONE_SEED = 3


def _two_tone(seed):
    """61 x 47: the left half of synth_image scaled around 60, the right half around 190 (contrast 0.2, so +-18 grey levels)."""
    w, h = SHAPES["ld32"][:2]
    img = glf.synth_image(w, h, seed=seed).astype(np.float64)
    tone = np.where(np.arange(w) < w // 2, 60.0, 190.0)[None]
    return np.clip(np.rint(tone + 0.2 * (img - 127.5)), 0, 255).astype(np.uint8)


def _python_lloyd(g, c0, max_iter=50):
    """The driver restated on cluster_step + glf.cluster_update."""
    labels, sums, counts, changed = g.cluster_step(c0)
    cent, it, converged = glf.cluster_update(sums, counts, None, c0), 1, 0
    while it < max_iter and not converged:
        labels, sums, counts, changed = g.cluster_step(cent, prev=labels, labels=labels)
        converged = int(changed == 0)
        it += 1
        cent = glf.cluster_update(sums, counts, None, cent)
    return labels, cent, it, converged, changed, counts


def test_segment_driver():
    """dim = m = 8: at epsilon = 0.1 the eigensolver stops long before the single vectors have settled, only the span of the m
    columns carries the two halves (on all 8 columns Lloyd's iteration finds them; on the first 2 it splits off a dozen outliers).
    (c)'s input condition -- no pixel of any iteration of the f64 Lloyd run is undecided -- holds for the two-tone image of
    TWO_TONE_SEED = 3: 4 iterations, the closest pixel 3000 E away from a tie (on the handle's own Phi; seeds 0 .. 11 all hold it, the
    closest at 37 E). It is asserted below, so a seed that breaks it shows as such."""
    w, h = SHAPES["ld32"][:2]
    n, k, dim = w * h, 2, 8
    with glf.Context(0) as ctx:
        g = ctx.graph(ctx.to_device(_two_tone(TWO_TONE_SEED)), _opt("ld32"))
        phi = _phi(g, "cpu")
        pick = [(h // 2) * w + w // 4, (h // 2) * w + (3 * w) // 4]               # one pixel per half
        c0 = phi[pick, :dim].numpy().copy()
        # (a) the driver is the loop
        labels, cent, st = g.segment(k, dim, init=c0)
        pl, pc, pit, pconv, pchanged, pcounts = _python_lloyd(g, c0)
        assert st["iterations"] == pit and st["converged"] == pconv == 1 and st["changed_last"] == pchanged == 0
        assert torch.equal(labels, pl)
        np.testing.assert_array_equal(st["counts"], pcounts)
        assert float(np.abs(cent - pc).max()) <= 1e-12 * float(np.abs(pc).max())
        assert labels.dtype == torch.int32 and tuple(labels.shape) == (h, w) and st["counts"].sum() == n
        # (b) a fixed point: one more step moves nothing
        l2, _, _, moved = g.cluster_step(cent, prev=labels)
        assert moved == 0 and torch.equal(l2, labels)
        # (c) the same number of f64 Lloyd iterations in torch
        c64, lab64 = c0.copy(), None
        for it in range(st["iterations"]):
            S, E = _scores(phi, c64, None, 32)
            lab64 = S.argmin(dim=1)
            assert _check_labels(lab64, S, E, "f64 Lloyd iteration %d" % it) == 0   # the input condition: nobody undecided
            for j in range(k):
                if bool((lab64 == j).any()):
                    c64[j] = phi[lab64 == j, :dim].mean(dim=0).numpy()
        assert torch.equal(_flat(labels).cpu(), lab64)
        left = (torch.arange(n) % w < w // 2)
        agree = float(((lab64 == 0) == left).double().mean())
        print("two-tone seed %d: %d iterations, agreement with the two halves %.4f" % (TWO_TONE_SEED, st["iterations"], max(agree, 1.0 - agree)))
        # (d) seeding: reproducible, and the documented rule
        for sample_rows in (4096, 500):
            la, ca, sa = g.segment(k, dim, seed=7, sample_rows=sample_rows)
            lb, cb, sb = g.segment(k, dim, seed=7, sample_rows=sample_rows)
            assert torch.equal(la, lb) and sa["iterations"] == sb["iterations"]
            np.testing.assert_array_equal(ca, cb)
            ns = min(sample_rows, n)
            rows = phi[[(i * n) // ns for i in range(ns)], :dim].numpy()
            lc, cc, sc = g.segment(k, dim, init=glf.cluster_seed(rows, k, seed=7))
            assert torch.equal(la, lc) and sa["iterations"] == sc["iterations"]
            np.testing.assert_array_equal(ca, cc)
        # (e) one step only
        l1, c1, s1 = g.segment(k, dim, init=c0, max_iter=1)
        assert s1["converged"] == 0 and s1["iterations"] == 1 and s1["changed_last"] == 0
        first = g.cluster_step(c0)
        assert torch.equal(l1, first[0])
        np.testing.assert_array_equal(c1, glf.cluster_update(first[1], first[2], None, c0))
        # a scale and the default dim through the driver: dim = max(k, 2) columns, one of them dropped
        l5, c5, s5 = g.segment(3, scale=np.array([1.0, 0.0, 2.0]), seed=2)
        assert c5.shape == (3, 3) and not c5[:, 1].any() and int(l5.max()) < 3 and s5["counts"].sum() == n
        g.close()
