"""The C-ABI of the spectral segmentation under unit-length rows and per-pixel weights (glf_graph_cluster_step_ex,
glf_cluster_update_w, glf_cluster_seed_w, glf_graph_segment_ex): exported by libglf.so, declared in include/glf.h, listed in
glf.EXPORTS; glf_cluster_embed's layout against the ctypes mirror; without a handle the two device calls answer GLF_ERR_INVALID before
any device work; and the two host-only functions against numpy restatements. CPU only.

glf_cluster_update_w is one multiplication and one division per entry: the comparison with numpy's (scale * sums) / mass is exact.
glf_cluster_seed_w runs on small integer lattice points under small integer weights, so that every weighted squared distance and every
running sum is an exact integer in f64 and the comparison with the restatement, which draws its uniforms from
glf.random_vectors(k, 1, seed), is exact too; doubling every weight doubles every sum exactly and must choose the same rows."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("glf_graph_cluster_step_ex", "glf_cluster_update_w", "glf_cluster_seed_w", "glf_graph_segment_ex")


def test_nw_entry_points_are_exported_and_declared():
    lib = C.CDLL(glf.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in glf.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"typedef\s+struct\s+glf_cluster_embed\s*\{", header)
    assert callable(glf.cluster_update_w) and callable(glf.cluster_seed_w)
    assert hasattr(glf.Graph, "cluster_step_ex")


def test_embed_layout_matches_the_header(tmp_path):
    names = [f[0] for f in glf.ClusterEmbed._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "glf.h"', "int main(void) {", 'printf("%zu", sizeof(glf_cluster_embed));']
    lines += ['printf(" %%zu", offsetof(glf_cluster_embed, %s));' % n for n in names]
    lines += ['printf("\\n");', "return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(glf.ClusterEmbed)] + [getattr(glf.ClusterEmbed, n).offset for n in names]


def test_device_calls_without_a_handle_are_invalid():
    lib = C.CDLL(glf.LIB_PATH)
    one = C.c_void_p(1)
    buf = (C.c_double * 64)()
    cnt = (C.c_uint64 * 32)()
    mass = (C.c_double * 32)()
    changed = C.c_uint64(7)
    emb = glf.ClusterEmbed(C.sizeof(glf.ClusterEmbed), 1, None)
    for e in (None, C.byref(emb)):
        for k, dim in ((2, 2), (0, 2), (33, 2), (2, 0), (2, 65)):
            assert lib.glf_graph_cluster_step_ex(None, e, C.c_uint(k), C.c_uint(dim), buf, None, None, one, buf, cnt, mass,
                                                 C.byref(changed)) == glf.ERR_INVALID
        assert lib.glf_graph_cluster_step_ex(None, e, C.c_uint(2), C.c_uint(2), None, None, None, None, None, None, None, None) == glf.ERR_INVALID
        opt = glf.SegmentOptions(C.sizeof(glf.SegmentOptions), 2, 2, 50, 4096, 0, 1, None)
        st = glf.SegmentStats()
        assert lib.glf_graph_segment_ex(None, C.byref(opt), e, one, buf, C.byref(st), mass) == glf.ERR_INVALID
        assert lib.glf_graph_segment_ex(None, None, e, None, None, None, None) == glf.ERR_INVALID
    assert changed.value == 7 and not any(mass)


# ---- glf_cluster_update_w ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,dim", [(1, 1), (2, 7), (5, 64), (32, 32)])
@pytest.mark.parametrize("with_scale", [False, True])
def test_cluster_update_w_against_numpy(k, dim, with_scale):
    rng = np.random.default_rng(10 * k + dim)
    sums = rng.normal(size=(k, dim)) * 1e3
    mass = rng.uniform(0.01, 5000.0, k)
    prev = rng.normal(size=(k, dim))
    empty = [] if k == 1 else [k // 2, k - 1]
    mass[empty] = 0.0
    scale = None
    if with_scale:
        scale = rng.uniform(0.5, 2.0, dim)
        scale[dim // 2] = 0.0
    cent = glf.cluster_update_w(sums, mass, scale, prev)
    want = prev.copy()
    live = mass > 0
    want[live] = ((np.ones(dim) if scale is None else scale)[None] * sums[live]) / mass[live][:, None]
    np.testing.assert_array_equal(cent, want)
    np.testing.assert_array_equal(cent[empty], prev[empty])                      # a cluster of mass 0 keeps its centroid
    if not empty:
        np.testing.assert_array_equal(glf.cluster_update_w(sums, mass, scale), want)   # (no cent_prev needed)
    # integer masses: the bits of glf_cluster_update on the same counts
    counts = rng.integers(1, 5000, k).astype(np.uint64)
    counts[empty] = 0
    np.testing.assert_array_equal(glf.cluster_update_w(sums, counts.astype(np.float64), scale, prev), glf.cluster_update(sums, counts, scale, prev))


def test_cluster_update_w_empty_means_not_positive():
    sums, prev = np.ones((4, 2)), np.full((4, 2), 9.0)
    cent = glf.cluster_update_w(sums, np.array([2.0, -1.0, np.nan, 0.0]), None, prev)
    np.testing.assert_array_equal(cent, [[0.5, 0.5], [9.0, 9.0], [9.0, 9.0], [9.0, 9.0]])


def test_cluster_update_w_refusals_leave_cent_untouched():
    k, dim = 3, 2
    sums, mass, prev = np.ones((k, dim)), np.array([2.0, 0.0, 3.0]), np.zeros((k, dim))
    fill = np.full((k, dim), 12345.0)

    def raw(kk, dd, s, c, p, out):
        return glf._lib.glf_cluster_update_w(C.c_uint(kk), C.c_uint(dd), None, glf._ptr(s), glf._ptr(c), glf._ptr(p), glf._ptr(out))

    cases = {"k = 0": (0, dim, sums, mass, prev), "dim = 0": (k, 0, sums, mass, prev), "sums NULL": (k, dim, None, mass, prev),
             "mass NULL": (k, dim, sums, None, prev), "mass 0, no cent_prev": (k, dim, sums, mass, None),
             "mass NaN, no cent_prev": (k, dim, sums, np.array([2.0, np.nan, 3.0]), None),
             "mass < 0, no cent_prev": (k, dim, sums, np.array([2.0, -1.0, 3.0]), None)}
    for what, (kk, dd, s, c, p) in cases.items():
        out = fill.copy()
        assert raw(kk, dd, s, c, p, out) == glf.ERR_INVALID, what
        np.testing.assert_array_equal(out, fill, err_msg=what)
    assert raw(k, dim, sums, mass, prev, None) == glf.ERR_INVALID
    out = prev.copy()                                                            # in place: cent is cent_prev
    assert raw(k, dim, sums, mass, out, out) == glf.OK
    np.testing.assert_array_equal(out, [[0.5, 0.5], [0.0, 0.0], [1.0 / 3.0, 1.0 / 3.0]])
    with pytest.raises(glf.GlfError) as e:
        glf.cluster_update_w(sums, mass)
    assert e.value.status == glf.ERR_INVALID
    with pytest.raises(ValueError):
        glf.cluster_update_w(sums, mass[:2], None, prev)
    with pytest.raises(ValueError):
        glf.cluster_update_w(sums, mass, np.ones(dim + 1), prev)


# ---- glf_cluster_seed_w ------------------------------------------------------------------------------------------------------------

def _seed_rule_w(rows, w, k, seed):
    """The documented rule in numpy: the indices of the k rows chosen, or None when a total is 0."""
    n = rows.shape[0]
    u = glf.random_vectors(k, 1, seed).reshape(-1)
    run = np.cumsum(w)                                                            # (sequential, and exact on small integers)
    if run[-1] == 0:
        return None
    pick = [int(np.argmax(run > u[0] * run[-1]))]
    d2 = np.full(n, np.inf)
    for t in range(1, k):
        d2 = np.minimum(d2, ((rows - rows[pick[-1]]) ** 2).sum(axis=1))
        run = np.cumsum(w * d2)
        if run[-1] == 0:
            return None
        pick.append(int(np.argmax(run > u[t] * run[-1])))
    return pick


def _lattice(n, dim, seed):
    rng = np.random.default_rng(seed)
    rows = rng.integers(-8, 9, size=(n, dim)).astype(np.float64)
    rows[:, 0] = 32.0 * rng.permutation(n)                                        # (no two rows alike)
    return rows, rng.integers(0, 5, size=n).astype(np.float64)                    # weights 0 .. 4, about a fifth of them 0


@pytest.mark.parametrize("n,dim,k", [(1, 3, 1), (40, 2, 1), (40, 2, 5), (40, 7, 20), (300, 64, 32), (4096, 8, 8)])
@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_cluster_seed_w_against_the_rule(n, dim, k, seed):
    rows, w = _lattice(n, dim, 1000 * n + k)
    w[0] = max(w[0], 1.0)
    assert np.count_nonzero(w) >= k
    pick = _seed_rule_w(rows, w, k, seed)
    cent = glf.cluster_seed_w(rows, w, k, seed)
    assert cent.shape == (k, dim)
    np.testing.assert_array_equal(cent, rows[pick])
    assert len(set(pick)) == k and np.all(w[pick] > 0)                            # k distinct rows, none of weight 0
    np.testing.assert_array_equal(glf.cluster_seed_w(rows, 2.0 * w, k, seed), cent)   # weights x 2: the same seeds
    np.testing.assert_array_equal(glf.cluster_seed_w(rows, 0.5 * w, k, seed), cent)
    # w NULL is glf_cluster_seed bit for bit
    np.testing.assert_array_equal(glf.cluster_seed_w(rows, None, k, seed), glf.cluster_seed(rows, k, seed))


def test_cluster_seed_w_first_centre_follows_the_weights():
    rows = np.arange(8, dtype=np.float64)[:, None]
    w = np.zeros(8)
    w[5] = 3.0
    for seed in range(8):
        np.testing.assert_array_equal(glf.cluster_seed_w(rows, w, 1, seed), [[5.0]])
    w[2] = 1.0
    for seed in range(8):
        u0 = glf.random_vectors(1, 1, seed).reshape(-1)[0]
        np.testing.assert_array_equal(glf.cluster_seed_w(rows, w, 1, seed), [[2.0 if 1.0 > u0 * 4.0 else 5.0]])
        assert sorted(glf.cluster_seed_w(rows, w, 2, seed).reshape(-1).tolist()) == [2.0, 5.0]


def test_cluster_seed_w_refusals_leave_cent_untouched():
    rows, _ = _lattice(6, 2, 1)
    w = np.array([1.0, 0.0, 2.0, 0.0, 0.0, 1.0])
    fill = np.full((8, 2), 12345.0)

    def raw(r, ww, n, dim, k, out):
        return glf._lib.glf_cluster_seed_w(glf._ptr(r), glf._ptr(ww), C.c_size_t(n), C.c_uint(dim), C.c_uint(k), C.c_uint64(1), glf._ptr(out))

    def bad(v):
        y = w.copy()
        y[3] = v
        return y

    with_nan = rows.copy()
    with_nan[2, 1] = np.nan
    dup = np.repeat(rows[:2], 3, axis=0)
    cases = {"rows NULL": (None, w, 6, 2, 2), "n = 0": (rows, w, 0, 2, 1), "dim = 0": (rows, w, 6, 0, 2), "k = 0": (rows, w, 6, 2, 0),
             "k > n": (rows, w, 6, 2, 7), "NaN row": (with_nan, w, 6, 2, 2), "duplicates": (dup, np.ones(6), 6, 2, 3),
             "k > rows of positive weight": (rows, w, 6, 2, 4), "negative weight": (rows, bad(-1.0), 6, 2, 2),
             "NaN weight": (rows, bad(np.nan), 6, 2, 2), "Inf weight": (rows, bad(np.inf), 6, 2, 2), "total 0": (rows, np.zeros(6), 6, 2, 1),
             "rows NULL, w NULL": (None, None, 6, 2, 2), "k > n, w NULL": (rows, None, 6, 2, 7)}
    for what, (r, ww, n, dim, k) in cases.items():
        out = fill.copy()
        assert raw(r, ww, n, dim, k, out) == glf.ERR_INVALID, what
        np.testing.assert_array_equal(out, fill, err_msg=what)
    assert raw(rows, w, 6, 2, 2, None) == glf.ERR_INVALID
    out = fill.copy()
    assert raw(rows, w, 6, 2, 3, out) == glf.OK                                   # every row of positive weight, once
    assert sorted(map(tuple, out[:3])) == sorted(map(tuple, rows[w > 0]))
    np.testing.assert_array_equal(out[3:], fill[3:])
    with pytest.raises(ValueError):
        glf.cluster_seed_w(np.zeros(5), None, 2)
    with pytest.raises(ValueError):
        glf.cluster_seed_w(rows, np.ones(5), 2)
    with pytest.raises(glf.GlfError) as e:
        glf.cluster_seed_w(rows, np.zeros(6), 1)
    assert e.value.status == glf.ERR_INVALID
