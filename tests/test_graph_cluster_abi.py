"""The spectral segmentation's C-ABI (glf_graph_cluster_step, glf_cluster_update, glf_cluster_seed, glf_graph_segment): exported by
libglf.so, declared in include/glf.h, listed in glf.EXPORTS; without a handle the two device calls answer GLF_ERR_INVALID before any
device work; and the two host-only functions against numpy restatements. CPU only.

glf_cluster_update is one multiplication and one division per entry: the comparison with numpy's (scale * sums) / counts is exact.
glf_cluster_seed runs on small integer lattice points, so that every squared distance and every running sum is an exact integer in
f64 and the comparison with the restatement, which draws its uniforms from glf.random_vectors(k, 1, seed), is exact too."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("glf_graph_cluster_step", "glf_cluster_update", "glf_cluster_seed", "glf_graph_segment")


def test_cluster_entry_points_are_exported_and_declared():
    lib = C.CDLL(glf.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in glf.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    cmax = re.search(r"#define\s+GLF_CLUSTER_MAX\s+(\d+)\b", header)
    assert cmax and int(cmax.group(1)) == glf.CLUSTER_MAX == 32
    for struct in ("glf_segment_options", "glf_segment_stats"):
        assert re.search(r"typedef\s+struct\s+%s\s*\{" % struct, header), struct
    assert callable(glf.cluster_update) and callable(glf.cluster_seed)
    for method in ("cluster_step", "segment"):
        assert hasattr(glf.Graph, method), method


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof and every offsetof of the two structs, as a C compiler lays out include/glf.h, against the ctypes mirrors."""
    fields = {"glf_segment_options": [f[0] for f in glf.SegmentOptions._fields_], "glf_segment_stats": [f[0] for f in glf.SegmentStats._fields_]}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "glf.h"', "int main(void) {"]
    for struct, names in fields.items():
        lines.append('printf("%%zu", sizeof(%s));' % struct)
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (struct, n) for n in names]
        lines.append('printf("\\n");')
    lines += ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)]).decode().split("\n")
    for line, mirror in zip(out, (glf.SegmentOptions, glf.SegmentStats)):
        got = [int(x) for x in line.split()]
        assert got == [C.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_], mirror.__name__
    assert C.sizeof(glf.SegmentStats) == 16 + 8 * glf.CLUSTER_MAX


def test_device_calls_without_a_handle_are_invalid():
    lib = C.CDLL(glf.LIB_PATH)
    one = C.c_void_p(1)
    buf = (C.c_double * 64)()
    cnt = (C.c_uint64 * 32)()
    changed = C.c_uint64(7)
    for k, dim in ((2, 2), (0, 2), (33, 2), (2, 0), (2, 65)):
        assert lib.glf_graph_cluster_step(None, C.c_uint(k), C.c_uint(dim), buf, None, None, one, buf, cnt, C.byref(changed)) == glf.ERR_INVALID
        assert lib.glf_graph_cluster_step(None, C.c_uint(k), C.c_uint(dim), None, None, None, None, None, None, None) == glf.ERR_INVALID
    opt = glf.SegmentOptions(C.sizeof(glf.SegmentOptions), 2, 2, 50, 4096, 0, 1, None)
    st = glf.SegmentStats()
    assert lib.glf_graph_segment(None, C.byref(opt), one, buf, C.byref(st)) == glf.ERR_INVALID
    assert lib.glf_graph_segment(None, None, None, None, None) == glf.ERR_INVALID
    assert changed.value == 7


# ---- glf_cluster_update ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,dim", [(1, 1), (2, 7), (5, 64), (32, 32)])
@pytest.mark.parametrize("with_scale", [False, True])
def test_cluster_update_against_numpy(k, dim, with_scale):
    rng = np.random.default_rng(10 * k + dim)
    sums = rng.normal(size=(k, dim)) * 1e3
    counts = rng.integers(1, 5000, k).astype(np.uint64)
    prev = rng.normal(size=(k, dim))
    empty = [] if k == 1 else [k // 2, k - 1]
    counts[empty] = 0
    scale = None
    if with_scale:
        scale = rng.uniform(0.5, 2.0, dim)
        scale[dim // 2] = 0.0
    cent = glf.cluster_update(sums, counts, scale, prev)
    want = prev.copy()
    live = counts > 0
    want[live] = ((np.ones(dim) if scale is None else scale)[None] * sums[live]) / counts[live].astype(np.float64)[:, None]
    np.testing.assert_array_equal(cent, want)
    np.testing.assert_array_equal(cent[empty], prev[empty])                      # an empty cluster keeps its centroid
    if not empty:
        np.testing.assert_array_equal(glf.cluster_update(sums, counts, scale), want)   # (no cent_prev needed)


def test_cluster_update_refusals_leave_cent_untouched():
    k, dim = 3, 2
    sums, counts, prev = np.ones((k, dim)), np.array([2, 0, 3], dtype=np.uint64), np.zeros((k, dim))
    fill = np.full((k, dim), 12345.0)

    def raw(kk, dd, s, c, p, out):
        return glf._lib.glf_cluster_update(C.c_uint(kk), C.c_uint(dd), None, glf._ptr(s), glf._ptr(c), glf._ptr(p), glf._ptr(out))

    cases = {"k = 0": (0, dim, sums, counts, prev), "dim = 0": (k, 0, sums, counts, prev), "sums NULL": (k, dim, None, counts, prev),
             "counts NULL": (k, dim, sums, None, prev), "empty cluster, no cent_prev": (k, dim, sums, counts, None)}
    for what, (kk, dd, s, c, p) in cases.items():
        out = fill.copy()
        assert raw(kk, dd, s, c, p, out) == glf.ERR_INVALID, what
        np.testing.assert_array_equal(out, fill, err_msg=what)
    assert raw(k, dim, sums, counts, prev, None) == glf.ERR_INVALID
    out = prev.copy()                                                            # in place: cent is cent_prev
    assert raw(k, dim, sums, counts, out, out) == glf.OK
    np.testing.assert_array_equal(out, [[0.5, 0.5], [0.0, 0.0], [1.0 / 3.0, 1.0 / 3.0]])
    with pytest.raises(glf.GlfError) as e:
        glf.cluster_update(sums, counts)
    assert e.value.status == glf.ERR_INVALID
    with pytest.raises(ValueError):
        glf.cluster_update(sums, counts[:2], None, prev)
    with pytest.raises(ValueError):
        glf.cluster_update(sums, counts, np.ones(dim + 1), prev)


# ---- glf_cluster_seed --------------------------------------------------------------------------------------------------------------

def _seed_rule(rows, k, seed):
    """The documented rule in numpy: the indices of the k rows chosen, or None when a total is 0."""
    n = rows.shape[0]
    u = glf.random_vectors(k, 1, seed).reshape(-1)
    pick = [int(np.floor(u[0] * n))]
    d2 = np.full(n, np.inf)
    for t in range(1, k):
        d2 = np.minimum(d2, ((rows - rows[pick[-1]]) ** 2).sum(axis=1))
        run = np.cumsum(d2)                                                       # (sequential, and exact on the lattice)
        if run[-1] == 0:
            return None
        pick.append(int(np.argmax(run > u[t] * run[-1])))
    return pick


def _lattice(n, dim, seed, distinct=True):
    rng = np.random.default_rng(seed)
    rows = rng.integers(-8, 9, size=(n, dim)).astype(np.float64)
    if distinct:
        rows[:, 0] = 32.0 * rng.permutation(n)                                    # (no two rows alike)
    return rows


@pytest.mark.parametrize("n,dim,k", [(1, 3, 1), (5, 1, 5), (40, 2, 1), (40, 2, 5), (40, 7, 40), (300, 64, 32), (4096, 8, 8)])
@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_cluster_seed_against_the_rule(n, dim, k, seed):
    rows = _lattice(n, dim, 1000 * n + k)
    pick = _seed_rule(rows, k, seed)
    cent = glf.cluster_seed(rows, k, seed)
    assert cent.shape == (k, dim)
    np.testing.assert_array_equal(cent, rows[pick])
    assert len(set(pick)) == k                                                    # k distinct rows: a chosen row has D^2 = 0


def test_cluster_seed_on_duplicate_rows():
    base = _lattice(6, 3, 5)
    rows = np.repeat(base, 4, axis=0)[np.random.default_rng(2).permutation(24)]   # 24 rows, 6 distinct
    for seed in (1, 2, 3):
        for k in (1, 2, 6):
            pick = _seed_rule(rows, k, seed)
            cent = glf.cluster_seed(rows, k, seed)
            np.testing.assert_array_equal(cent, rows[pick])
            assert np.unique(cent, axis=0).shape[0] == k
        assert _seed_rule(rows, 7, seed) is None
        with pytest.raises(glf.GlfError) as e:                                    # fewer than k distinct rows
            glf.cluster_seed(rows, 7, seed)
        assert e.value.status == glf.ERR_INVALID
    same = np.ones((5, 2))
    np.testing.assert_array_equal(glf.cluster_seed(same, 1, 9), same[:1])
    with pytest.raises(glf.GlfError):
        glf.cluster_seed(same, 2, 9)


def test_cluster_seed_refusals_leave_cent_untouched():
    rows = _lattice(6, 2, 1)
    fill = np.full((8, 2), 12345.0)

    def raw(r, n, dim, k, out):
        return glf._lib.glf_cluster_seed(glf._ptr(r), C.c_size_t(n), C.c_uint(dim), C.c_uint(k), C.c_uint64(1), glf._ptr(out))

    with_nan = rows.copy()
    with_nan[3, 1] = np.nan
    dup = np.repeat(rows[:2], 3, axis=0)
    for what, (r, n, dim, k) in {"rows NULL": (None, 6, 2, 2), "n = 0": (rows, 0, 2, 1), "dim = 0": (rows, 6, 0, 2), "k = 0": (rows, 6, 2, 0),
                                 "k > n": (rows, 6, 2, 7), "NaN": (with_nan, 6, 2, 2), "duplicates": (dup, 6, 2, 3)}.items():
        out = fill.copy()
        assert raw(r, n, dim, k, out) == glf.ERR_INVALID, what
        np.testing.assert_array_equal(out, fill, err_msg=what)
    assert raw(rows, 6, 2, 2, None) == glf.ERR_INVALID
    out = fill.copy()
    assert raw(rows, 6, 2, 6, out) == glf.OK                                      # n = k: every row, once
    assert sorted(map(tuple, out[:6])) == sorted(map(tuple, rows))
    np.testing.assert_array_equal(out[6:], fill[6:])
    with pytest.raises(ValueError):
        glf.cluster_seed(np.zeros(5), 2)
