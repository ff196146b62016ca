"""The robust fit's C-ABI (glf_robust_weight, glf_robust_scale, glf_graph_robust_step, glf_graph_fit_robust): exported by libglf.so,
declared in include/glf.h, listed in glf.EXPORTS, the three structs laid out as a C compiler lays them out; without a handle the two
device calls answer GLF_ERR_INVALID before any device work; and the two host-only functions against numpy restatements. CPU only.

glf_robust_weight is the f64 statement of the table of include/glf.h as functions of q = r^2. The restatement below writes the same
table with the same operations (IEEE +, *, /, sqrt are correctly rounded on both sides; log1p is the platform's on both sides, a few
ulp apart at most), so the comparison is to 4 ulp of the value, branch points q = c^2 -/+ 1 ulp included. glf_robust_scale is a
selection: the comparison with a sort is exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("glf_robust_weight", "glf_robust_scale", "glf_graph_robust_step", "glf_graph_fit_robust")
LOSSES = ("huber", "cauchy", "tukey")
DEFAULT_C = {"huber": 1.345, "cauchy": 2.385, "tukey": 4.685}


def table64(loss, c, q):
    """(u, rho) of the table in numpy f64; q an array."""
    q = np.asarray(q, dtype=np.float64)
    c2 = c * c
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if loss == "huber":
            return np.where(q <= c2, 1.0, c / np.sqrt(q)), np.where(q <= c2, 0.5 * q, c * np.sqrt(q) - 0.5 * c2)
        if loss == "cauchy":
            return 1.0 / (1.0 + q / c2), 0.5 * c2 * np.log1p(q / c2)
        t = q / c2
        v = 1.0 - np.minimum(t, 1.0)
        return np.where(t < 1.0, (1.0 - t) * (1.0 - t), 0.0), c2 / 6.0 * (1.0 - v * v * v)


def test_robust_entry_points_are_exported_and_declared():
    lib = C.CDLL(glf.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in glf.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    kinds = re.search(r"enum\s*\{\s*GLF_ROBUST_HUBER\s*=\s*(\d+),\s*GLF_ROBUST_CAUCHY\s*=\s*(\d+),\s*GLF_ROBUST_TUKEY\s*=\s*(\d+)\s*\}", header)
    assert kinds and tuple(int(x) for x in kinds.groups()) == (glf.ROBUST_HUBER, glf.ROBUST_CAUCHY, glf.ROBUST_TUKEY) == (0, 1, 2)
    nobj = re.search(r"#define\s+GLF_ROBUST_OBJECTIVES\s+(\d+)\b", header)
    assert nobj and int(nobj.group(1)) == glf.ROBUST_OBJECTIVES == 32
    for struct in ("glf_robust_loss", "glf_robust_options", "glf_robust_stats"):
        assert re.search(r"typedef\s+struct\s+%s\s*\{" % struct, header), struct
    assert callable(glf.robust_weight) and callable(glf.robust_scale)
    for method in ("robust_step", "fit_robust"):
        assert hasattr(glf.Graph, method), method


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof and every offsetof of the three structs, as a C compiler lays out include/glf.h, against the ctypes mirrors."""
    mirrors = {"glf_robust_loss": glf.RobustLoss, "glf_robust_options": glf.RobustOptions, "glf_robust_stats": glf.RobustStats}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "glf.h"', "int main(void) {"]
    for struct, mirror in mirrors.items():
        lines.append('printf("%%zu", sizeof(%s));' % struct)
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (struct, f[0]) for f in mirror._fields_]
        lines.append('printf("\\n");')
    lines += ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)]).decode().split("\n")
    for line, mirror in zip(out, mirrors.values()):
        got = [int(x) for x in line.split()]
        assert got == [C.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_], mirror.__name__
    assert C.sizeof(glf.RobustLoss) == 16 + 8 * glf.MAX_SIGNALS
    assert C.sizeof(glf.RobustStats) == 16 + 8 * glf.MAX_SIGNALS + 8 + 8 * glf.ROBUST_OBJECTIVES


def _branch_points(c):
    c2 = c * c
    return np.array([0.0, np.nextafter(c2, 0.0), c2, np.nextafter(c2, np.inf), 1e-300, 1e-3 * c2, 0.25 * c2, 0.999 * c2, 1.001 * c2, 4.0 * c2,
                     1e6 * c2, 1e200])


@pytest.mark.parametrize("c", [None, 0.0, 0.5, 1.0, 3.0, 1e-6, 1e18])
@pytest.mark.parametrize("loss", LOSSES)
def test_robust_weight_against_the_table(loss, c):
    cc = DEFAULT_C[loss] if not c else c
    q = np.concatenate([_branch_points(cc), np.random.default_rng(5).uniform(0.0, 9.0, 200) * cc * cc])
    u, rho = glf.robust_weight(loss, q, c)
    wu, wrho = table64(loss, cc, q)
    assert u.shape == rho.shape == q.shape
    # near q = c^2 Tukey's u is (1 - t)^2 with t one ulp from 1, and Huber's rho a difference of two terms of size c^2 / 2:
    # 4 ulp of the value, or of the scale the value is a difference on
    assert np.all(np.abs(u - wu) <= 4 * 2.0 ** -52 * np.maximum(wu, 2.0 ** -52)), (loss, c)
    assert np.all(np.abs(rho - wrho) <= 4 * 2.0 ** -52 * np.maximum(wrho, cc * cc)), (loss, c)
    assert np.all((u >= 0.0) & (u <= 1.0) & (rho >= 0.0))
    # the branch points themselves
    c2 = cc * cc
    assert glf.robust_weight(loss, 0.0, c) == (1.0, 0.0)
    at, below, above = (glf.robust_weight(loss, x, c) for x in (c2, np.nextafter(c2, 0.0), np.nextafter(c2, np.inf)))
    if loss == "huber":
        assert at == (1.0, 0.5 * c2) and below[0] == 1.0 and 1.0 - 2.0 ** -50 < above[0] <= 1.0
    if loss == "cauchy":
        assert at[0] == 0.5 and below[0] >= 0.5 >= above[0]
    if loss == "tukey":
        assert at == (0.0, c2 / 6.0) and above == (0.0, c2 / 6.0) and 0.0 <= below[0] < 2.0 ** -100
        assert glf.robust_weight(loss, 1e200, c) == (0.0, c2 / 6.0)
    # rho is continuous and non-decreasing, u non-increasing
    qs = np.sort(q)
    us, rs = glf.robust_weight(loss, qs, c)
    assert np.all(np.diff(rs) >= -4 * 2.0 ** -52 * c2) and np.all(np.diff(us) <= 2.0 ** -50)
    # a string and the constant name the same loss
    assert glf.robust_weight(glf.ROBUST_LOSSES[loss], 2.0 * c2, c) == glf.robust_weight(loss, 2.0 * c2, c)


def test_robust_weight_refusals_leave_the_outputs_untouched():
    lib = glf._lib
    u, rho = C.c_double(-3.0), C.c_double(-4.0)
    for kind, c, q in ((-1, 1.0, 1.0), (3, 1.0, 1.0), (0, -1.0, 1.0), (0, float("inf"), 1.0), (1, float("nan"), 1.0), (2, 1.0, -1e-300),
                       (2, 1.0, float("nan")), (0, 1.0, float("-inf"))):
        assert lib.glf_robust_weight(C.c_int(kind), C.c_double(c), C.c_double(q), C.byref(u), C.byref(rho)) == glf.ERR_INVALID, (kind, c, q)
    assert (u.value, rho.value) == (-3.0, -4.0)
    assert lib.glf_robust_weight(C.c_int(0), C.c_double(1.0), C.c_double(4.0), None, None) == glf.OK
    assert lib.glf_robust_weight(C.c_int(0), C.c_double(1.0), C.c_double(4.0), C.byref(u), None) == glf.OK and u.value == 0.5 and rho.value == -4.0
    assert lib.glf_robust_weight(C.c_int(0), C.c_double(1.0), C.c_double(4.0), None, C.byref(rho)) == glf.OK and rho.value == 1.5
    with pytest.raises(glf.GlfError):
        glf.robust_weight("huber", -1.0)
    with pytest.raises(glf.GlfError):
        glf.robust_weight("huber", 1.0, c=-2.0)
    with pytest.raises(ValueError):
        glf.robust_weight("l1", 1.0)


def _scale_rule(res, w=None):
    mag = np.abs(np.asarray(res, dtype=np.float64))
    if w is not None:
        mag = mag[np.asarray(w) > 0]
    return 1.4826 * np.sort(mag)[(mag.size - 1) // 2]


def test_robust_scale_is_the_lower_median():
    assert glf.robust_scale([-5.0, 1.0, 3.0, -2.0, 4.0]) == 1.4826 * 3.0            # odd: the middle
    assert glf.robust_scale([-5.0, 1.0, 3.0, -2.0, 4.0, 6.0]) == 1.4826 * 3.0       # even: element floor((6 - 1) / 2) = 2, the lower one
    assert glf.robust_scale([7.0, -2.0]) == 1.4826 * 2.0
    assert glf.robust_scale([-0.5]) == 1.4826 * 0.5
    # weights that are zero or negative drop their entries: 5 1 . 2 . 6 -> element 1 of 1 2 5 6
    assert glf.robust_scale([-5.0, 1.0, 3.0, -2.0, 4.0, 6.0], [1.0, 0.5, 0.0, 2.0, -1.0, 1e-300]) == 1.4826 * 2.0
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 10, 11, 1000, 4097):
        res = rng.normal(size=n)
        assert glf.robust_scale(res) == _scale_rule(res)
        w = (rng.uniform(size=n) < 0.6).astype(np.float64)
        w[0] = 1.0
        assert glf.robust_scale(res, w) == _scale_rule(res, w)
        assert glf.robust_scale(res.reshape(1, n), w.reshape(1, n)) == _scale_rule(res, w)
    # Gaussian residuals: the estimate is the standard deviation to sampling error
    assert abs(glf.robust_scale(rng.normal(0.0, 2.5, 200000)) - 2.5) < 0.03


def test_robust_scale_refusals_leave_sigma_untouched():
    lib = glf._lib
    sigma = C.c_double(-9.0)
    res, zeros = np.array([1.0, 2.0, 3.0]), np.array([0.0, 0.0, 5.0])
    cases = ((None, None, 3), (res, None, 0), (res, np.zeros(3), 3), (res, -np.ones(3), 3), (np.array([1.0, np.nan, 3.0]), None, 3),
             (np.array([1.0, np.inf, 3.0]), None, 3), (np.array([1.0, np.nan, 3.0]), np.zeros(3), 3), (res, np.array([1.0, np.nan, 1.0]), 3),
             (res, np.array([1.0, np.inf, 1.0]), 3), (zeros, None, 3))
    for r, w, n in cases:
        assert lib.glf_robust_scale(glf._ptr(r), glf._ptr(w), C.c_size_t(n), C.byref(sigma)) == glf.ERR_INVALID
    assert lib.glf_robust_scale(glf._ptr(res), None, C.c_size_t(3), None) == glf.ERR_INVALID
    assert sigma.value == -9.0
    with pytest.raises(glf.GlfError):
        glf.robust_scale([0.0, 0.0, 1.0])
    with pytest.raises(glf.GlfError):
        glf.robust_scale([])
    with pytest.raises(ValueError):
        glf.robust_scale([1.0, 2.0], [1.0])


def test_device_calls_without_a_handle_are_invalid():
    lib = C.CDLL(glf.LIB_PATH)
    one = C.c_void_p(1)
    buf = (C.c_double * 64)()
    loss = glf.RobustLoss(struct_size=C.sizeof(glf.RobustLoss), kind=0, c=1.0)
    loss.sigma[0] = 1.0
    out = C.c_double(7.0)
    assert lib.glf_graph_robust_step(None, C.byref(loss), None, C.c_int(1), one, buf, buf, buf, C.byref(out), C.byref(out), None, None) == glf.ERR_INVALID
    assert lib.glf_graph_robust_step(None, None, None, C.c_int(0), None, None, None, None, None, None, None, None) == glf.ERR_INVALID
    opt = glf.RobustOptions(struct_size=C.sizeof(glf.RobustOptions), loss=loss)
    st = glf.RobustStats(struct_size=C.sizeof(glf.RobustStats))
    assert lib.glf_graph_fit_robust(None, C.byref(opt), None, C.c_int(1), one, buf, None, None, C.byref(st)) == glf.ERR_INVALID
    assert lib.glf_graph_fit_robust(None, None, None, C.c_int(1), None, None, None, None, None) == glf.ERR_INVALID
    assert out.value == 7.0 and st.iterations == 0
