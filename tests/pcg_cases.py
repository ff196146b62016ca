"""The graphs and right-hand sides of tests/test_pcg_ref.py (CPU) and tests/test_gpu_pcg.py, built once per process from the oracle's
K_A, degree and alpha in float64 (tests/pcg_ref.py: make_rhs).

Shapes (grey u8, glf.synth_image, glf.Sampling; w, h, samples requested, seed): those of tests/test_gpu_operator.py, and
  dense70  21 x 15, 70      p = 70 (7 x 10), sample pitch 2, h_loc = 5 (the others: 40): D^-1 A has condition number 1.34, a general
                            column takes 5 steps and a column of dimension d <= 5 exactly d (at the 1 % sampling of the others
                            the system is so diagonally dominant that nothing takes more than 3; at pitch 2 with h_loc = 40 the
                            spectrum has four separated eigenvalues and nothing takes more than 4, which is one step short of
                            the staircase); one reduction block of 128 rows in which 58 hold nothing
(ld, m) per shape: CASES. dense70 carries the whole grid ld 32 .. 256 x m = ld, ld - 5 (at ld 256, m = 251 the staircase); the
others one or two widths each, so that every ld and both kinds of m also meet p = 24, 132 (p % 64 != 0, p % 128 != 0), 320 and
1350 (11 reduction blocks)."""
import numpy as np

import glf
import oracle as orc
import pcg_ref as pr

SHAPES = {"dense70": (21, 15, 70, 8), "tiny": (53, 37, 20, 3), "edge128": (60, 58, 120, 4), "mid": (192, 64, 300, 5),
          "slabs": (450, 300, 1350, 6)}
CASES = [("dense70", ld, m) for ld in (32, 64, 128, 256) for m in (ld, ld - 5)] + [
    ("tiny", 32, 32), ("tiny", 256, 251), ("edge128", 64, 59), ("edge128", 128, 128), ("mid", 128, 123), ("mid", 64, 64),
    ("slabs", 32, 27), ("slabs", 256, 256)]
STAIRCASE = ("dense70", 256, 251)
RTOL = 1e-5
H_LOC, H_VAL = {"dense70": 5.0}, 30.0          # h_loc where it is not tests/test_gpu_operator.py's 40


class _Case:
    pass


_SHAPES, _RHS = {}, {}


def dinv_f32(alpha, D):
    """k_dinv_from_degree: 1.0f / (float)(alpha (D_i - 1.0))."""
    return (np.float32(1.0) / (alpha * (np.asarray(D, dtype=np.float64) - 1.0)).astype(np.float32)).astype(np.float32)


def shape(name):
    """The CPU side of a shape: image, samples, K_A, D, alpha (oracle, float64), A = alpha (diag(D) - K_A), the f32 preconditioner."""
    if name not in _SHAPES:
        w, h, ns, seed = SHAPES[name]
        c = _Case()
        c.w, c.h = w, h
        c.img = glf.synth_image(w, h, seed=seed)
        c.idx = glf.Sampling(w, h, ns)
        c.p = int(c.idx.size)
        c.h_loc = H_LOC.get(name, 40.0)
        prm = orc.default_params()
        prm.h_loc, prm.h_val = c.h_loc, H_VAL
        c.KA, _ = orc.affinity(c.img, c.idx, prm, want_KB=False)
        c.D = orc.degree(c.img, c.idx, prm)
        c.alpha = 1.0 / c.D.mean()
        c.A = c.alpha * (np.diag(c.D) - c.KA)
        c.dinv = dinv_f32(c.alpha, c.D)
        _SHAPES[name] = c
    return _SHAPES[name]


def rhs(name, ld, m):
    """pcg_ref.make_rhs of the shape's oracle operator, once (read-only afterwards)."""
    key = (name, ld, m)
    if key not in _RHS:
        c = shape(name)
        r = pr.make_rhs(c.A, c.dinv, c.p, ld, m, seed=len(name), rtol=RTOL, staircase=(key == STAIRCASE))
        r.B.setflags(write=False)
        _RHS[key] = r
    return _RHS[key]
