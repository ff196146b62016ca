"""The Jacobi-preconditioned block PCG of the eigen-solve on its own, through glf_operator_solve (the solver's set-up and loop: one
code), in every form of the operator against a float64 solve. Needs an MI355X: -m gpu.

Reference: tests/pcg_ref.py (pcg64, pcg_f32, drift_bound; its docstring holds the recurrences and where the kernels round).
A = alpha (diag(D) - K_A) in float64 with D and alpha the GPU's own and K_A the oracle's, as in tests/test_gpu_operator.py; stored
forms: the stored matrix as downloaded, f32 bits widened. Right-hand sides: tests/pcg_cases.py (shapes, (ld, m) per shape, the
staircase), built from the oracle's operator; their counts are taken again under the GPU's A and must be robust there too.

Runs: stored with f32 operands (the f32 contraction), stored split-f16, grid, rank, band (the split-f16 contraction: the factored
forms exist under it only). rtol 1e-5; once per run also 1e-7.

Per run and case (test_against_fp64):
  a  the rule, exactly: ||R_j||^2 <= rtol^2 ||B_j||^2 (1 + 1e-12) in float64 of the returned f32 values (1e-12 covers p 2^-53 of
     another summation order); a solve cut at k < iters answers GLF_ERR_NOCONV with `unconverged` = the number of columns whose
     count exceeds k, every such column of its R fails the rule, and every column that had converged by k has the bits of the
     whole solve (a converged column is never touched again)
  b  R is the residual: |(B - A X) - R| <= drift_bound componentwise on the first m columns, whole solve and cuts at 1 and 2
  c  counts: single-column solves (one column of each kind, the others zero) take what pcg64 takes, the block takes their maximum,
     and every run of a case takes the same
  d  a column solved alone has the bits of that column in the block (where it went through packed sweeps at other positions)
  f  a column times 2^+-30 returns the exact multiple (every form scales its operand per column by powers of two: the operator
     test's test_power_of_two_column_scaling_is_exact holds for all of them)
  g  the all-zero column returns exact zeros and, alone, costs no step and no sweep; padding columns m .. ld - 1 filled with 7.0
     change no bit of the first m columns and return X = 0, R = 7.0 (R = B: k_cg_init copies the block, nothing iterates there)
The other tests: tunings, the device's active count after every step and the widths of its packed sweeps against the reference's
(the VERBOSE log; the staircase: 192, 128, 64, 32) (e), a second run (f), refusals (h), rtol 1e-7.

Set GLF_PCG_ERROR_JSON to a path to have the largest drift / bound, the largest true relative residual and the counts per run and
ld written there (tools/pcg_error.py; a record: the asserted bound is the derived one)."""
import json
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import operator_ref as oref  # noqa: E402
import pcg_cases as pc  # noqa: E402
import pcg_ref as pr  # noqa: E402
import test_gpu_operator as top  # noqa: E402
from test_gpu_operator import FORMS, _bits, _operator  # noqa: E402

RUNS = [("f32", "dense"), ("f16s", "dense"), ("f16s", "grid"), ("f16s", "rank"), ("f16s", "band")]
RUN_IDS = ["%s-%s" % r for r in RUNS]
CASE_IDS = ["%s-%d-%d" % c for c in pc.CASES]
RTOL = pc.RTOL
DESIGNED = ("eig1", "eig2", "eig3", "eig4", "eig5", "unit", "halfzero", "scaled-", "scaled+")
_RECORD, _COUNTS, _SIDES, _PROBLEMS, _REFS = {}, {}, {}, {}, {}

assert {k: v for k, v in pc.SHAPES.items() if k != "dense70"} == top.SHAPES


@pytest.fixture(scope="module")
def ctxs():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    out = {}
    for mode in ("f16s", "f32"):
        c = glf.Context(0)
        c.set_contraction(glf.CONTRACT_F16_SPLIT if mode == "f16s" else glf.CONTRACT_F32_MFMA)
        c.mode, c.graphs = mode, {}
        out[mode] = c
    yield out
    for c in out.values():
        for d_img, K_B, L_B, alpha, D in c.graphs.values():
            c.destroy(K_B)
        c.close()
    path = os.environ.get("GLF_PCG_ERROR_JSON")
    if path and _RECORD:
        what = ("per run (contraction-form) and ld over the cases of tests/test_gpu_pcg.py on an MI355X (python tools/pcg_error.py): the largest "
                "|(B - A X) - R| / drift_bound (asserted <= 1), the largest true relative residual ||B - A X|| / ||B|| over the non-zero columns "
                "at rtol 1e-5 and (ld 64, the rtol 1e-7 case) at 1e-7, and the block's step counts seen. A record only.")
        rows = [dict(run=k[0], ld=k[1], **v) for k, v in sorted(_RECORD.items())]
        with open(path, "w") as f:
            json.dump(dict(what=what, rows=rows), f, indent=1)


@pytest.fixture(autouse=True)
def _default_kernel_selection(ctxs):
    yield
    for c in ctxs.values():
        c.reset_tuning()


def _note(mode, form, ld, **kw):
    r = _RECORD.setdefault(("%s-%s" % (mode, form), ld), dict(worst_drift_over_bound=0.0, true_rel_residual_1e5=0.0, true_rel_residual_1e7=None, iters=[]))
    for k, v in kw.items():
        if k == "iters":
            r[k] = sorted(set(r[k]) | {int(v)})
        else:
            r[k] = max(r[k] or 0.0, float(v))       # (None: not measured at this ld)


def _side(ctx, name):
    """The graph of a shape on this context and what the bounds need of its CPU side."""
    key = (ctx.mode, name)
    if key not in _SIDES:
        c = pc.shape(name)
        s = top._Ref()
        s.c, s.p = c, c.p
        s.d_img, s.K_B, s.L_B, s.alpha, s.D = top._graph(ctx, ("pcg", name), ctx.to_device(c.img), c.idx, h_loc=c.h_loc, h_val=pc.H_VAL)
        s.nr, s.nc = oref.grid_shape(c.idx, c.w)
        rr, cc = (c.idx // c.w).astype(np.float64), (c.idx % c.w).astype(np.float64)
        s.Ksp = np.exp(-((rr[:, None] - rr[None, :]) ** 2 + (cc[:, None] - cc[None, :]) ** 2) / c.h_loc ** 2)
        s.dinv = pc.dinv_f32(s.alpha, s.D)
        assert abs(s.alpha - c.alpha) <= 1e-5 * c.alpha
        _SIDES[key] = s
    return _SIDES[key]


def _problem(ctx, form, name, op):
    """(A float64, |A|, op_bound: P -> the sweep's bound on the operand P) of a run on a shape; the stored forms: from the operator."""
    s = _side(ctx, name)
    key = (ctx.mode, form if form == "dense" else "factored", name)
    if key not in _PROBLEMS:
        if form == "dense":
            S = op.stored().astype(np.float64)
            A = S if ctx.mode == "f32" else S.T
            op.apply_numpy(np.ones((s.p, 32), dtype=np.float32))
            ksplit = max(op.info["ksplit"], 1)
        else:
            A, ksplit = s.alpha * (np.diag(s.D) - s.c.KA), 1
        _PROBLEMS[key] = (A, np.abs(A), ksplit)
    A, absL, ksplit = _PROBLEMS[key]
    p = s.p

    def op_bound(P):
        aP = np.abs(P)
        if form == "dense":
            g = oref.gamma(ctx.mode, p, ksplit=ksplit)
            return oref.bound(ctx.mode, g, absL @ aP, P, p, absL_rowsum=absL.sum(axis=1))
        bform = FORMS[form][1]
        g = oref.gamma(bform, p, nr=s.nr, nc=s.nc)
        Kabs = s.Ksp if bform == "rank" else s.c.KA
        absLX = s.alpha * (s.D[:, None] * aP + Kabs @ aP)
        return oref.bound(bform, g, absLX, P, p, alpha=s.alpha, Ksp_X=(s.Ksp @ aP) if bform == "rank" else None)

    return key, A, absL, op_bound


def _reference(key, A, dinv, r, rtol=RTOL):
    """pcg64's counts with their robustness and the pcg_f32 trajectories (whole, cut at 1 and at 2) under this A, once."""
    k = key + (r.ld, r.m, rtol)
    if k not in _REFS:
        count, robust = pr.counts_robust(A, dinv, r.B, r.m, rtol)
        _REFS[k] = (count, robust, {it: pr.pcg_f32(A, dinv, r.B, r.m, rtol, it) for it in (1, 2, 1000)})
    return _REFS[k]


def _expected_widths(traj, ld):
    """The packed sweeps of a solve that goes through traj's active counts (block_pcg_work: from ld 64 on, step k + 1 is applied to
    32 columns when at most 32 were active after step k, else to that count rounded up to 64 -- where that is narrower than ld)."""
    if ld < 64:
        return []
    cand = [32 if na <= 32 else pr.round_up(na, 64) for na in traj.nactive[1:traj.iters]]
    return [w for w in cand if w < ld]


def _rule(B, R, p, rtol):
    f8 = np.float64
    rr, bn2 = (R[:p].astype(f8) ** 2).sum(axis=0), (B[:p].astype(f8) ** 2).sum(axis=0)
    return rr, rtol * rtol * bn2


def _drift_ratio(A, B, X, R, p, m, bound):
    d = pr.drift(A, B, X, R, p)[:, :m]
    b = bound[:, :m]
    assert np.isfinite(d).all()
    bad = np.argwhere(d > b)
    ratio = float((d[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    assert bad.size == 0, "%d elements beyond the drift bound, first (row %d, column %d): drift %.3e, bound %.3e; worst ratio %.2f" % (
        len(bad), bad[0][0], bad[0][1], d[tuple(bad[0])], b[tuple(bad[0])], ratio)
    return ratio


def _true_residual(A, B, X, p, m):
    f8 = np.float64
    t = B[:p, :m].astype(f8) - A @ X[:p, :m].astype(f8)
    bn = np.linalg.norm(B[:p, :m].astype(f8), axis=0)
    return float((np.linalg.norm(t, axis=0)[bn > 0] / bn[bn > 0]).max())


@pytest.mark.parametrize("name,ld,m", pc.CASES, ids=CASE_IDS)
@pytest.mark.parametrize("mode,form", RUNS, ids=RUN_IDS)
def test_against_fp64(ctxs, mode, form, name, ld, m):
    ctx = ctxs[mode]
    s, r = _side(ctx, name), pc.rhs(name, ld, m)
    p, B, kind = s.p, r.B, np.array(r.kind)
    with _operator(ctx, form, s.L_B, ld_hint=ld) as op:
        key, A, absL, op_bound = _problem(ctx, form, name, op)
        count, robust, traj = _reference(key, A, s.dinv, r)
        live = traj[1000].active0
        assert robust[np.isin(kind, DESIGNED)].all(), "a designed column has no robust count under the GPU's own D and alpha"
        X, R, info = op.solve_numpy(B, m, RTOL, max_it=100)
        assert info["status"] == glf.OK and info["unconverged"] == 0 and info["path"] == FORMS[form][2]
        assert np.isfinite(X).all() and np.isfinite(R).all() and not X[p:].any() and not R[p:].any()
        # a: the rule on every column
        rr, lim = _rule(B, R, p, RTOL)
        assert (rr[:m] <= lim[:m] * (1 + 1e-12)).all(), np.flatnonzero(rr[:m] > lim[:m] * (1 + 1e-12))
        # c: the block's count
        iters = info["iters"]
        if robust[live].all():
            assert iters == count.max(), (iters, count.max())
        else:
            assert count[robust].max() <= iters <= count.max() + 1
        assert info["matvecs"] == (0 if mode == "f32" else iters)        # (timed sweeps: the stored f32-operand form times none)
        if robust[live].all():      # which sweeps are packed follows from the active counts, one step old
            assert info["narrow_sweeps"] == (0 if form == "dense" else len(_expected_widths(traj[1000], ld))), info
        if form != "dense" and name == "dense70" and ld >= 64:
            assert info["narrow_sweeps"] > 0
        # b: R is the residual
        ratio = _drift_ratio(A, B, X, R, p, m, pr.drift_bound(traj[1000], absL, op_bound))
        print("%s-%s %s ld %d m %d: %d steps, worst drift / bound %.3f" % (mode, form, name, ld, m, iters, ratio))
        _note(mode, form, ld, worst_drift_over_bound=ratio, true_rel_residual_1e5=_true_residual(A, B, X, p, m), iters=iters)
        # a, b, i: solves cut at k < iters
        for k in range(1, iters):
            Xk, Rk, ik = op.solve_numpy(B, m, RTOL, max_it=k, allow_noconv=True)
            later = live & robust & (count > k)
            unsure = int((live & ~robust).sum())
            assert ik["status"] == glf.ERR_NOCONV and ik["iters"] == k
            assert later.sum() <= ik["unconverged"] <= later.sum() + unsure, (k, ik, int(later.sum()))
            rrk, limk = _rule(B, Rk, p, RTOL)
            assert (rrk[later] > limk[later]).all()
            done = robust & (count <= k)
            np.testing.assert_array_equal(_bits(Xk[:, done]), _bits(X[:, done]))
            np.testing.assert_array_equal(_bits(Rk[:, done]), _bits(R[:, done]))
            if k <= 2:
                ratio = _drift_ratio(A, B, Xk, Rk, p, m, pr.drift_bound(traj[k], absL, op_bound))
                _note(mode, form, ld, worst_drift_over_bound=ratio)
        with pytest.raises(glf.GlfError) as e:         # (and without allow_noconv the cut is an error that names the count)
            op.solve_numpy(B, m, RTOL, max_it=iters - 1)
        assert e.value.status == glf.ERR_NOCONV and "unconverged" in str(e.value)
        # c, d: one column of each kind alone
        seen = {}
        for kd in dict.fromkeys(kind[:m]):
            j = int(np.flatnonzero(kind == kd)[0])
            if kd in ("zero", "pad"):
                continue
            B1 = np.zeros_like(B)
            B1[:, j] = B[:, j]
            X1, R1, i1 = op.solve_numpy(B1, m, RTOL, max_it=100)
            seen[kd] = i1["iters"]
            if robust[j]:
                assert i1["iters"] == count[j], (kd, j, i1["iters"], count[j])
            np.testing.assert_array_equal(_bits(X1[:, j]), _bits(X[:, j]), err_msg="column %d (%s) alone" % (j, kd))
            np.testing.assert_array_equal(_bits(R1[:, j]), _bits(R[:, j]), err_msg="column %d (%s) alone" % (j, kd))
            other = np.arange(ld) != j
            assert not X1[:, other].any() and not R1[:, other].any()
        for other_run, other_seen in _COUNTS.setdefault((name, ld, m), {}).items():
            for kd, n in seen.items():
                if kd != "general":
                    assert other_seen[kd] == n, "%s takes %d steps here and %d under %s" % (kd, n, other_seen[kd], other_run)
        _COUNTS[(name, ld, m)][(mode, form)] = seen
        # f: exact power-of-two multiples
        for j in np.flatnonzero(np.isin(kind, ("scaled-", "scaled+"))):
            sc = np.float32(2.0 ** (30 if kind[j] == "scaled+" else -30))
            np.testing.assert_array_equal(_bits(X[:, j]), _bits(X[:, r.base[j]] * sc))
            np.testing.assert_array_equal(_bits(R[:, j]), _bits(R[:, r.base[j]] * sc))
            assert np.abs(X[:, j]).max() > 0
        # g: the all-zero column, alone and in the block; padding columns of 7.0
        jz = int(np.flatnonzero(kind == "zero")[0])
        assert not _bits(X[:, jz]).any() and not _bits(R[:, jz]).any()
        X0, R0, i0 = op.solve_numpy(np.zeros_like(B), m, RTOL, max_it=100)
        assert (i0["iters"], i0["matvecs"], i0["unconverged"], i0["status"]) == (0, 0, 0, glf.OK)
        assert not _bits(X0).any() and not _bits(R0).any()
        assert not _bits(X[:, m:]).any() and not _bits(R[:, m:]).any()
        if m < ld:
            B7 = B.copy()
            B7[:p, m:] = 7.0
            X7, R7, i7 = op.solve_numpy(B7, m, RTOL, max_it=100)
            assert i7["iters"] == iters and i7["narrow_sweeps"] == info["narrow_sweeps"]
            np.testing.assert_array_equal(_bits(X7[:, :m]), _bits(X[:, :m]))
            np.testing.assert_array_equal(_bits(R7[:, :m]), _bits(R[:, :m]))
            assert not _bits(X7[:, m:]).any()
            np.testing.assert_array_equal(_bits(R7[:, m:]), _bits(B7[:, m:]))


@pytest.mark.parametrize("mode,form", RUNS, ids=RUN_IDS)
def test_rtol_1e_7(ctxs, mode, form):
    """The rule and the drift at rtol 1e-7, below the relative error of a split-f16 sweep: the recurrence reaches it, and R stays the
    residual within the bound. The counts are not compared column by column (no robustness is claimed at this rtol); the block's may
    differ from the emulation's by one."""
    ctx = ctxs[mode]
    name, ld, m, rtol = "dense70", 64, 59, 1e-7
    s, r = _side(ctx, name), pc.rhs(name, ld, m)
    with _operator(ctx, form, s.L_B, ld_hint=ld) as op:
        key, A, absL, op_bound = _problem(ctx, form, name, op)
        X, R, info = op.solve_numpy(r.B, m, rtol, max_it=60)
        assert info["status"] == glf.OK and info["unconverged"] == 0
        rr, lim = _rule(r.B, R, s.p, rtol)
        assert (rr[:m] <= lim[:m] * (1 + 1e-12)).all()
        t = pr.pcg_f32(A, s.dinv, r.B, m, rtol, max_it=60)
        assert abs(info["iters"] - t.iters) <= 1, (info["iters"], t.iters)
        ratio = _drift_ratio(A, r.B, X, R, s.p, m, pr.drift_bound(t, absL, op_bound))
        true = _true_residual(A, r.B, X, s.p, m)
        print("%s-%s rtol 1e-7: %d steps (emulation %d), worst drift / bound %.3f, true relative residual %.3e" % (mode, form, info["iters"], t.iters, ratio, true))
        _note(mode, form, ld, worst_drift_over_bound=ratio, true_rel_residual_1e7=true)


def _widths(err):
    return [int(w) for w in re.findall(r"operator applied to (\d+) packed columns", err)]


@pytest.mark.parametrize("mode,form", RUNS, ids=RUN_IDS)
def test_tunings_and_a_second_run_give_the_same_bits(ctxs, mode, form, capfd):
    """e, f: NO_NARROW=1 and OPERAND_MAXIMA=sweep against the default, and the default again: the same bits of X and R. The staircase
    (ld 256, m 251: 160, 100, 48 and 20 columns active after the steps 1 .. 4) is applied 192, 128, 64 and 32 columns wide by the
    factored forms (the VERBOSE log), never packed by the stored ones or under NO_NARROW."""
    ctx = ctxs[mode]
    for name, ld, m in (pc.STAIRCASE, ("dense70", 128, 123), ("slabs", 256, 256)):
        s, r = _side(ctx, name), pc.rhs(name, ld, m)
        with _operator(ctx, form, s.L_B, ld_hint=ld) as op:
            key, A, absL, op_bound = _problem(ctx, form, name, op)
            count, robust, traj = _reference(key, A, s.dinv, r)
            assert robust[traj[1000].active0].all()
            capfd.readouterr()
            ctx.set_tuning(VERBOSE="1")
            X, R, info = op.solve_numpy(r.B, m, RTOL, max_it=100)
            err = capfd.readouterr().err
            ctx.set_tuning(VERBOSE=None)
            widths = _widths(err)
            active = [int(a) for a in re.findall(r"step \d+: (\d+) of \d+ columns active", err)]
            assert active == traj[1000].nactive[1:], (active, traj[1000].nactive)      # which columns are active at which step
            assert info["narrow_sweeps"] == len(widths)
            assert widths == ([] if form == "dense" else _expected_widths(traj[1000], ld)), widths
            if (name, ld, m) == pc.STAIRCASE:
                assert info["iters"] == 5 and active == list(pr.STAIRCASE_AFTER) + [0]
                assert widths == ([] if form == "dense" else [192, 128, 64, 32]), widths
            elif form != "dense":
                assert widths, "no packed sweep at %s ld %d" % (name, ld)
            X2, R2, info2 = op.solve_numpy(r.B, m, RTOL, max_it=100)
            assert info2 == info
            np.testing.assert_array_equal(_bits(X2), _bits(X))
            np.testing.assert_array_equal(_bits(R2), _bits(R))
            for tuning in (dict(NO_NARROW="1"), dict(OPERAND_MAXIMA="sweep"), dict(NO_NARROW="1", OPERAND_MAXIMA="sweep")):
                ctx.set_tuning(**tuning)
                Xt, Rt, it = op.solve_numpy(r.B, m, RTOL, max_it=100)
                ctx.set_tuning(**{k: None for k in tuning})
                assert it["iters"] == info["iters"] and it["matvecs"] == info["matvecs"]
                assert it["narrow_sweeps"] == (0 if "NO_NARROW" in tuning else info["narrow_sweeps"])
                np.testing.assert_array_equal(_bits(Xt), _bits(X), err_msg=str(tuning))
                np.testing.assert_array_equal(_bits(Rt), _bits(R), err_msg=str(tuning))


@pytest.mark.parametrize("mode,form", RUNS, ids=RUN_IDS)
def test_refusals_leave_X_and_R_untouched(ctxs, mode, form):
    """h: every refusal names its reason and leaves a fill pattern's bits in X and R."""
    ctx = ctxs[mode]
    name, ld, m = "edge128", 64, 59
    s, r = _side(ctx, name), pc.rhs(name, ld, m)
    rows64 = oref.round_up(s.p, 64)
    fill = np.full((rows64, ld), -7.25, dtype=np.float32)

    def refused(op, status, word, B=r.B, m=m):
        with pytest.raises(glf.GlfError) as e:
            op.solve_numpy(B, m, RTOL, fill=np.full((rows64, B.shape[1]), -7.25, dtype=np.float32))
        assert e.value.status == status and word in str(e.value), str(e.value)
        assert (_bits(op.last_X) == _bits(fill[:1, :1])).all() and (_bits(op.last_R) == _bits(fill[:1, :1])).all()

    with _operator(ctx, form, s.L_B, ld_hint=ld) as op:
        refused(op, glf.ERR_INVALID, "m = 0", m=0)
        refused(op, glf.ERR_INVALID, "m = 65", m=ld + 1)
        refused(op, glf.ERR_INVALID, "fewer than p", B=r.B[:s.p - 1])
        refused(op, glf.ERR_INVALID, "ld", B=np.ones((s.p, 96), dtype=np.float32))
        if form != "dense":
            refused(op, glf.ERR_INVALID, "ld", B=np.ones((s.p, 192), dtype=np.float32), m=100)   # a sweep takes 192, the block PCG does not
        # B, X and R of different ld; X = B
        dB, dX, dR = ctx.dense_from_numpy(r.B, ld=ld), ctx.dense_from_numpy(fill, ld=ld), ctx.dense_from_numpy(np.full((rows64, 32), -7.25, dtype=np.float32), ld=32)
        for args, word in (((dB, dX, dR), "ld"), ((dB, dR, dX), "ld"), ((dB, dB, dX), "distinct"), ((dB, dX, dX), "distinct"), ((dB, s.L_B, dX), "dense")):
            with pytest.raises(glf.GlfError) as e:
                op.solve(*args, m)
            assert e.value.status == glf.ERR_INVALID and word in str(e.value), str(e.value)
            assert (_bits(ctx.mat_to_numpy(dX, padded=True)) == _bits(fill[:1, :1])).all() and (_bits(ctx.mat_to_numpy(dR, padded=True)) == _bits(fill[:1, :1])).all()
        np.testing.assert_array_equal(_bits(ctx.mat_to_numpy(dB, padded=True)), _bits(r.B))
        with pytest.raises(glf.GlfError) as e:
            op.solve(dB, dX, None, m, rtol=0.0)
        assert e.value.status == glf.ERR_INVALID and "rtol" in str(e.value)
        ctx.destroy(dB, dX, dR)
        # a tuning changed since creation
        ctx.set_tuning(MV_PATH="dense" if form != "dense" else "grid")
        refused(op, glf.ERR_INVALID, "changed since")
        ctx.set_tuning(**FORMS[form][0])
        X, R, info = op.solve_numpy(r.B, m, RTOL, want_R=False)          # the handle still works, and R may be left out
        assert R is None and info["status"] == glf.OK and np.abs(X[:s.p, :m]).max() > 0
    # an operator created for a row range
    if mode == "f16s":
        rows = (0, 64) if form == "dense" else (0, s.nc)
        with _operator(ctx, form, s.L_B, rows=rows, ld_hint=ld) as op:
            refused(op, glf.ERR_UNSUPPORTED, "communicator")
