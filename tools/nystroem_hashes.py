"""SHA-256 of what the Nystroem stage, the L_A operator and the degree stage write, with their info structs, in every form: whether a
change to the host code that drives those kernels -- the request, the scale rule, the shared tables of csrc/nystroem*.inc and
csrc/grid_common.inc -- left every bit alone. Run it once per build and compare the two files.
    python tools/nystroem_hashes.py new            # this tree's glf.py and libglf.so -> nystroem_hashes_new.json in the current directory
    python tools/nystroem_hashes.py parent DIR     # DIR holds another commit's glf.py and libglf.so -> nystroem_hashes_parent.json
On every shape of tests/nystroem_ref.py (SHAPES: its comments say what each is for), under both contraction modes:
  nystroem/  glf_Nystroem_ex for every entry of FORMS in tests/test_gpu_nystroem.py at ld 32, 64, 128 and 256 (the block of
             nystroem_ref.make_block, m = ld - 5) with skip_exact_zeros 0 and 1; once per form with a row sub-range written into a
             fill pattern; and once per form with the edge block: L_B's scale set to 1 so that Psi is phi_A, whose columns 10 .. 13
             are all zero, of maximum 2^-140 (subnormal), of maximum 3e37 (times the grid's rows it leaves the f32 range) and one
             holding an Inf -- the inputs at which two statements of the operand scale rule could part (csrc/scale_rule.hpp).
  operator/  Operator.apply_numpy at ld 32, 64, 128 and 256 and solve_numpy (ld 64, at most 12 iterations) for every entry of FORMS
             in tests/test_gpu_operator.py (operator_ref.make_block); a refusal is recorded as its status and message.
  degree/    glf_Degree_ex under DEG_PATH=grid (with the value-weighted sums) and auto, skip_exact_zeros 0 and 1, and a row sub-range.
One child process per (group, shape), each under its own time limit; nothing is started after one that fails.
The file to keep and compare holds one digest per (group, shape, contraction, form) -- SHA-256 over that form's cases, key and hash, in
sorted order -- and one per (shape, contraction) over the forms' edge-block cases; nystroem_hashes_<tag>_cases.json beside it holds every case, to find
the one that moved."""
import hashlib, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # (tools/ sits under the repository root)
CHILD_SECONDS = 240
GROUPS = ("nystroem", "operator", "degree")
MODES = ("f16s", "f32")
LDS = (32, 64, 128, 256)


def child(lib_dir, group, shape):
    if lib_dir:
        os.environ["GLF_LIBRARY"] = os.path.join(lib_dir, "libglf.so")
    for path in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), lib_dir or os.path.join(ROOT, "image-processing-graph-laplacian_amd")):
        sys.path.insert(0, path)
    import numpy as np
    import glf
    import nystroem_ref as nref
    import operator_ref as oref
    import test_gpu_nystroem as tnys
    import test_gpu_operator as top

    def sha(info, *arrays):
        h = hashlib.sha256(json.dumps(info, sort_keys=True).encode())
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()

    w, h, ns, seed, h_loc, p, nr, nc = nref.SHAPES[shape]
    img, idx = glf.synth_image(w, h, seed=seed), glf.Sampling(w, h, ns)
    assert idx.size == p
    sub = (3, min(h, 10))              # (off any multiple of a workgroup's pixels, as tests/test_gpu_nystroem.py's)
    out = {}
    for mode in MODES:
        one_mode(glf, np, nref, oref, tnys, top, sha, group, mode, (w, h, h_loc, p, img, idx, sub), out)
    print(json.dumps(out))


def one_mode(glf, np, nref, oref, tnys, top, sha, group, mode, case, res):
    w, h, h_loc, p, img, idx, sub = case
    out = {}
    with glf.Context(0) as ctx:
        ctx.set_contraction(glf.CONTRACT_F16_SPLIT if mode == "f16s" else glf.CONTRACT_F32_MFMA)
        d_img = ctx.to_device(img)
        if group == "degree":
            for path in ("grid", "auto"):
                for skip, rows in ((0, None), (1, None), (0, sub)):
                    ctx.reset_tuning()
                    ctx.set_tuning(DEG_PATH=path)
                    D, Uy, info = ctx.Degree_ex(d_img, idx, h_loc=h_loc, h_val=nref.H_VAL, skip_exact_zeros=skip, rows=rows, want_ysum=path == "grid")
                    out["%s/skip%d/%s" % (path, skip, "all" if rows is None else "rows")] = sha(info, D, *([Uy] if path == "grid" else []))
            res.update({"%s/%s" % (mode, k): v for k, v in out.items()})
            return
        _, K_B = ctx.ComputeAffinityMatrices(d_img, idx, want_KA=False, h_loc=h_loc, h_val=nref.H_VAL)
        L_A, L_B, alpha = ctx.ComputeLaplacianMatrix(None, K_B)
        ctx.destroy(L_A)
        if group == "nystroem":
            def run(form, phi_A, pinv, ld, skip=0, rows=None, fill=None, B=L_B):
                ctx.reset_tuning()
                ctx.set_tuning(**tnys.FORMS[form][0])
                dA, dP = ctx.dense_from_numpy(phi_A[:, :pinv.size], ld=ld), ctx.diag_from_numpy(pinv)
                given = None
                if fill is not None:
                    given = ctx.dense_from_numpy(fill, ld=ld, row_order=glf.ROWS_SAMPLE_FIRST)
                    given.cols = pinv.size
                phi, info = ctx.Nystroem_ex(B, dA, dP, skip_exact_zeros=skip, rows=rows, phi=given)
                res = sha(info, ctx.mat_to_numpy(phi, padded=True))
                ctx.destroy(dA, dP, phi)
                return res

            for form in tnys.FORMS:
                for ld in LDS:
                    phi_A, pinv = nref.make_block(p, ld, ld - 5, tnys.BLOCK_SEED)
                    for skip in (0, 1):
                        out["%s/ld%d/skip%d" % (form, ld, skip)] = run(form, phi_A, pinv, ld, skip=skip)
                phi_A, pinv = nref.make_block(p, 64, 59, tnys.BLOCK_SEED)
                out["%s/ld64/rows" % form] = run(form, phi_A, pinv, 64, rows=sub, fill=np.full((w * h, 64), -7.25, dtype=np.float32))
                # the edge block (see above): Psi = phi_A exactly
                unit = type(L_B).from_buffer_copy(L_B)
                unit.scale = 1.0
                rng = np.random.default_rng(5)
                edge = rng.uniform(-1.0, 1.0, (p, 64)).astype(np.float32)
                edge[:, 10] = 0.0
                edge[:, 11] *= np.float32(2.0 ** -141)
                edge[p // 3, 11] = np.float32(2.0 ** -140)
                edge[:, 12] *= np.float32(1e37)
                edge[p // 2, 12] = np.float32(3e37)
                edge[p - 1, 13] = np.float32("inf")
                with np.errstate(all="ignore"):
                    out["%s/ld64/edge_columns" % form] = run(form, edge, np.ones(59, dtype=np.float32), 64, B=unit)
        else:
            for form in top.FORMS:
                for ld in LDS:
                    ctx.reset_tuning()
                    ctx.set_tuning(**top.FORMS[form][0])
                    try:
                        with ctx.operator(L_B, ld_hint=ld) as op:
                            X = oref.make_block(p, ld, ld - 5, seed=100 + ld)
                            out["%s/ld%d/apply" % (form, ld)] = sha(op.info, op.apply_numpy(X))
                            if ld == 64:
                                Xs, R, info = op.solve_numpy(X, ld - 5, 1e-5, max_it=12, allow_noconv=True)
                                out["%s/ld%d/solve" % (form, ld)] = sha(info, Xs, R)
                    except glf.GlfError as e:
                        out["%s/ld%d" % (form, ld)] = "refused: %s %s" % (e.status, e)
        ctx.destroy(K_B)
    res.update({"%s/%s" % (mode, k): v for k, v in out.items()})


def main():
    tag, lib_dir = sys.argv[1], os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else None
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nystroem_ref as nref
    out = {}
    for group in GROUPS:
        for shape in nref.SHAPES:
            name = "%s/%s" % (group, shape)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", lib_dir or "", group, shape]
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=CHILD_SECONDS)
            except subprocess.TimeoutExpired:
                sys.exit("nystroem_hashes: %s exceeded %d s; nothing more is started" % (name, CHILD_SECONDS))
            if r.returncode != 0:
                sys.exit("nystroem_hashes: %s ended with status %d; nothing more is started" % (name, r.returncode))
            for key, val in json.loads(r.stdout.decode().strip().splitlines()[-1]).items():
                out["%s/%s" % (name, key)] = val
            print(name, "done", flush=True)
    json.dump(out, open("nystroem_hashes_%s_cases.json" % tag, "w"), indent=1, sort_keys=True)
    json.dump(digests(out), open("nystroem_hashes_%s.json" % tag, "w"), indent=1, sort_keys=True)
    print(tag, len(out), "cases")


def digests(cases):
    """{group/shape/contraction/form: SHA-256 of its cases' "key=hash" lines in sorted order}; the edge block's cases of all forms go
    into group/shape/contraction/edge_columns."""
    groups = {}
    for key in sorted(cases):
        part = key.split("/")
        name = "/".join(part[:3] + ["edge_columns"] if part[-1] == "edge_columns" else part[:4])
        groups.setdefault(name, hashlib.sha256()).update(("%s=%s\n" % (key, cases[key])).encode())
    return {name: h.hexdigest() for name, h in groups.items()}


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2] or None, sys.argv[3], sys.argv[4])
    else:
        main()
