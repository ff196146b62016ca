"""SHA-256 of everything the graph-handle passes over Phi write -- synthesize (nout 1, 5, 32, with and without identity terms),
normal_equations (no weight, a 0/1 weight, a real weight; 0, 1, 4 planes), project_wide (1, 7, 32 planes, with and without w),
robust_step (each loss, 1 and 3 planes, all optional outputs), fit_robust with an estimated scale (the sampled rows), transform
(m_new = m and m_new < m, Phi hashed afterwards), orthonormalize (both modes), quadform (r = 5 and 40, 1 and 7 centres, plain and
accumulating), classify (k = 2, 8, 32, with and without identity planes and bias, all three outputs), edges (the default directions)
and one cluster_step -- the per-pixel and reduction passes three times: on the f32 handle, on that handle compacted after those
calls (f32_then_compact/: equal to compact/ hash for hash, or a call left something in the handle) and on a handle compacted before its
first call (compact/) -- on the five shapes of tests/test_gpu_graph.py, on
509 x 515 with 300 samples (more tiles than resident waves) at m = 8, 40, 100 and 200, and on 1031 x 517 at ld 32 (more than
4 x 4096 tiles: a wave ends an f32 chain mid-run); then tools/cluster_hashes.py for the segmentation. Whether a change left the bits of
the graph handle alone: run it once per build and compare the files.
    python tools/graph_hashes.py new            # this tree's glf.py and libglf.so -> graph_hashes_new.json, cluster_hashes_new.json here
    python tools/graph_hashes.py parent DIR     # DIR holds another commit's glf.py and libglf.so -> graph_hashes_parent.json, ...
    python tools/graph_hashes.py --digest FILE...   # the files' cases in groups (shape, storage), one SHA-256 per group: what is kept
Every run is a child process of its own under its own time limit; nothing is started after one that fails."""
import hashlib, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # (tools/ sits under the repository root)
W, H = 61, 47
# name: (width, height, samples, m)
SHAPES = {"ld32": (W, H, 100, 8), "ld64": (W, H, 100, 40), "ld128": (W, H, 200, 100), "ld256": (W, H, 200, 200),
          "tiny": (16, 10, 12, 4), "tiles_m8": (509, 515, 300, 8), "tiles_m40": (509, 515, 300, 40),
          "tiles_m100": (509, 515, 300, 100), "tiles_m200": (509, 515, 300, 200), "chain_ld32": (1031, 517, 300, 8)}
CHILD_SECONDS = 300


def child(tag, lib_dir, shape):
    if lib_dir:
        os.environ["GLF_LIBRARY"] = os.path.join(lib_dir, "libglf.so")
        sys.path.insert(0, lib_dir)
    else:
        sys.path.insert(0, os.path.join(ROOT, "image-processing-graph-laplacian_amd"))
    import numpy as np
    import torch
    import glf

    def sha(*arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).tobytes())
        return h.hexdigest()

    w, h, ns, m = SHAPES[shape]
    out = {}
    with glf.Context(0) as ctx:
        seed = [11, list(SHAPES).index(shape)]
        rng = np.random.default_rng(seed)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)
        planes = dev(rng.normal(0.0, 40.0, (32, h, w)).astype(np.float32))
        wreal = dev(rng.uniform(0.0, 2.0, (h, w)).astype(np.float32))
        wmask = dev((rng.uniform(size=(h, w)) < 0.3).astype(np.float32))
        opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=0.1)
        img = ctx.to_device(glf.synth_image(w, h, seed=3))

        def passes(g, prefix):
            """every per-pixel and reduction pass on the handle as it is stored, the inputs the same at every call"""
            rng = np.random.default_rng(seed + [1])
            for nout in (1, 5, 32):
                a = rng.normal(0.0, 1.0, (nout, m))
                out[prefix + "synthesize/%d" % nout] = sha(g.synthesize(a))
                out[prefix + "synthesize/%d/ident" % nout] = sha(g.synthesize(a, ident=rng.uniform(0.5, 1.5, nout).astype(np.float32),
                                                                              plane=np.arange(nout) % 4 - 1, planes=planes[:3]))
            for wname, wt in (("none", None), ("mask", wmask), ("real", wreal)):
                for k in (0, 1, 4):
                    G, b = g.normal_equations(wt, planes[:k] if k else None)
                    out[prefix + "normal/%s/%d" % (wname, k)] = sha(G, b)
                for k in (1, 7, 32):
                    if wname != "mask":
                        out[prefix + "project_wide/%s/%d" % (wname, k)] = sha(g.project_wide(planes[:k], wt))
            a4 = rng.normal(0.0, 1.0, (4, m))
            for loss in ("huber", "cauchy", "tukey"):
                for k in (1, 3):
                    G, b, lo, ma, wout, rout = g.robust_step(planes[:k], a4[:k], loss, sigma=rng.uniform(20.0, 60.0, k), weight=wreal, want_weights=True,
                                                             want_residuals=True)
                    out[prefix + "robust_step/%s/%d" % (loss, k)] = sha(G, b, np.array([lo, ma]), wout, rout)
            fit, info = g.fit_robust(planes[:2], weight=wreal, loss="huber", sigma=None, ridge=0.1, max_iter=3, sample_rows=500, return_info=True)
            out[prefix + "fit_robust/estimated_sigma"] = sha(fit, info["coeffs"], info["weights"], info["sigma"], info["objective"])
            for r in (5, 40):
                for ncent in (1, 7):
                    R, cen = rng.normal(0.0, 1.0, (m, r)) / np.sqrt(m), rng.normal(0.0, 0.01, (ncent, r))
                    q = g.quadform(R, cen)
                    out[prefix + "quadform/%d/%d" % (r, ncent)] = sha(q)
                    out[prefix + "quadform/%d/%d/accumulate" % (r, ncent)] = sha(g.quadform(R, cen, out=q, accumulate=True))
            for k in (2, 8, 32):
                a = rng.normal(0.0, 1.0, (k, m))
                res = g.classify(a, want=("label", "best", "margin"))
                out[prefix + "classify/%d" % k] = sha(res["label"], res["best"], res["margin"])
                res = g.classify(a, ident=rng.uniform(0.5, 1.5, k).astype(np.float32), plane=np.arange(k) % 4 - 1, planes=planes[:3],
                                 bias=rng.normal(0.0, 1.0, k), want=("label", "best", "margin"))
                out[prefix + "classify/%d/ident_bias" % k] = sha(res["label"], res["best"], res["margin"])
            out[prefix + "edges"] = sha(g.edges())
            labels, sums, counts, changed = g.cluster_step(rng.normal(0.0, 0.01, (5, min(m, 64))))
            out[prefix + "cluster_step"] = sha(labels, sums, counts, np.array([changed]))

        g = ctx.graph(img, opt)
        assert g.info["m"] == m
        out["phi"] = sha(g.phi)
        passes(g, "")
        g.compact()                          # every call made once as f32: nothing of it may reach the f16 instances
        passes(g, "f32_then_compact/")
        g.close()
        g = ctx.graph(img, opt)
        g.compact()
        passes(g, "compact/")
        g.close()
        # the changes of basis, each on a fresh handle
        for name in ("transform_full", "transform_cut", "ritz", "cholesky"):
            g = ctx.graph(img, opt)
            if name.startswith("transform"):
                m_new = m if name == "transform_full" else max(1, m - 3)
                g.transform(rng.normal(0.0, 1.0, (m, m_new)) / np.sqrt(m), np.linspace(0.0, 1.0, m_new))
                out[name] = sha(g.phi, g.eigenvalues)
            else:
                st = g.orthonormalize(name, passes=1, verify=True)
                out["orthonormalize/" + name] = sha(g.phi, g.eigenvalues, np.array([st["defect_in"], st["defect_out"]]))
            g.close()
    print(json.dumps(out))


def digest(paths):
    """{file: {group: "cases SHA-256 of the group's sorted 'key hash' lines"}}; a group is a key's shape and, where it has one, its
    f32_then_compact / compact prefix. Two runs agree hash for hash exactly when their digests agree."""
    out = {}
    for path in paths:
        groups = {}
        for key, val in sorted(json.load(open(path)).items()):
            part = key.split("/")
            group = "/".join(part[:2]) if len(part) > 2 and part[1] in ("f32_then_compact", "compact") else part[0]
            groups.setdefault(group, []).append("%s %s" % (key, val))
        out[os.path.basename(path)] = {g: "%d %s" % (len(v), hashlib.sha256("\n".join(v).encode()).hexdigest()) for g, v in groups.items()}
    print(json.dumps(out, indent=1, sort_keys=True))


def main():
    tag, lib_dir = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else None
    out = {}
    for shape in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", tag, lib_dir or "", shape]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=CHILD_SECONDS)
        except subprocess.TimeoutExpired:
            sys.exit("graph_hashes: %s exceeded %d s; nothing more is started" % (shape, CHILD_SECONDS))
        if r.returncode != 0:
            sys.exit("graph_hashes: %s ended with status %d; nothing more is started" % (shape, r.returncode))
        for key, val in json.loads(r.stdout.decode().strip().splitlines()[-1]).items():
            out["%s/%s" % (shape, key)] = val
    json.dump(out, open("graph_hashes_%s.json" % tag, "w"), indent=1, sort_keys=True)
    print(tag, len(out), "cases")
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cluster_hashes.py"), tag] + ([lib_dir] if lib_dir else []), timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired:
        sys.exit("graph_hashes: cluster_hashes.py exceeded %d s" % CHILD_SECONDS)
    sys.exit(r.returncode)


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3] or None, sys.argv[4])
    elif sys.argv[1] == "--digest":
        digest(sys.argv[2:])
    else:
        main()
