"""SHA-256 of what one Lloyd iteration writes (labels, sums, counts, mass, changed) on the shapes tiny, ld32, ld64 and ld256 of
tests/test_gpu_graph.py, k in (1, 5, 32), with and without prev, in the modes plain, weight, normalize and both (plus the plain step
through glf_graph_cluster_step itself), and of the labels, centroids and iteration count of one segment and one
segment(normalize, weight) run on ld64: whether a change left the bits of the spectral segmentation alone. Run it once per build and
compare the two files:
    python tools/cluster_hashes.py new                # this tree's glf.py and libglf.so -> cluster_hashes_new.json in the current directory
    python tools/cluster_hashes.py parent DIR         # DIR holds another commit's glf.py and libglf.so -> cluster_hashes_parent.json"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # (tools/ sits under the repository root)
tag = sys.argv[1]
if len(sys.argv) > 2:
    os.environ["GLF_LIBRARY"] = os.path.join(sys.argv[2], "libglf.so")
    sys.path.insert(0, sys.argv[2])
else:
    sys.path.insert(0, os.path.join(ROOT, "image-processing-graph-laplacian_amd"))
import numpy as np
import torch
import glf
print("library:", glf.LIB_PATH)
SHAPES = {"tiny": (16, 10, 12, 4), "ld32": (61, 47, 100, 8), "ld64": (61, 47, 100, 40), "ld256": (61, 47, 200, 200)}  # width, height, samples, m
MODES = {"plain": dict(), "weight": dict(weight=True), "normalize": dict(normalize=True), "both": dict(normalize=True, weight=True)}


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a).tobytes())
    return h.hexdigest()


out = {}
with glf.Context(0) as ctx:
    for shape, (w, h, ns, m) in SHAPES.items():
        g = ctx.graph(ctx.to_device(glf.synth_image(w, h, seed=3)), glf.default_options(num_samples=ns, num_eigvals=m, epsilon=0.1))
        assert g.info["m"] == m
        n, dim = w * h, min(m, 64)
        rng = np.random.default_rng([5, list(SHAPES).index(shape)])
        weight = torch.from_numpy(rng.uniform(0.0, 2.0, (h, w)).astype(np.float32)).to(ctx.device)
        scale = rng.uniform(0.5, 2.0, dim)
        for k in (1, 5, 32):
            raw = g.phi[torch.from_numpy(rng.choice(n, size=k, replace=False)).to(ctx.device), :dim].double().cpu().numpy() * scale[None]
            unit = raw / np.maximum(np.sqrt((raw * raw).sum(axis=1)), 1e-300)[:, None]
            prev = torch.from_numpy(rng.integers(0, k, size=(h, w)).astype(np.int32)).to(ctx.device)
            for with_prev in (0, 1):
                kw = dict(prev=prev) if with_prev else dict()
                key = "%s/k%d/prev%d/" % (shape, k, with_prev)
                labels, sums, counts, changed = g.cluster_step(raw, scale, **kw)
                out[key + "step"] = dict(labels=sha(labels), sums=sha(sums), counts=sha(counts), changed=changed)
                for mode, emb in MODES.items():
                    labels, sums, counts, mass, changed = g.cluster_step_ex(unit if emb.get("normalize") else raw, scale, normalize=bool(emb.get("normalize")),
                                                                            weight=weight if emb.get("weight") else None, **kw)
                    out[key + mode] = dict(labels=sha(labels), sums=sha(sums), counts=sha(counts), mass=sha(mass), changed=changed)
        if shape == "ld64":
            labels, cent, st = g.segment(5, seed=7)
            out["ld64/segment"] = dict(labels=sha(labels), cent=sha(cent), iterations=st["iterations"])
            labels, cent, st = g.segment(5, dim=m, seed=7, normalize=True, weight=weight)
            out["ld64/segment_normalize_weight"] = dict(labels=sha(labels), cent=sha(cent), mass=sha(st["mass"]), iterations=st["iterations"])
        g.close()
json.dump(out, open("cluster_hashes_%s.json" % tag, "w"), indent=1, sort_keys=True)
print(tag, len(out), "cases")
