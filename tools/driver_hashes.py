"""SHA-256 of the u8 and float outputs of every E2E case of tests/test_gpu_parity.py under the four forced paths, both contraction modes
and skip_exact_zeros 0 / 1 (80 runs), with matvec_path, outer iterations and sweep count: whether a change left the whole-path
driver's bits alone. Run it once per build and compare the two files:
    python tools/driver_hashes.py new                 # this tree's glf.py and libglf.so -> hash_new.json in the current directory
    python tools/driver_hashes.py parent DIR          # DIR holds another commit's glf.py and libglf.so -> hash_parent.json"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # (tools/ sits under the repository root)
tag = sys.argv[1]
if len(sys.argv) > 2:
    os.environ["GLF_LIBRARY"] = os.path.join(sys.argv[2], "libglf.so")
    sys.path.insert(0, sys.argv[2])
else:
    sys.path.insert(0, os.path.join(ROOT, "image-processing-graph-laplacian_amd"))
import numpy as np
from PIL import Image
import glf
print("library:", glf.LIB_PATH, "operator entry:", hasattr(glf._lib, "glf_operator_create"))
G = os.path.join(ROOT, "tests", "golden")
imgs = {"syn32": np.load(os.path.join(G, "syn32.npz"))["img"], "test": np.array(Image.open(os.path.join(G, "test.png"))),
        "ragged": glf.synth_image(53, 37, seed=3), "cat50": np.array(Image.open(os.path.join(G, "cat_small.png")))}
E2E = [("syn32", 10, 4, 1e-3), ("test", 100, 16, 0.1), ("test", 100, 99, 0.1), ("ragged", 20, 5, 0.1), ("cat50", 50, 53, 0.1)]
out = {}
for mode in ("f16s", "f32"):
    with glf.Context(0) as ctx:
        ctx.set_contraction(glf.CONTRACT_F16_SPLIT if mode == "f16s" else glf.CONTRACT_F32_MFMA)
        for paths in ("direct", "grid", "rank", "band"):
            ctx.reset_tuning()
            ctx.set_tuning(NYS_PATH=paths, DEG_PATH="direct" if paths == "direct" else "grid",
                           MV_PATH={"direct": "dense", "grid": "grid", "rank": "rank", "band": "band"}[paths])
            for name, ns, m, eps in E2E:
                for skip in (0, 1):
                    opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=eps, skip_exact_zeros=skip)
                    o, zf, info = ctx.image_processing(ctx.to_device(imgs[name]), opt, want_float=True)
                    key = "%s/%s/%s-%d-%d/skip%d" % (mode, paths, name, ns, m, skip)
                    out[key] = dict(u8=hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest(), zf=hashlib.sha256(zf.cpu().numpy().tobytes()).hexdigest(),
                                    matvec_path=info["matvec_path"], outer_its=info["outer_its"], matvecs=info["matvecs"])
json.dump(out, open("hash_%s.json" % tag, "w"), indent=1, sort_keys=True)
print(tag, len(out), "cases")
