#!/usr/bin/env python3
"""Cost of colour-guided filtering (glf_image_processing_rgb) against the grey step, on the benchmark workload.

  python tools/rgb_time.py [--size 4096] [--steps 3] [--warmup 1] [--out FILE]

One step = one call on a resident synthetic image at 0.5 % sampling, m = 64 (bench.py's cfg4): the grey step on the luma
(glf_image_processing) and the colour step on the RGB image (glf_image_processing_rgb) alternate within one process after a
warm-up; each step is timed with HIP events on the library's stream and the median is reported with the colour step's stage
times and routes. One more grey step with the windowed direct degree (DEG_PATH=direct) times that degree sweep on its own.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-processing-graph-laplacian_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import glf

    size = a.size
    grey = glf.synth_image(size, size, seed=0)
    # colour: the grey image's noise on three differently shifted channels
    rgb = np.stack([grey, np.roll(grey, size // 7, axis=1), 255 - grey], axis=2).copy()
    luma = np.clip(np.floor(rgb.astype(np.float64) @ np.array([0.299, 0.587, 0.114]) + 0.5), 0, 255).astype(np.uint8)
    opt = glf.default_options(num_samples=int(size * size * 0.005), num_eigvals=64, epsilon=0.1)
    times = {"grey": [], "rgb": []}
    keys = ("ms_affinity", "ms_laplacian", "ms_eigen", "ms_nystroem", "ms_filter", "ms_total", "nystroem_kernel_ms")
    with glf.Context(0) as ctx:
        d_luma, d_rgb = ctx.to_device(luma), torch.from_numpy(rgb).to(ctx.device)
        torch.cuda.synchronize()

        def step(kind):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ctx.stream)
            if kind == "grey":
                _, _, info = ctx.image_processing(d_luma, opt)
            else:
                _, _, info = ctx.image_processing_rgb(d_rgb, opt)
            e1.record(ctx.stream)
            e1.synchronize()
            return e0.elapsed_time(e1), info

        for _ in range(a.warmup):
            for k in times:
                step(k)
        infos = {}
        for _ in range(a.steps):
            for k in times:
                ms, infos[k] = step(k)
                times[k].append(ms)
        ctx.set_tuning(DEG_PATH="direct")
        _, deg_direct = step("grey")
    med = {k: statistics.median(t) for k, t in times.items()}
    res = dict(size=size, p=int(infos["rgb"]["p"]), m=int(infos["rgb"]["m"]), steps=a.steps, warmup=a.warmup,
               ms_median={k: round(v, 3) for k, v in med.items()}, ms_all={k: [round(x, 3) for x in t] for k, t in times.items()},
               ratio_rgb_vs_grey=round(med["rgb"] / med["grey"], 3),
               rgb_stages={k: round(float(infos["rgb"][k]), 3) for k in keys},
               grey_stages={k: round(float(infos["grey"][k]), 3) for k in keys},
               rgb_routes=dict(nystroem_path=infos["rgb"]["nystroem_path"], matvec_path=infos["rgb"]["matvec_path"],
                               filter_fused=infos["rgb"]["filter_fused"], contraction=infos["rgb"]["contraction"],
                               degree_evaluated=infos["rgb"]["degree_evaluated"], nystroem_evaluated=infos["rgb"]["nystroem_evaluated"]),
               grey_routes=dict(nystroem_path=infos["grey"]["nystroem_path"], matvec_path=infos["grey"]["matvec_path"],
                                filter_fused=infos["grey"]["filter_fused"]),
               grey_direct_degree_ms_affinity=round(float(deg_direct["ms_affinity"]), 3),
               device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
