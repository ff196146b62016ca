#!/usr/bin/env python3
"""Cost of float colour filtering (glf_image_processing_rgbf32) against the 8-bit colour step, on the benchmark workload.

  python tools/rgbf32_time.py [--size 4096] [--steps 3] [--warmup 1] [--out FILE]

One step = one call on a resident synthetic colour image at 0.5 % sampling, m = 64 (bench.py's cfg4): the 8-bit colour step on
tools/rgb_time.py's image (glf_image_processing_rgb) and the float colour step on the same values as float32
(glf_image_processing_rgbf32, the same options: the same graph, bit for bit) alternate within one process after a warm-up, first
with the PIX_BAND key off, then with it on (a context each). Each step is timed with HIP events on the library's stream; the medians
and every single time are reported with both formats' stage times and routes, so the spread of the alternating runs can be read next
to the difference. The float step reads 12 instead of 3 bytes per pixel, one more 16-byte value entry per sample in the
entry-by-entry kernels and three instead of one u32 per sample in the band form's chunk tails, and adds the finite check's one pass
over the image. Prints one JSON line."""
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
    rgb8 = np.stack([grey, np.roll(grey, size // 7, axis=1), 255 - grey], axis=2).copy()
    rgb32 = rgb8.astype(np.float32)
    opt = glf.default_options(num_samples=int(size * size * 0.005), num_eigvals=64, epsilon=0.1)
    keys = ("ms_affinity", "ms_laplacian", "ms_eigen", "ms_nystroem", "ms_filter", "ms_total", "nystroem_kernel_ms")
    res = dict(size=size, steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0))
    for key in ("off", "on"):
        times = {"rgb": [], "rgbf32": []}
        with glf.Context(0) as ctx:
            if key == "on":
                ctx.set_tuning(PIX_BAND="1")
            d_8, d_32 = torch.from_numpy(rgb8).to(ctx.device), torch.from_numpy(rgb32).to(ctx.device)
            torch.cuda.synchronize()

            def step(kind):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ctx.stream)
                if kind == "rgb":
                    _, _, info = ctx.image_processing_rgb(d_8, opt)
                else:
                    _, info = ctx.image_processing_rgbf32(d_32, opt)
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
        med = {k: statistics.median(t) for k, t in times.items()}
        spread = {k: round(max(t) - min(t), 3) for k, t in times.items()}
        res["pix_band_" + key] = dict(
            p=int(infos["rgbf32"]["p"]), m=int(infos["rgbf32"]["m"]),
            ms_median={k: round(v, 3) for k, v in med.items()}, ms_all={k: [round(x, 3) for x in t] for k, t in times.items()},
            ms_spread=spread, rgbf32_minus_rgb_ms=round(med["rgbf32"] - med["rgb"], 3),
            ratio_rgbf32_vs_rgb=round(med["rgbf32"] / med["rgb"], 4),
            same_eigenvalues=bool(np.array_equal(infos["rgbf32"]["eigvals"], infos["rgb"]["eigvals"])),
            rgbf32_stages={k: round(float(infos["rgbf32"][k]), 3) for k in keys}, rgb_stages={k: round(float(infos["rgb"][k]), 3) for k in keys},
            routes={k: dict(nystroem_path=infos[k]["nystroem_path"], matvec_path=infos[k]["matvec_path"], filter_fused=infos[k]["filter_fused"],
                            contraction=infos[k]["contraction"], degree_evaluated=infos[k]["degree_evaluated"],
                            nystroem_evaluated=infos[k]["nystroem_evaluated"]) for k in times})
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
