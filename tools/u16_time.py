#!/usr/bin/env python3
"""Cost of 16-bit greyscale filtering (glf_image_processing_u16) against the grey step, on the benchmark workload.

  python tools/u16_time.py [--size 4096] [--steps 3] [--warmup 1] [--out FILE]

One step = one call on a resident synthetic image at 0.5 % sampling, m = 64 (bench.py's cfg4): the grey step on the 8-bit image
(glf_image_processing) and the 16-bit step on 257 times it plus a sub-level pattern (glf_image_processing_u16 at h_val 30 * 257,
the same graph scale) alternate within one process after a warm-up; each step is timed with HIP events on the library's stream and
the median is reported with the 16-bit step's stage times and routes. Prints one JSON line."""
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
    # 16-bit: the grey image at 257 x plus a pattern below one 8-bit level
    r, c = np.mgrid[0:size, 0:size]
    img16 = (grey.astype(np.int64) * 257 + (r * 7 + c * 3) % 200).clip(0, 65535).astype(np.uint16)
    opt = glf.default_options(num_samples=int(size * size * 0.005), num_eigvals=64, epsilon=0.1)
    opt16 = glf.default_options(num_samples=int(size * size * 0.005), num_eigvals=64, epsilon=0.1, h_val=30.0 * 257.0)
    times = {"grey": [], "u16": []}
    keys = ("ms_affinity", "ms_laplacian", "ms_eigen", "ms_nystroem", "ms_filter", "ms_total", "nystroem_kernel_ms")
    with glf.Context(0) as ctx:
        d_grey, d_16 = ctx.to_device(grey), torch.from_numpy(img16).to(ctx.device)
        torch.cuda.synchronize()

        def step(kind):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ctx.stream)
            if kind == "grey":
                _, _, info = ctx.image_processing(d_grey, opt)
            else:
                _, _, info = ctx.image_processing_u16(d_16, opt16)
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
    res = dict(size=size, p=int(infos["u16"]["p"]), m=int(infos["u16"]["m"]), steps=a.steps, warmup=a.warmup,
               ms_median={k: round(v, 3) for k, v in med.items()}, ms_all={k: [round(x, 3) for x in t] for k, t in times.items()},
               ratio_u16_vs_grey=round(med["u16"] / med["grey"], 3),
               u16_stages={k: round(float(infos["u16"][k]), 3) for k in keys},
               grey_stages={k: round(float(infos["grey"][k]), 3) for k in keys},
               u16_routes=dict(nystroem_path=infos["u16"]["nystroem_path"], matvec_path=infos["u16"]["matvec_path"],
                               filter_fused=infos["u16"]["filter_fused"], contraction=infos["u16"]["contraction"],
                               degree_evaluated=infos["u16"]["degree_evaluated"], nystroem_evaluated=infos["u16"]["nystroem_evaluated"]),
               grey_routes=dict(nystroem_path=infos["grey"]["nystroem_path"], matvec_path=infos["grey"]["matvec_path"],
                                filter_fused=infos["grey"]["filter_fused"]),
               device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
