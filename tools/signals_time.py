#!/usr/bin/env python3
"""Cost of joint filtering (glf_image_processing_signals) against the plain step, on the benchmark workload.

  python tools/signals_time.py [--size 4096] [--steps 10] [--warmup 3] [--out FILE]

One step = one call on a resident 4096 x 4096 synthetic image at 0.5 % sampling, m = 64 (bench.py's cfg4), with nsig = 0
(glf_image_processing), 1 or 2 float planes. The three variants alternate within one process after a warm-up; each step is
timed with HIP events on the library's stream and the median of the steps is reported. Prints one JSON line."""
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import glf

    size = a.size
    img = glf.synth_image(size, size, seed=0)
    rng = np.random.default_rng(0)
    opt = glf.default_options(num_samples=int(size * size * 0.005), num_eigvals=64, epsilon=0.1)
    times = {0: [], 1: [], 2: []}
    with glf.Context(0) as ctx:
        d_img = ctx.to_device(img)
        sig = torch.from_numpy(rng.normal(0.0, 40.0, (2, size, size)).astype(np.float32)).to(ctx.device)
        planes = {1: sig[:1].contiguous(), 2: sig}
        torch.cuda.synchronize()

        def step(nsig):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ctx.stream)
            if nsig == 0:
                _, _, info = ctx.image_processing(d_img, opt)
            else:
                _, _, _, info = ctx.image_processing_signals(d_img, planes[nsig], opt)
            e1.record(ctx.stream)
            e1.synchronize()
            return e0.elapsed_time(e1), info

        for _ in range(a.warmup):
            for n in (0, 1, 2):
                step(n)
        fused = {}
        for _ in range(a.steps):
            for n in (0, 1, 2):
                ms, info = step(n)
                times[n].append(ms)
                fused[n] = info["filter_fused"]
    med = {n: statistics.median(t) for n, t in times.items()}
    res = dict(size=size, p=int(info["p"]), m=int(info["m"]), steps=a.steps, warmup=a.warmup,
               ms_median={str(n): round(med[n], 3) for n in med}, ms_all={str(n): [round(x, 3) for x in t] for n, t in times.items()},
               ratio_vs_plain={str(n): round(med[n] / med[0], 3) for n in (1, 2)}, guide_filter_fused=fused,
               device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
