#!/usr/bin/env python3
"""Cost of the band form of the 16-bit and colour kernels (tuning key PIX_BAND) against the entry-by-entry route and the grey step.

  python tools/pix_band_time.py [--size 4096] [--steps 3] [--warmup 1] [--out FILE]

One step = one call on a resident synthetic image at 0.5 % sampling, m = 64 (bench.py's cfg4). Five kinds of step alternate within
one process and one context after a warm-up: the grey step (glf_image_processing), the 16-bit step with the key off and with it on
(glf_image_processing_u16 on tools/u16_time.py's image), and the same pair for colour (glf_image_processing_rgb on
tools/rgb_time.py's image); the key is switched with glf_ctx_set_tuning between steps. Each step is timed with HIP events on the
library's stream. Reported: the median step, the median of every stage time, the stage sum the form was built for (eigen-solve +
Nystroem + Laplacian, key on against key off), the band kernels' own times (the Nystroem launch; one operator sweep = the
eigen-solve's sweep time over its sweeps, chunk preparation included) next to the grey ones, and the routes. Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-processing-graph-laplacian_amd"))

KINDS = ("grey", "u16_off", "u16_on", "rgb_off", "rgb_on")
STAGES = ("ms_affinity", "ms_laplacian", "ms_eigen", "ms_nystroem", "ms_filter", "ms_total", "nystroem_kernel_ms")


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
    r, c = np.mgrid[0:size, 0:size]
    img16 = (grey.astype(np.int64) * 257 + (r * 7 + c * 3) % 200).clip(0, 65535).astype(np.uint16)
    rgb = np.stack([grey, np.roll(grey, size // 7, axis=1), 255 - grey], axis=2).copy()
    base = dict(num_samples=int(size * size * 0.005), num_eigvals=64, epsilon=0.1)
    opt, opt16 = glf.default_options(**base), glf.default_options(h_val=30.0 * 257.0, **base)
    times = {k: [] for k in KINDS}
    infos = {k: [] for k in KINDS}
    with glf.Context(0) as ctx:
        d_grey, d_16, d_rgb = ctx.to_device(grey), torch.from_numpy(img16).to(ctx.device), torch.from_numpy(rgb).to(ctx.device)
        torch.cuda.synchronize()

        def step(kind):
            ctx.set_tuning(PIX_BAND="1" if kind.endswith("_on") else None)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ctx.stream)
            if kind == "grey":
                _, _, info = ctx.image_processing(d_grey, opt)
            elif kind.startswith("u16"):
                _, _, info = ctx.image_processing_u16(d_16, opt16)
            else:
                _, _, info = ctx.image_processing_rgb(d_rgb, opt)
            e1.record(ctx.stream)
            e1.synchronize()
            return e0.elapsed_time(e1), info

        for _ in range(a.warmup):
            for k in KINDS:
                step(k)
        for _ in range(a.steps):
            for k in KINDS:
                ms, info = step(k)
                times[k].append(ms)
                infos[k].append(info)

    def med(kind, key):
        return statistics.median(float(i[key]) for i in infos[kind])

    def three(kind):  # the stages the band form replaces
        return statistics.median(float(i["ms_eigen"]) + float(i["ms_nystroem"]) + float(i["ms_laplacian"]) for i in infos[kind])

    last = {k: infos[k][-1] for k in KINDS}
    res = dict(size=size, p=int(last["u16_on"]["p"]), m=int(last["u16_on"]["m"]), steps=a.steps, warmup=a.warmup,
               ms_median={k: round(statistics.median(t), 3) for k, t in times.items()},
               ms_all={k: [round(x, 3) for x in t] for k, t in times.items()},
               stages_median={k: {s: round(med(k, s), 3) for s in STAGES} for k in KINDS},
               eigen_nystroem_laplacian_ms={k: round(three(k), 3) for k in KINDS},
               ratio_off_over_on=dict(u16=round(three("u16_off") / three("u16_on"), 2), rgb=round(three("rgb_off") / three("rgb_on"), 2)),
               band_kernels_ms={k: dict(nystroem_launch=round(med(k, "nystroem_kernel_ms"), 3),
                                        operator_sweep=round(med(k, "matvec_ms") / max(1.0, med(k, "matvecs")), 4),
                                        sweeps=int(med(k, "matvecs")))
                                for k in ("grey", "u16_on", "rgb_on")},
               routes={k: dict(nystroem_path=last[k]["nystroem_path"], matvec_path=last[k]["matvec_path"], filter_fused=last[k]["filter_fused"],
                               contraction=last[k]["contraction"], outer_its=last[k]["outer_its"], nystroem_evaluated=last[k]["nystroem_evaluated"])
                       for k in KINDS},
               device=torch.cuda.get_device_name(0))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
