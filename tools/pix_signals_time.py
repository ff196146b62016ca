#!/usr/bin/env python3
"""Cost of joint filtering under a 16-bit or a colour guide (glf_image_processing_u16_signals / _rgb_signals) against the plain step.

  python tools/pix_signals_time.py [--size 4096] [--steps 5] [--warmup 1] [--out FILE] [--only u16_4]

One step = one call on a resident synthetic image at 0.5 % sampling, m = 64 (bench.py's cfg4) with the PIX_BAND tuning key, for
each format with nsig = 0 (the plain glf_image_processing_u16 / _rgb call: the baseline), 1, 2 and 4 float planes. The eight
variants alternate within one process and one context after a warm-up. Reported: the medians of the library's ms_total and
ms_filter (the filter stage is where the planes ride) and of the step timed with HIP events on the library's stream, the
increments over the format's nsig = 0 step, and the routes. --only runs one variant alone (one call under a kernel trace). Prints
one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-processing-graph-laplacian_amd"))

NSIGS = (0, 1, 2, 4)
KINDS = tuple("%s_%d" % (f, n) for f in ("u16", "rgb") for n in NSIGS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default=None, choices=KINDS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import glf

    size = a.size
    kinds = (a.only,) if a.only else KINDS
    grey = glf.synth_image(size, size, seed=0)
    r, c = np.mgrid[0:size, 0:size]
    img16 = (grey.astype(np.int64) * 257 + (r * 7 + c * 3) % 200).clip(0, 65535).astype(np.uint16)   # tools/pix_band_time.py's images
    rgb = np.stack([grey, np.roll(grey, size // 7, axis=1), 255 - grey], axis=2).copy()
    base = dict(num_samples=int(size * size * 0.005), num_eigvals=64, epsilon=0.1)
    opts = dict(u16=glf.default_options(h_val=30.0 * 257.0, **base), rgb=glf.default_options(**base))
    times = {k: [] for k in kinds}
    infos = {k: [] for k in kinds}
    with glf.Context(0) as ctx:
        ctx.set_tuning(PIX_BAND="1")
        d_img = dict(u16=torch.from_numpy(img16).to(ctx.device), rgb=torch.from_numpy(rgb).to(ctx.device))
        depth = (1000.0 + 400.0 * ((r - size / 2) ** 2 + (c - size / 3) ** 2 < (size / 4) ** 2)).astype(np.float32)
        sig = torch.empty((4, size, size), dtype=torch.float32, device=ctx.device)
        sig[0] = torch.from_numpy(depth).to(ctx.device)
        sig[1:].normal_(0.0, 40.0, generator=torch.Generator(device=ctx.device).manual_seed(0))
        planes = {n: sig[:n].contiguous() for n in NSIGS if n}
        del r, c, depth
        torch.cuda.synchronize()

        def step(kind):
            fmt, n = kind.split("_")[0], int(kind.split("_")[1])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ctx.stream)
            if n == 0:
                info = (ctx.image_processing_u16 if fmt == "u16" else ctx.image_processing_rgb)(d_img[fmt], opts[fmt])[2]
            else:
                info = (ctx.image_processing_u16_signals if fmt == "u16" else ctx.image_processing_rgb_signals)(d_img[fmt], planes[n], opts[fmt])[3]
            e1.record(ctx.stream)
            e1.synchronize()
            return e0.elapsed_time(e1), info

        for _ in range(a.warmup):
            for k in kinds:
                step(k)
        for _ in range(a.steps):
            for k in kinds:
                ms, info = step(k)
                times[k].append(ms)
                infos[k].append(info)

    def med(kind, key):
        return statistics.median(float(i[key]) for i in infos[kind])

    last = {k: infos[k][-1] for k in kinds}
    res = dict(size=size, p=int(last[kinds[0]]["p"]), m=int(last[kinds[0]]["m"]), steps=a.steps, warmup=a.warmup,
               ms_total_median={k: round(med(k, "ms_total"), 3) for k in kinds},
               ms_filter_median={k: round(med(k, "ms_filter"), 3) for k in kinds},
               ms_step_median={k: round(statistics.median(times[k]), 3) for k in kinds},
               ms_filter_all={k: [round(float(i["ms_filter"]), 3) for i in infos[k]] for k in kinds},
               routes={k: (last[k]["nystroem_path"], last[k]["matvec_path"], last[k]["filter_fused"]) for k in kinds},
               device=torch.cuda.get_device_name(0))
    if not a.only:
        res["increment_over_nsig0_ms"] = {
            k: dict(ms_total=round(med(k, "ms_total") - med(k.split("_")[0] + "_0", "ms_total"), 3),
                    ms_filter=round(med(k, "ms_filter") - med(k.split("_")[0] + "_0", "ms_filter"), 3))
            for k in kinds if not k.endswith("_0")}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
