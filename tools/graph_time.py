#!/usr/bin/env python3
"""Cost of the graph handle (glf_graph_build / _project / _synthesize) against the plain call, on the benchmark workload.

  python tools/graph_time.py [--size 4096] [--steps 3] [--warmup 1] [--timeout 300] [--out profiles/graph_time_cfg4.json]

bench.py's cfg4 (0.5 % sampling, m = 64, ld = 64) on one GPU, for a grey 8-bit image and for an 8-bit colour image with the
PIX_BAND key. Each format is measured in a child process of its own under a time limit (a format that fails or runs out of time ends
the run: nothing more is started on the GPU). In the child, after a warm-up, the plain call and glf_graph_build alternate; then
glf_graph_project runs for 1 and 4 planes and glf_graph_synthesize for 1, 8 and 32 outputs on 2 planes (into a preallocated
output, so that no fill is timed). Every step is timed with HIP events on the library's stream and with the host clock; medians,
every single time and the spreads are reported. For project and synthesize the bytes each must move by construction -- Phi once,
the planes read, the outputs written -- and the rate they give are reported next to the 6.3 TB/s the device streams at best, and
t(32 outputs) / t(1 output) next to the ratio of those byte counts. Prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-processing-graph-laplacian_amd"))
HBM_CEILING_GBS = 6300.0


def _summary(ev, wall):
    return dict(ms_median=round(statistics.median(ev), 3), ms_all=[round(x, 3) for x in ev], ms_spread=round(max(ev) - min(ev), 3),
                wall_ms_median=round(statistics.median(wall), 3), wall_ms_all=[round(x, 3) for x in wall])


def child(fmt, size, steps, warmup):
    import ctypes as C

    import numpy as np
    import torch
    import glf

    grey = glf.synth_image(size, size, seed=0)
    img = grey if fmt == "grey" else np.stack([grey, np.roll(grey, size // 7, axis=1), 255 - grey], axis=2).copy()   # tools/rgb_time.py's image
    opt = glf.default_options(num_samples=int(size * size * 0.005), num_eigvals=64, epsilon=0.1)
    n = size * size
    res = dict(format=fmt, pix_band=fmt != "grey", device=torch.cuda.get_device_name(0))
    with glf.Context(0) as ctx:
        if fmt != "grey":
            ctx.set_tuning(PIX_BAND="1")
        d = torch.from_numpy(img).to(ctx.device)
        rng = np.random.default_rng(0)
        planes = torch.from_numpy(rng.normal(0.0, 40.0, (4, size, size)).astype(np.float32)).to(ctx.device)
        torch.cuda.synchronize()

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(ctx.stream)
            r = fn()
            e1.record(ctx.stream)
            e1.synchronize()
            return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, r

        def plain():
            return (ctx.image_processing(d, opt) if fmt == "grey" else ctx.image_processing_rgb(d, opt))[-1]

        def build():
            g = ctx.graph(d, opt)
            stats = g.stats
            g.close()
            return stats

        for _ in range(warmup):
            plain()
            build()
        t = {"plain": ([], [], []), "build": ([], [], [])}
        last = {}
        for _ in range(steps):
            for name, fn in (("plain", plain), ("build", build)):
                ev, wall, info = timed(fn)
                t[name][0].append(ev)
                t[name][1].append(wall)
                t[name][2].append(float(info["ms_total"]))
                last[name] = info
        for name in t:
            res[name] = _summary(t[name][0], t[name][1])
            res[name]["stats_ms_total_median"] = round(statistics.median(t[name][2]), 3)
            res[name]["route"] = {k: last[name][k] for k in ("nystroem_path", "matvec_path", "filter_fused")}
        g = ctx.graph(d, opt)
        ld, m = g.info["ld"], g.info["m"]
        res.update(p=g.info["p"], m=m, ld=ld, phi_bytes=g.info["phi_bytes"])
        lam = g.eigenvalues
        for nplanes in (1, 4):
            sub = planes[:nplanes].contiguous()
            for _ in range(warmup):
                g.project(sub)
            runs = [timed(lambda: g.project(sub)) for _ in range(steps)]
            nbytes = n * ld * 4 + nplanes * n * 4
            s = _summary([r[0] for r in runs], [r[1] for r in runs])
            s.update(bytes=nbytes, gb_per_s=round(nbytes / s["ms_median"] / 1e6, 1), ceiling_gb_per_s=HBM_CEILING_GBS)
            res["project_%d" % nplanes] = s
        two = planes[:2].contiguous()
        c = g.project(two)
        out = torch.empty((32, size, size), dtype=torch.float32, device=ctx.device)
        torch.cuda.synchronize()
        for nout in (1, 8, 32):
            a = np.ascontiguousarray(np.stack([(0.5 + j) * lam * c[j % 2] for j in range(nout)]))
            ident = np.ones(nout, dtype=np.float32)
            plane = np.array([j % 2 for j in range(nout)], dtype=np.int32)

            def synth():
                rc = glf._lib.glf_graph_synthesize(g._g, nout, glf._ptr(a), glf._ptr(ident), glf._ptr(plane), 2, C.c_void_p(two.data_ptr()),
                                                   C.c_void_p(out.data_ptr()))
                assert rc == glf.OK, rc

            for _ in range(warmup):
                synth()
            runs = [timed(synth) for _ in range(steps)]
            nbytes = n * ld * 4 + min(nout, 2) * n * 4 + nout * n * 4
            s = _summary([r[0] for r in runs], [r[1] for r in runs])
            s.update(bytes=nbytes, gb_per_s=round(nbytes / s["ms_median"] / 1e6, 1), ceiling_gb_per_s=HBM_CEILING_GBS)
            res["synthesize_%d" % nout] = s
        g.close()
    res["synthesize_32_over_1"] = dict(time_ratio=round(res["synthesize_32"]["ms_median"] / res["synthesize_1"]["ms_median"], 3),
                                       bytes_ratio=round(res["synthesize_32"]["bytes"] / res["synthesize_1"]["bytes"], 3))
    # k variants of a filter on one plane: one build + k (project + synthesize) against k plain calls
    per = res["project_1"]["ms_median"] + res["synthesize_1"]["ms_median"]
    res["variants"] = dict(per_variant_ms=round(per, 3), build_ms=res["build"]["ms_median"], plain_ms=res["plain"]["ms_median"],
                           crossover_k=round(res["build"]["ms_median"] / max(res["plain"]["ms_median"] - per, 1e-9), 2))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=300, help="seconds for each format's child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.size, a.steps, a.warmup)
    res = dict(size=a.size, steps=a.steps, warmup=a.warmup)
    for fmt in ("grey", "rgb"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", fmt, "--size", str(a.size), "--steps", str(a.steps), "--warmup", str(a.warmup)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            sys.exit("graph_time: the %s run exceeded %d s; nothing more is started" % (fmt, a.timeout))
        if r.returncode != 0:
            sys.exit("graph_time: the %s run ended with status %d; nothing more is started" % (fmt, r.returncode))
        res[fmt] = json.loads(r.stdout.decode().strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
