#!/usr/bin/env python3
"""Cost of the weighted fit on a graph handle (glf_graph_normal_equations, Graph.fit) against the existing unweighted pieces, on the
benchmark workload.

  python tools/graph_fit_time.py [--size 4096] [--steps 3] [--warmup 1] [--timeout 600] [--out profiles/graph_fit_time_cfg4.json]

bench.py's cfg4 (0.5 % sampling, m = 64, ld = 64) on one GPU, a resident grey graph, in one child process under a time limit (a run
that fails or runs out of time ends there: nothing more is started on the GPU). After a warm-up the calls alternate, `steps` rounds:
normal_equations with 0, 1 and 4 planes, with and without a weight plane; glf_graph_gram on a fresh handle each time (a handle caches
its Gram matrix; only the gram call is timed, not the build) and glf_graph_project for 1 and 4 planes; Graph.fit end to end for 1 and
4 planes. Every call is timed with HIP events on the library's stream and with the host clock; medians, every single time and the
spreads are reported. The yardstick is the weighted call with k planes against gram + project(k), which do strictly less (no
weights). For normal_equations the bytes it must move by construction (Phi once, the weights, the planes) and the flops of the
32 x 32 tiles it computes (the upper triangle: 2 N 1024 tiles) give the achieved fractions of 6.3 TB/s and of the 155 TFLOP/s the
f32 MFMA reaches; the full product's 2 N ld^2 is reported next to it. Prints one JSON line."""
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
MFMA_F32_TFLOPS = 155.0


def _summary(ev, wall):
    return dict(ms_median=round(statistics.median(ev), 3), ms_all=[round(x, 3) for x in ev], ms_spread=round(max(ev) - min(ev), 3),
                wall_ms_median=round(statistics.median(wall), 3), wall_ms_all=[round(x, 3) for x in wall])


def child(size, steps, warmup):
    import numpy as np
    import torch
    import glf

    img = glf.synth_image(size, size, seed=0)
    opt = glf.default_options(num_samples=int(size * size * 0.005), num_eigvals=64, epsilon=0.1)
    n = size * size
    res = dict(device=torch.cuda.get_device_name(0), chain=glf.GRAPH_NORMAL_CHAIN)
    with glf.Context(0) as ctx:
        d = torch.from_numpy(img).to(ctx.device)
        rng = np.random.default_rng(0)
        planes = torch.from_numpy(rng.normal(0.0, 40.0, (4, size, size)).astype(np.float32)).to(ctx.device)
        weight = torch.from_numpy((rng.uniform(size=(size, size)) < 0.3).astype(np.float32)).to(ctx.device)
        sub = {0: None, 1: planes[:1].contiguous(), 4: planes}
        torch.cuda.synchronize()

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(ctx.stream)
            fn()
            e1.record(ctx.stream)
            e1.synchronize()
            return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

        g = ctx.graph(d, opt)
        ld, m = g.info["ld"], g.info["m"]
        res.update(p=g.info["p"], m=m, ld=ld, phi_bytes=g.info["phi_bytes"])
        calls = {}
        for k in (0, 1, 4):
            calls["normal_w_%d" % k] = lambda k=k: g.normal_equations(weight, sub[k])
            calls["normal_now_%d" % k] = lambda k=k: g.normal_equations(None, sub[k])
        for k in (1, 4):
            calls["project_%d" % k] = lambda k=k: g.project(sub[k])
            calls["fit_%d" % k] = lambda k=k: g.fit(sub[k], weight, smooth=0.1, ridge=0.1)
        t = {name: ([], []) for name in list(calls) + ["gram"]}
        for rnd in range(warmup + steps):
            fresh = ctx.graph(d, opt)                                            # (glf_graph_gram caches: a fresh handle each round)
            torch.cuda.synchronize()
            ev, wall = timed(fresh.gram)
            fresh.close()
            if rnd >= warmup:
                t["gram"][0].append(ev)
                t["gram"][1].append(wall)
            for name, fn in calls.items():
                ev, wall = timed(fn)
                if rnd >= warmup:
                    t[name][0].append(ev)
                    t[name][1].append(wall)
        g.close()
    for name in t:
        res[name] = _summary(*t[name])
    ntiles = (ld // 32) * (ld // 32 + 1) // 2
    for k in (0, 1, 4):
        for wname, has_w in (("w", 1), ("now", 0)):
            s = res["normal_%s_%d" % (wname, k)]
            nbytes = n * ld * 4 + has_w * n * 4 + k * n * 4
            flops = 2.0 * n * 1024 * ntiles + 2.0 * n * ld * k
            s.update(bytes=nbytes, gb_per_s=round(nbytes / s["ms_median"] / 1e6, 1), hbm_fraction=round(nbytes / s["ms_median"] / 1e6 / HBM_CEILING_GBS, 3),
                     tile_flops=flops, full_product_flops=2.0 * n * ld * ld, tflops=round(flops / s["ms_median"] / 1e9, 1),
                     mfma_fraction=round(flops / s["ms_median"] / 1e9 / MFMA_F32_TFLOPS, 3))
    # the yardstick: the weighted call with k planes against the unweighted gram + project(k)
    res["yardstick"] = {}
    for k in (1, 4):
        old = res["gram"]["ms_median"] + res["project_%d" % k]["ms_median"]
        spread = res["gram"]["ms_spread"] + res["project_%d" % k]["ms_spread"] + res["normal_w_%d" % k]["ms_spread"]
        new = res["normal_w_%d" % k]["ms_median"]
        res["yardstick"]["planes_%d" % k] = dict(normal_w_ms=new, gram_plus_project_ms=round(old, 3), ratio=round(new / old, 3),
                                                 spread_ms=round(spread, 3), not_slower_beyond_spread=bool(new <= old + spread))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=600, help="seconds for the child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.size, a.steps, a.warmup)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--size", str(a.size), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        sys.exit("graph_fit_time: the run exceeded %d s; nothing more is started" % a.timeout)
    if r.returncode != 0:
        sys.exit("graph_fit_time: the run ended with status %d; nothing more is started" % r.returncode)
    res = dict(size=a.size, steps=a.steps, warmup=a.warmup, grey=json.loads(r.stdout.decode().strip().splitlines()[-1]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
