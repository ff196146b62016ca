#!/usr/bin/env python3
"""Cost of the wide projection on a graph handle (glf_graph_project_wide) against the existing calls that do the same work, on the
benchmark workload.

  python tools/graph_project_wide_time.py [--size 4096] [--eigvals 64] [--steps 3] [--warmup 1] [--timeout 900]
                                          [--out profiles/graph_project_wide_time_cfg4.json] [--merge-into FILE --key NAME]

bench.py's cfg4 (0.5 % sampling, m = ld = 64 at 4096 x 4096) on one GPU, a resident grey graph, in one child process under a time limit
(a run that fails or runs out of time ends there: nothing more is started on the GPU). After a warm-up the calls alternate, `steps`
rounds: project_wide at 1, 4, 8, 16 and 32 planes, with and without a weight plane; as yardsticks ceil(k / 4) calls of
glf_graph_project(4) (the planes in chunks of four; k = 1: one call of one plane), glf_graph_normal_equations with 4 planes, and
planes.view(k, N) @ phi in torch f32 on the same Phi. Every call is timed with HIP events on the library's stream (the torch product on
the same stream) and with the host clock; medians, every single time and the spreads are reported. For project_wide the bytes it must
move by construction (Phi once, the planes and the weights once per column group of 128) and the 2 N ld 32 flops the MFMAs issue give
the achieved fractions of 6.3 TB/s and of the 155 TFLOP/s the f32 MFMA reaches. --eigvals 256 --size 2048 is the m = ld = 256 run;
--merge-into adds this run's result under --key to an existing JSON file. Prints one JSON line."""
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
PLANES = (1, 4, 8, 16, 32)


def _summary(ev, wall):
    return dict(ms_median=round(statistics.median(ev), 3), ms_all=[round(x, 3) for x in ev], ms_spread=round(max(ev) - min(ev), 3),
                wall_ms_median=round(statistics.median(wall), 3), wall_ms_all=[round(x, 3) for x in wall])


def child(size, eigvals, steps, warmup):
    import numpy as np
    import torch
    import glf

    img = glf.synth_image(size, size, seed=0)
    opt = glf.default_options(num_samples=int(size * size * 0.005), num_eigvals=eigvals, epsilon=0.1)
    n = size * size
    res = dict(device=torch.cuda.get_device_name(0), chain=glf.GRAPH_NORMAL_CHAIN)
    with glf.Context(0) as ctx:
        d = torch.from_numpy(img).to(ctx.device)
        gen = torch.Generator(device=ctx.device)
        gen.manual_seed(0)
        planes = torch.randn((32, size, size), generator=gen, device=ctx.device, dtype=torch.float32) * 40.0
        weight = (torch.rand((size, size), generator=gen, device=ctx.device) < 0.3).float()
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

        def chunked(k):
            for k0 in range(0, k, 4):
                g.project(planes[k0:min(k0 + 4, k)])

        def torch_f32(k):
            with torch.cuda.stream(ctx.stream):
                return planes[:k].view(k, n) @ g.phi

        calls = {}
        for k in PLANES:
            calls["wide_w_%d" % k] = lambda k=k: g.project_wide(planes[:k], weight)
            calls["wide_now_%d" % k] = lambda k=k: g.project_wide(planes[:k])
            calls["project4_chunks_%d" % k] = lambda k=k: chunked(k)
            calls["torch_f32_%d" % k] = lambda k=k: torch_f32(k)
        calls["normal_w_4"] = lambda: g.normal_equations(weight, planes[:4])
        t = {name: ([], []) for name in calls}
        for rnd in range(warmup + steps):
            for name, fn in calls.items():
                ev, wall = timed(fn)
                if rnd >= warmup:
                    t[name][0].append(ev)
                    t[name][1].append(wall)
        g.close()
    for name in t:
        res[name] = _summary(*t[name])
    groups = max(1, ld // 128)
    for k in PLANES:
        for wname, has_w in (("w", 1), ("now", 0)):
            s = res["wide_%s_%d" % (wname, k)]
            nbytes = n * ld * 4 + groups * (has_w + k) * n * 4
            flops = 2.0 * n * ld * 32
            s.update(bytes=nbytes, gb_per_s=round(nbytes / s["ms_median"] / 1e6, 1), hbm_fraction=round(nbytes / s["ms_median"] / 1e6 / HBM_CEILING_GBS, 3),
                     mfma_flops=flops, useful_flops=2.0 * n * ld * k, tflops=round(flops / s["ms_median"] / 1e9, 1),
                     mfma_fraction=round(flops / s["ms_median"] / 1e9 / MFMA_F32_TFLOPS, 3))
    # the yardsticks: the wide call with k planes (no weight) against ceil(k / 4) project(4) calls and against the torch f32 product
    res["yardstick"] = {}
    for k in PLANES:
        new, old, tf = res["wide_now_%d" % k], res["project4_chunks_%d" % k], res["torch_f32_%d" % k]
        spread = new["ms_spread"] + old["ms_spread"]
        res["yardstick"]["planes_%d" % k] = dict(wide_ms=new["ms_median"], project4_chunks_ms=old["ms_median"], torch_f32_ms=tf["ms_median"],
                                                 ratio_to_chunks=round(new["ms_median"] / old["ms_median"], 3),
                                                 ratio_to_torch_f32=round(new["ms_median"] / tf["ms_median"], 3), spread_ms=round(spread, 3),
                                                 faster_beyond_spread=bool(new["ms_median"] + spread < old["ms_median"]))
    res["yardstick"]["weighted_4"] = dict(wide_w_ms=res["wide_w_4"]["ms_median"], normal_w_ms=res["normal_w_4"]["ms_median"],
                                          ratio=round(res["wide_w_4"]["ms_median"] / res["normal_w_4"]["ms_median"], 3))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--eigvals", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=900, help="seconds for the child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-into", default=None, help="an existing JSON file that receives this run under --key")
    ap.add_argument("--key", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.size, a.eigvals, a.steps, a.warmup)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--size", str(a.size), "--eigvals", str(a.eigvals), "--steps", str(a.steps),
           "--warmup", str(a.warmup)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        sys.exit("graph_project_wide_time: the run exceeded %d s; nothing more is started" % a.timeout)
    if r.returncode != 0:
        sys.exit("graph_project_wide_time: the run ended with status %d; nothing more is started" % r.returncode)
    res = dict(size=a.size, eigvals=a.eigvals, steps=a.steps, warmup=a.warmup, grey=json.loads(r.stdout.decode().strip().splitlines()[-1]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if a.merge_into:
        with open(a.merge_into) as f:
            whole = json.load(f)
        whole[a.key or "size%d_m%d" % (a.size, a.eigvals)] = res
        with open(a.merge_into, "w") as f:
            f.write(json.dumps(whole, indent=1) + "\n")


if __name__ == "__main__":
    main()
