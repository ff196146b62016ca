#!/usr/bin/env python3
"""Cost of one Lloyd iteration on a graph handle (glf_graph_cluster_step) against glf_graph_synthesize, on the benchmark workload.

  python tools/graph_cluster_time.py [--size 4096] [--steps 3] [--warmup 1] [--wide 256] [--timeout 600]
                                     [--out profiles/graph_cluster_time_cfg4.json]

bench.py's cfg4 (0.5 % sampling, m = 64, ld = 64) on one GPU, a resident grey graph, in one child process under a time limit (a run
that fails or runs out of time ends there: nothing more is started on the GPU); then, in a second child, the same image with
--wide eigenpairs (ld 256: the step reads 256 of every row's 1024 bytes; 0 skips it). After a warm-up the calls alternate, `steps`
rounds: cluster_step at (k, dim) = (2, 2), (8, 8), (32, 32), (32, 64) without prev, at (32, 64) with prev in place, and
glf_graph_synthesize with nout = k random coefficient rows and no identity term -- the assignment's MFMA work on the same pass over
Phi, without the argmin and the update, but with k output planes to write: the yardstick. Every call is timed with HIP events on the
library's stream and with the host clock; medians, every single time and the spreads are reported. For a step the bytes it must move
by construction are N CW 4 of Phi plus 4 N of labels (8 N with prev); they give the achieved fraction of 6.3 TB/s. Last, Graph.segment
end to end at k = 8 (seeded) with its iteration count. Prints one JSON line."""
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
CASES = ((2, 2), (8, 8), (32, 32), (32, 64))


def _summary(ev, wall):
    return dict(ms_median=round(statistics.median(ev), 3), ms_all=[round(x, 3) for x in ev], ms_spread=round(max(ev) - min(ev), 3),
                wall_ms_median=round(statistics.median(wall), 3), wall_ms_all=[round(x, 3) for x in wall])


def child(size, steps, warmup, m, segment):
    import numpy as np
    import torch
    import glf

    img = glf.synth_image(size, size, seed=0)
    opt = glf.default_options(num_samples=int(size * size * 0.005), num_eigvals=m, epsilon=0.1)
    n = size * size
    res = dict(device=torch.cuda.get_device_name(0))
    with glf.Context(0) as ctx:
        d = torch.from_numpy(img).to(ctx.device)
        rng = np.random.default_rng(0)
        torch.cuda.synchronize()

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(ctx.stream)
            out = fn()
            e1.record(ctx.stream)
            e1.synchronize()
            return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out

        g = ctx.graph(d, opt)
        ld, m = g.info["ld"], g.info["m"]
        cw = 32 if ld < 64 else 64
        res.update(p=g.info["p"], m=m, ld=ld, cw=cw, phi_bytes=g.info["phi_bytes"])
        labels = torch.zeros((size, size), dtype=torch.int32, device=ctx.device)
        torch.cuda.synchronize()
        calls, cents = {}, {}
        for k, dim in CASES:
            px = rng.choice(n, size=k, replace=False)
            cents[(k, dim)] = g.phi[torch.from_numpy(px).to(ctx.device), :dim].double().cpu().numpy()
            calls["step_%d_%d" % (k, dim)] = lambda k=k, dim=dim: g.cluster_step(cents[(k, dim)], labels=labels)
        calls["step_32_64_prev"] = lambda: g.cluster_step(cents[(32, 64)], prev=labels, labels=labels)
        for k in sorted({k for k, _ in CASES}):
            a = rng.normal(size=(k, m))
            calls["synth_%d" % k] = lambda a=a: g.synthesize(a)
        t = {name: ([], []) for name in calls}
        for rnd in range(warmup + steps):
            for name, fn in calls.items():
                ev, wall, out = timed(fn)
                del out
                if rnd >= warmup:
                    t[name][0].append(ev)
                    t[name][1].append(wall)
        for name in t:
            res[name] = _summary(*t[name])
        for name in t:
            if not name.startswith("step_"):
                continue
            k = int(name.split("_")[1])
            s, y = res[name], res["synth_%d" % k]
            nbytes = n * cw * 4 + (8 if name.endswith("prev") else 4) * n
            s.update(bytes=nbytes, gb_per_s=round(nbytes / s["ms_median"] / 1e6, 1), hbm_fraction=round(nbytes / s["ms_median"] / 1e6 / HBM_CEILING_GBS, 3),
                     synth_ms=y["ms_median"], ratio_to_synth=round(s["ms_median"] / y["ms_median"], 3),
                     spread_ms=round(s["ms_spread"] + y["ms_spread"], 3))
        if segment:
            t0 = time.perf_counter()
            _, _, st = g.segment(8, seed=1)
            res["segment_8"] = dict(wall_ms=round((time.perf_counter() - t0) * 1e3, 3), iterations=st["iterations"], converged=st["converged"],
                                    changed_last=st["changed_last"], counts=[int(c) for c in st["counts"]])
        g.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--wide", type=int, default=256, help="eigenpairs of the second, wide handle (0: skip it)")
    ap.add_argument("--timeout", type=int, default=600, help="seconds for each child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.size, a.steps, a.warmup, a.child, a.child == 64)
    res = dict(size=a.size, steps=a.steps, warmup=a.warmup)
    for name, m in (("grey", 64), ("grey_wide", a.wide)):
        if not m:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(m), "--size", str(a.size), "--steps", str(a.steps), "--warmup", str(a.warmup)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            sys.exit("graph_cluster_time: the %s run exceeded %d s; nothing more is started" % (name, a.timeout))
        if r.returncode != 0:
            sys.exit("graph_cluster_time: the %s run ended with status %d; nothing more is started" % (name, r.returncode))
        res[name] = json.loads(r.stdout.decode().strip().splitlines()[-1])
        if a.out:                                                                # (what is measured so far survives a later failure)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
