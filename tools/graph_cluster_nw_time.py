#!/usr/bin/env python3
"""Cost of one Lloyd iteration with unit-length rows and a weight plane (glf_graph_cluster_step_ex, the weight and normalise modes of k_graph_cluster)
against the plain step (glf_graph_cluster_step, its plain mode) of the same build, on the benchmark workload.

  python tools/graph_cluster_nw_time.py [--size 4096] [--steps 3] [--warmup 1] [--timeout 600]
                                        [--out profiles/graph_cluster_nw_time_cfg4.json]

bench.py's cfg4 (0.5 % sampling, m = 64, ld = 64) on one GPU, a resident grey graph, in one child process under a time limit (a run
that fails or runs out of time ends there: nothing more is started on the GPU). After a warm-up the calls alternate, `steps` rounds, at
(k, dim) = (8, 8) and (32, 64), all without prev and into one label buffer: the plain step (the yardstick), cluster_step_ex with
normalize, with a weight plane, and with both. Every call is timed with HIP events on the library's stream and with the
host clock; medians, every single time and the spreads are reported. The bytes a step must move by construction are N CW 4 of Phi plus
4 N of labels, plus 4 N with a weight plane; they give the achieved fraction of 6.3 TB/s. Prints one JSON line."""
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
CASES = ((8, 8), (32, 64))


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
        weight = torch.from_numpy(rng.uniform(0.0, 2.0, (size, size)).astype(np.float32)).to(ctx.device)
        torch.cuda.synchronize()
        calls, nbytes = {}, {}
        for k, dim in CASES:
            px = torch.from_numpy(rng.choice(n, size=k, replace=False)).to(ctx.device)
            raw = g.phi[px, :dim].double().cpu().numpy()
            unit = raw / np.sqrt((raw * raw).sum(axis=1))[:, None]
            tag = "%d_%d" % (k, dim)
            calls["plain_" + tag] = lambda raw=raw: g.cluster_step(raw, labels=labels)
            calls["normalize_" + tag] = lambda unit=unit: g.cluster_step_ex(unit, labels=labels, normalize=True)
            calls["weight_" + tag] = lambda raw=raw: g.cluster_step_ex(raw, labels=labels, weight=weight)
            calls["normalize_weight_" + tag] = lambda unit=unit: g.cluster_step_ex(unit, labels=labels, normalize=True, weight=weight)
            nbytes["plain_" + tag] = nbytes["normalize_" + tag] = n * cw * 4 + 4 * n
            nbytes["weight_" + tag] = nbytes["normalize_weight_" + tag] = n * cw * 4 + 8 * n
        t = {name: ([], []) for name in calls}
        for rnd in range(warmup + steps):
            for name, fn in calls.items():
                ev, wall, out = timed(fn)
                del out
                if rnd >= warmup:
                    t[name][0].append(ev)
                    t[name][1].append(wall)
        for name in t:
            s = res[name] = _summary(*t[name])
            s.update(bytes=nbytes[name], gb_per_s=round(nbytes[name] / s["ms_median"] / 1e6, 1),
                     hbm_fraction=round(nbytes[name] / s["ms_median"] / 1e6 / HBM_CEILING_GBS, 3))
        for name in t:
            if name.startswith("plain_"):
                continue
            y = res["plain_" + "_".join(name.split("_")[-2:])]
            s = res[name]
            s.update(plain_ms=y["ms_median"], over_plain_ms=round(s["ms_median"] - y["ms_median"], 3),
                     ratio_to_plain=round(s["ms_median"] / y["ms_median"], 3), spread_ms=round(s["ms_spread"] + y["ms_spread"], 3))
        g.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=600, help="seconds for the child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.size, a.steps, a.warmup)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "1", "--size", str(a.size), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        sys.exit("graph_cluster_nw_time: the run exceeded %d s; nothing more is started" % a.timeout)
    if r.returncode != 0:
        sys.exit("graph_cluster_nw_time: the run ended with status %d; nothing more is started" % r.returncode)
    res = dict(size=a.size, steps=a.steps, warmup=a.warmup, grey=json.loads(r.stdout.decode().strip().splitlines()[-1]))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
