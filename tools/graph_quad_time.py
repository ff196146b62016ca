#!/usr/bin/env python3
"""Cost of the per-pixel quadratic forms on a graph handle (glf_graph_quadform, Graph.leverage) against what a caller paid before
the call existed, on the benchmark workload.

  python tools/graph_quad_time.py [--size 4096] [--eigvals 64] [--steps 3] [--warmup 1] [--timeout 900]
                                  [--out profiles/graph_quad_time_cfg4.json] [--merge-into FILE --key NAME]

bench.py's cfg4 (0.5 % sampling, m = ld = 64 at 4096 x 4096) on one GPU, a resident grey graph, in one child process under a time limit
(a run that fails or runs out of time ends there: nothing more is started on the GPU). Two handles of the same image live in the
process, one f32 and one compacted. After a warm-up all calls alternate in one loop, `steps` rounds:
  quadform_K    Graph.quadform(R, t) at r = 64 columns and K = 1, 8, 32 centres
  yardstick_K   the same planes without the call: two synthesize(32 outputs, no identity term) into one [64, H, W] tensor, then per
                centre ((y - t_k) ** 2).sum(0) in torch on the library's stream
  leverage      Graph.leverage(weight): one normal_equations, fit_factor on the host, one quadform with one centre
Every call is timed with HIP events on the library's stream and with the host clock; medians, every single time and the spreads are
reported. Bytes by construction (B = 4 or 2 bytes per entry of Phi):
  quadform_K    N ld B + K N 4                                     flops 2 N ld 64 + 3 N 64 K
  yardstick_K   2 N ld B + 64 N 4 + K (64 N 4 + N 4) at the least  (the planes written, then read once per centre if torch fused
                the subtraction, the square and the sum, which it does not)
`faster_beyond_spread` says whether quadform_K's median is below yardstick_K's by more than the two spreads added. --eigvals 256
--size 2048 is the m = ld = 256 run; --merge-into adds this run's result under --key to an existing JSON file. Prints one JSON line."""
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
COLS = 64
CENTRES = (1, 8, 32)


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
    res = dict(device=torch.cuda.get_device_name(0))
    rng = np.random.default_rng(0)
    with glf.Context(0) as ctx:
        d = torch.from_numpy(img).to(ctx.device)
        gen = torch.Generator(device=ctx.device)
        gen.manual_seed(0)
        weight = (torch.rand((size, size), generator=gen, device=ctx.device) >= 0.3).float()
        torch.cuda.synchronize()

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(ctx.stream)
            fn()
            e1.record(ctx.stream)
            e1.synchronize()
            return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

        g32, g16 = ctx.graph(d, opt), ctx.graph(d, opt)
        g16.compact()
        ld, m = g32.info["ld"], g32.info["m"]
        res.update(p=g32.info["p"], m=m, ld=ld, phi_bytes_f32=g32.info["phi_bytes"], phi_bytes_compact=g16.info["phi_bytes"])
        # a metric at the scale of the leverage's R, centres among the rows of Phi R
        G = g32.normal_equations(None)[0]
        R = glf.fit_factor(G, 1e-3 * np.trace(G) / m * np.ones(m))[:, :COLS]
        if R.shape[1] < COLS:
            R = np.hstack([R, rng.normal(size=(m, COLS - R.shape[1])) * np.abs(R).mean()])
        rows = g32.rows(rng.choice(n, 32, replace=False)).astype(np.float64)
        t = rows @ R
        with torch.cuda.stream(ctx.stream):
            y = torch.empty((COLS, size, size), dtype=torch.float32, device=ctx.device)
            out = torch.empty((32, size, size), dtype=torch.float32, device=ctx.device)
            ref = torch.empty((32, size, size), dtype=torch.float32, device=ctx.device)
            td = torch.from_numpy(t.astype(np.float32)).to(ctx.device)

        def yardstick(g, k):
            def run():
                g.synthesize(R[:, :32].T, out=y[:32])
                g.synthesize(R[:, 32:].T, out=y[32:])
                with torch.cuda.stream(ctx.stream):
                    for c in range(k):
                        ref[c] = ((y - td[c][:, None, None]) ** 2).sum(0)
            return run

        calls = {}
        for side, g in (("f32", g32), ("compact", g16)):
            for k in CENTRES:
                calls["quadform_%d|%s" % (k, side)] = (lambda g=g, k=k: g.quadform(R, t[:k], out=out[:k]))
                calls["yardstick_%d|%s" % (k, side)] = yardstick(g, k)
            calls["leverage|%s" % side] = (lambda g=g: g.leverage(weight, ridge=1e-3))
        tm = {key: ([], []) for key in calls}
        for rnd in range(warmup + steps):
            for key, fn in calls.items():
                ev, wall = timed(fn)
                if rnd >= warmup:
                    tm[key][0].append(ev)
                    tm[key][1].append(wall)
        # what the two routes disagree by on the last round's planes (compact handle, 32 centres)
        with torch.cuda.stream(ctx.stream):
            res["max_rel_difference_quadform_vs_yardstick"] = float(((out - ref).abs().max() / ref.abs().max()).item())
        g32.close()
        g16.close()
    res["calls"] = {}
    for side, elem in (("f32", 4), ("compact", 2)):
        phi = n * ld * elem
        for k in CENTRES:
            q, ys = _summary(*tm["quadform_%d|%s" % (k, side)]), _summary(*tm["yardstick_%d|%s" % (k, side)])
            qb, yb = phi + k * n * 4, 2 * phi + COLS * n * 4 + k * (COLS * n * 4 + n * 4)
            flops = 2 * n * ld * COLS + 3 * n * COLS * k
            q.update(bytes=qb, gb_per_s=round(qb / q["ms_median"] / 1e6, 1), hbm_fraction=round(qb / q["ms_median"] / 1e6 / HBM_CEILING_GBS, 3),
                     flops=flops, tflop_per_s=round(flops / q["ms_median"] / 1e9, 2))
            ys.update(bytes_at_least=yb, gb_per_s_at_least=round(yb / ys["ms_median"] / 1e6, 1))
            spread = q["ms_spread"] + ys["ms_spread"]
            res["calls"]["r64_ncent%d|%s" % (k, side)] = dict(quadform=q, yardstick=ys, time_ratio=round(q["ms_median"] / ys["ms_median"], 3),
                                                              spread_ms=round(spread, 3),
                                                              faster_beyond_spread=bool(q["ms_median"] + spread < ys["ms_median"]))
        res["calls"]["leverage|%s" % side] = _summary(*tm["leverage|%s" % side])
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
        sys.exit("graph_quad_time: the run exceeded %d s; nothing more is started" % a.timeout)
    if r.returncode != 0:
        sys.exit("graph_quad_time: the run ended with status %d; nothing more is started" % r.returncode)
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
