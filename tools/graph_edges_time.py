#!/usr/bin/env python3
"""Cost of the spectral edge map on a graph handle (glf_graph_edges, Graph.edges) against what a caller paid before the call
existed, on the benchmark workload, and the lengths of the sample pixels' rows of Phi against everybody else's.

  python tools/graph_edges_time.py [--size 4096] [--eigvals 64] [--steps 3] [--warmup 1] [--timeout 900]
                                   [--out profiles/graph_edges_time_cfg4.json]

bench.py's cfg4 (0.5 % sampling, m = ld = 64 at 4096 x 4096) on one GPU, a resident grey graph, in one child process under a time limit
(a run that fails or runs out of time ends there: nothing more is started on the GPU). Two handles of the same image live in the
process, one f32 and one compacted. After a warm-up all calls alternate in one loop, `steps` rounds:
  edges_D[_masked]      Graph.edges at D = 1 (E), 2 (E, S), 4 (E, S, SE, SW) directions, dim = m, response 1 - lam, without a mask and
                        with the mask that leaves out the sample pixels (built once, outside the timing)
  yardstick_D[_masked]  the same planes without the call: the shifted-slice expression on phi.view(H, W, ld) in torch on the
                        library's stream, per direction ((nb - px) * g) ** 2 summed over the columns, times the mask of both
                        endpoints; on the compact handle dequantize() first, which is what a caller has to do there
Every call is timed with HIP events on the library's stream and with the host clock; medians, every single time and the spreads are
reported. Bytes by construction (B = 4 or 2 bytes per entry of Phi; the kernel's strips of 62 columns read 2 halo columns each, its
blocks of 16 rows one halo row each):
  edges_D       N ld B (W + 2 strips - 2) / W (H + blocks - 1) / H + D N 4 (+ the mask, one byte per staged pixel)
  yardstick_D   at the least D (2 N ld 4 read + N 4 written) if torch fused the whole expression, which it does not; on the compact
                handle N ld (2 + 4) more for dequantize()
and the vector-pipe work of edges_D: 3 D dim operations per pixel (a subtraction, a multiplication and an fma per column and
direction) against 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz. `floor_set_by` compares these two constructed floors with each other and
nothing else: it names the larger one, not what the measured time is bound by (a call can sit well above both). `faster_beyond_spread` says whether the call's median is below the
yardstick's by more than the two spreads added. ld 32 / 128 / 256 are not timed. The row lengths: the median |Phi[px][0 .. m)| of
the sample pixels (Graph.samples) and of all other pixels on the f32 handle, how many of the 1000 longest rows belong to samples, and
the same on the test suite's two-tone image (61 x 47, 100 samples asked for, m = 8: its 12 longest rows). Prints one JSON line."""
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
VALU_LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9
STRIP, ROWS = 62, 16
DIRSETS = {1: ("E",), 2: ("E", "S"), 4: ("E", "S", "SE", "SW")}
SHIFT = {"E": (0, 1), "S": (1, 0), "SE": (1, 1), "SW": (1, -1)}


def _summary(ev, wall):
    return dict(ms_median=round(statistics.median(ev), 3), ms_all=[round(x, 3) for x in ev], ms_spread=round(max(ev) - min(ev), 3),
                wall_ms_median=round(statistics.median(wall), 3), wall_ms_all=[round(x, 3) for x in wall])


def _row_lengths(torch, g, top):
    """The lengths of the rows of an f32 handle's Phi, samples against the rest."""
    m = g.info["m"]
    length = g.phi[:, :m].double().norm(dim=1)
    is_sample = torch.zeros(length.numel(), dtype=torch.bool, device=length.device)
    is_sample[torch.from_numpy(g.samples().astype("int64")).to(length.device)] = True
    longest = torch.topk(length, top).indices
    rest = length[~is_sample]
    return dict(p=int(is_sample.sum().item()), median_sample=float(length[is_sample].median().item()), median_other=float(rest.median().item()),
                max_other=float(rest.max().item()), min_sample=float(length[is_sample].min().item()), longest_rows=top,
                longest_rows_that_are_samples=int(is_sample[longest].sum().item()),
                others_longer_than_the_shortest_sample=int((rest > length[is_sample].min()).sum().item()))


def child(size, eigvals, steps, warmup):
    import numpy as np
    import torch
    import glf

    img = glf.synth_image(size, size, seed=0)
    opt = glf.default_options(num_samples=int(size * size * 0.005), num_eigvals=eigvals, epsilon=0.1)
    n = size * size
    res = dict(device=torch.cuda.get_device_name(0))
    with glf.Context(0) as ctx:
        # the test suite's two-tone image first (tests/test_gpu_graph_cluster.py's _two_tone, seed 3)
        w, h = 61, 47
        tone = np.where(np.arange(w) < w // 2, 60.0, 190.0)[None]
        small = np.clip(np.rint(tone + 0.2 * (glf.synth_image(w, h, seed=3).astype(np.float64) - 127.5)), 0, 255).astype(np.uint8)
        with ctx.graph(ctx.to_device(small), glf.default_options(num_samples=100, num_eigvals=8, epsilon=0.1)) as g:
            res["row_lengths_two_tone_61x47"] = _row_lengths(torch, g, 12)

        d = torch.from_numpy(img).to(ctx.device)
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
        res["row_lengths"] = _row_lengths(torch, g32, 1000)
        g16.compact()
        ld, m = g32.info["ld"], g32.info["m"]
        res.update(p=g32.info["p"], m=m, ld=ld, phi_bytes_f32=g32.info["phi_bytes"], phi_bytes_compact=g16.info["phi_bytes"])
        resp = 1.0 - g32.eigenvalues
        with torch.cuda.stream(ctx.stream):
            mask = torch.ones(n, dtype=torch.uint8, device=ctx.device)
            mask[torch.from_numpy(g32.samples().astype(np.int64)).to(ctx.device)] = 0
            mask = mask.view(size, size)
            vb = mask != 0
            sc = torch.from_numpy(resp.astype(np.float32)).to(ctx.device)
            ref = torch.zeros((4, size, size), dtype=torch.float32, device=ctx.device)
        last = {}

        def yardstick(g, dirs, masked):
            def run():
                with torch.cuda.stream(ctx.stream):
                    phi = (g.phi if g.phi is not None else g.dequantize()).view(size, size, ld)[:, :, :m]
                    for k, name in enumerate(dirs):
                        dr, dc = SHIFT[name]
                        rows = slice(0, size - dr)
                        own = (rows, slice(0, size - 1) if dc == 1 else slice(1, size) if dc == -1 else slice(0, size))
                        nb = (slice(dr, size), slice(1, size) if dc == 1 else slice(0, size - 1) if dc == -1 else slice(0, size))
                        q = (((phi[nb] - phi[own]) * sc) ** 2).sum(-1)
                        if masked:
                            q = q * (vb[own] & vb[nb])
                        ref[k].zero_()
                        ref[k][own] = q
            return run

        def call(g, dirs, masked):
            def run():
                last["out"] = g.edges(dirs, valid=mask if masked else None, exclude_samples=False)
            return run

        calls = {}
        for side, g in (("f32", g32), ("compact", g16)):
            for nd, dirs in DIRSETS.items():
                for masked in (False, True):
                    tag = "%d%s|%s" % (nd, "_masked" if masked else "", side)
                    calls["edges_" + tag] = call(g, dirs, masked)
                    calls["yardstick_" + tag] = yardstick(g, dirs, masked)
        tm = {key: ([], []) for key in calls}
        for rnd in range(warmup + steps):
            for key, fn in calls.items():
                ev, wall = timed(fn)
                if rnd >= warmup:
                    tm[key][0].append(ev)
                    tm[key][1].append(wall)
        # what the two routes disagree by on the last round's planes (compact handle, four directions, masked)
        with torch.cuda.stream(ctx.stream):
            res["max_rel_difference_edges_vs_yardstick"] = float(((last["out"] - ref).abs().max() / ref.abs().max()).item())
        g32.close()
        g16.close()
    strips, blocks = -(-size // STRIP), -(-size // ROWS)
    halo = (size + 2 * strips - 2) / size * (size + blocks - 1) / size
    res["halo_factor"] = round(halo, 4)
    res["calls"] = {}
    for side, elem in (("f32", 4), ("compact", 2)):
        for nd in DIRSETS:
            for masked in (False, True):
                tag = "%d%s|%s" % (nd, "_masked" if masked else "", side)
                q, ys = _summary(*tm["edges_" + tag]), _summary(*tm["yardstick_" + tag])
                qb = int(n * ld * elem * halo + nd * n * 4 + (n * halo if masked else 0))
                yb = nd * (2 * n * ld * 4 + n * 4) + (n * ld * 6 if side == "compact" else 0)
                ops = 3 * nd * m * n
                q.update(bytes=qb, gb_per_s=round(qb / q["ms_median"] / 1e6, 1), hbm_fraction=round(qb / q["ms_median"] / 1e6 / HBM_CEILING_GBS, 3),
                         hbm_floor_ms=round(qb / HBM_CEILING_GBS / 1e6, 3), valu_lane_ops=ops, valu_floor_ms=round(ops / VALU_LANE_OPS_PER_S * 1e3, 3))
                q["floor_set_by"] = "vector pipe" if q["valu_floor_ms"] > q["hbm_floor_ms"] else "memory"
                ys.update(bytes_at_least=yb, gb_per_s_at_least=round(yb / ys["ms_median"] / 1e6, 1))
                spread = q["ms_spread"] + ys["ms_spread"]
                res["calls"][tag] = dict(edges=q, yardstick=ys, time_ratio=round(q["ms_median"] / ys["ms_median"], 3), spread_ms=round(spread, 3),
                                         faster_beyond_spread=bool(q["ms_median"] + spread < ys["ms_median"]))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--eigvals", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=900, help="seconds for the child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.size, a.eigvals, a.steps, a.warmup)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--size", str(a.size), "--eigvals", str(a.eigvals), "--steps", str(a.steps),
           "--warmup", str(a.warmup)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        sys.exit("graph_edges_time: the run exceeded %d s; nothing more is started" % a.timeout)
    if r.returncode != 0:
        sys.exit("graph_edges_time: the run ended with status %d; nothing more is started" % r.returncode)
    res = dict(size=a.size, eigvals=a.eigvals, steps=a.steps, warmup=a.warmup, grey=json.loads(r.stdout.decode().strip().splitlines()[-1]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
