#!/usr/bin/env python3
"""Cost of the blend read-out on a graph handle (glf_graph_blend, Graph.blend) against what a caller paid before the call existed, on
the benchmark workload.

  python tools/graph_blend_time.py [--size 4096] [--eigvals 64] [--steps 3] [--warmup 1] [--timeout 900]
                                   [--out profiles/graph_blend_time_cfg4.json]

bench.py's cfg4 (0.5 % sampling, m = ld = 64 at 4096 x 4096) on one GPU, a resident grey graph, in one child process under a time
limit (a run that fails or runs out of time ends there: nothing more is started on the GPU). Two handles of the same image live in
the process, one f32 and one compacted. After a warm-up all calls alternate in one loop, `steps` rounds, (nout, nlevels) = (1, 2),
(1, 8), (1, 32), (4, 8), the nout planes as identity planes of every level (the bank of Graph.apply_local), one level map of random
fractions in [0, nlevels - 1]:
  blend_O_L        Graph.blend into a resident [O, H, W] tensor
  torch_O_L        the same values without the call: synthesize(O * L) into one [O * L, H, W] tensor, then on the library's stream
                   the clamp, the floor, two torch.gather and the lerp f * z_hi + (z_lo - f * z_lo)
  synthesize_O     synthesize(O) with the planes as identity planes: the floor that Phi and the O stores set
Every call is timed with HIP events on the library's stream and with the host clock; medians, every single time and the spreads are
reported. Bytes by construction (B = 4 or 2 bytes per entry of Phi): blend N ld B + N 4 (the level map) + 2 O N 4 (the planes in, the
outputs out); the torch route writes and reads back O L N 4 more, besides its own temporaries.
`faster_beyond_spread` says whether blend's median is below the torch route's by more than the two spreads added. ld 32 / 128 / 256
are not timed. Prints one JSON line. Reads nothing outside the repository."""
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
CASES = ((1, 2), (1, 8), (1, 32), (4, 8))


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
    omax, smax = max(o for o, _ in CASES), max(o * l for o, l in CASES)
    with glf.Context(0) as ctx:
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
        g16.compact()
        ld, m = g32.info["ld"], g32.info["m"]
        res.update(p=g32.info["p"], m=m, ld=ld, phi_bytes_f32=g32.info["phi_bytes"], phi_bytes_compact=g16.info["phi_bytes"])
        # coefficients at the scale that makes the scores of order one; the identity planes are noise of the same order
        a = rng.normal(size=(smax, m)) / (np.sqrt(m) * float(g32.phi[:, :m].abs().max()))
        with torch.cuda.stream(ctx.stream):
            gen = torch.Generator(device=ctx.device)
            gen.manual_seed(0)
            planes = torch.randn((omax, size, size), generator=gen, device=ctx.device, dtype=torch.float32)
            unit = torch.rand((size, size), generator=gen, device=ctx.device, dtype=torch.float32)
            y = torch.empty((smax, size, size), dtype=torch.float32, device=ctx.device)
            out = torch.empty((omax, size, size), dtype=torch.float32, device=ctx.device)
            levels = {l: (unit * float(l - 1)).contiguous() for l in sorted({l for _, l in CASES})}
        ctx.synchronize()
        last = {}

        def bank(o, l):
            return (a[:o * l].reshape(o, l, m), np.linspace(1.0, 0.0, l, dtype=np.float32)[None, :].repeat(o, axis=0),
                    np.arange(o, dtype=np.int32)[:, None].repeat(l, axis=1))

        def blend(g, o, l):
            coeffs, ident, plane = bank(o, l)

            def run():
                last["blend"] = g.blend(coeffs, levels[l], ident, plane, planes[:o], out=out[:o])
            return run

        def synth(g, o):
            coeffs, ident, plane = bank(o, 2)
            return lambda: g.synthesize(coeffs[:, 0], ident[:, 0], plane[:, 0], planes[:o], out=out[:o])

        def torch_route(g, o, l):
            coeffs, ident, plane = bank(o, l)

            def run():
                g.synthesize(coeffs.reshape(o * l, m), ident.reshape(-1), plane.reshape(-1), planes[:o], out=y[:o * l])
                with torch.cuda.stream(ctx.stream):
                    z = y[:o * l].view(o, l, size, size)
                    tc = torch.nan_to_num(levels[l], nan=0.0).clamp(0.0, float(l - 1))
                    i = tc.floor().clamp(max=float(l - 2))
                    f = tc - i
                    idx = i.long()[None, None].expand(o, 1, size, size)
                    z_lo, z_hi = torch.gather(z, 1, idx)[:, 0], torch.gather(z, 1, idx + 1)[:, 0]
                    last["torch"] = torch.addcmul(z_lo - f * z_lo, f.expand_as(z_hi), z_hi)
            return run

        calls = {}
        for side, g in (("f32", g32), ("compact", g16)):
            for o in sorted({o for o, _ in CASES}):
                calls["synthesize_%d|%s" % (o, side)] = synth(g, o)
            for o, l in CASES:
                calls["blend_%d_%d|%s" % (o, l, side)] = blend(g, o, l)
                calls["torch_%d_%d|%s" % (o, l, side)] = torch_route(g, o, l)
        tm = {key: ([], []) for key in calls}
        for rnd in range(warmup + steps):
            for key, fn in calls.items():
                ev, wall = timed(fn)
                if rnd >= warmup:
                    tm[key][0].append(ev)
                    tm[key][1].append(wall)
                last.clear()
        # the two routes on the same bank (compact handle, (4, 8)): the lerp of the torch route is not the pinned one, so a few ulps
        calls["blend_4_8|compact"]()
        ours = last["blend"].clone()
        calls["torch_4_8|compact"]()
        with torch.cuda.stream(ctx.stream):
            res["max_abs_difference_to_torch"] = float((ours - last["torch"]).abs().max())
        ctx.synchronize()
        g32.close()
        g16.close()
    res["calls"] = {}
    for side, elem in (("f32", 4), ("compact", 2)):
        phi = n * ld * elem
        for o, l in CASES:
            sy = _summary(*tm["synthesize_%d|%s" % (o, side)])
            sy.update(bytes=phi + 2 * o * n * 4)
            q, ys = _summary(*tm["blend_%d_%d|%s" % (o, l, side)]), _summary(*tm["torch_%d_%d|%s" % (o, l, side)])
            qb = phi + n * 4 + 2 * o * n * 4
            q.update(bytes=qb, gb_per_s=round(qb / q["ms_median"] / 1e6, 1), hbm_fraction=round(qb / q["ms_median"] / 1e6 / HBM_CEILING_GBS, 3),
                     time_ratio=round(q["ms_median"] / ys["ms_median"], 3), spread_ms=round(q["ms_spread"] + ys["ms_spread"], 3),
                     faster_beyond_spread=bool(q["ms_median"] + q["ms_spread"] + ys["ms_spread"] < ys["ms_median"]),
                     ratio_to_synthesize=round(q["ms_median"] / sy["ms_median"], 3))
            res["calls"]["o%d_l%d|%s" % (o, l, side)] = dict(blend=q, torch=ys, synthesize=sy)
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
        sys.exit("graph_blend_time: the run exceeded %d s; nothing more is started" % a.timeout)
    if r.returncode != 0:
        sys.exit("graph_blend_time: the run ended with status %d; nothing more is started" % r.returncode)
    res = dict(size=a.size, eigvals=a.eigvals, steps=a.steps, warmup=a.warmup, grey=json.loads(r.stdout.decode().strip().splitlines()[-1]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
