#!/usr/bin/env python3
"""Cost of the robust fit on a graph handle (glf_graph_robust_step, Graph.fit_robust) against the existing calls that do the same
work, on the benchmark workload.

  python tools/graph_robust_time.py [--size 4096] [--steps 3] [--warmup 1] [--timeout 600] [--out profiles/graph_robust_time_cfg4.json]

bench.py's cfg4 (0.5 % sampling, m = 64, ld = 64) on one GPU, a resident grey graph, in one child process under a time limit (a run
that fails or runs out of time ends there: nothing more is started on the GPU). The planes are in the span of Phi under noise, with
5 % of the pixels moved by 20 standard deviations of the noise; a 0/1 weight plane with 70 % ones. After a warm-up the calls
alternate, `steps` rounds: robust_step for 1 and 3 planes under each loss, with and without the optional outputs; the yardstick,
the existing calls a caller would string together for one iteration -- glf_graph_synthesize(nout = nplanes) with no identity term,
then glf_graph_normal_equations under a weight plane -- and, timed on its own, the torch elementwise pass (residual, q, Huber's u,
the product with w) that caller would need between the two; Graph.fit (the plain fit: the cost of one quadratic solve end to end)
and Graph.fit_robust end to end for 1 plane under each loss, iterations reported. Every call is timed with HIP events on the library's
stream and with the host clock; medians, every single time and the spreads are reported. For the step the bytes it must move by
construction (Phi twice, the planes twice, the weights in and out and in again) give the achieved fraction of 6.3 TB/s. Prints one
JSON line."""
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
LOSSES = ("huber", "cauchy", "tukey")


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
        g = ctx.graph(d, opt)
        ld, m = g.info["ld"], g.info["m"]
        res.update(p=g.info["p"], m=m, ld=ld, phi_bytes=g.info["phi_bytes"])
        gen = torch.Generator(device=ctx.device).manual_seed(0)
        noise = torch.tensor([1.0, 0.1, 10.0], device=ctx.device)
        a_true = torch.randn((3, m), generator=gen, device=ctx.device)
        clean = (g.phi[:, :m] @ a_true.T).T.contiguous()
        clean *= (30.0 * noise / clean.std(dim=1))[:, None]
        planes = clean + noise[:, None] * torch.randn((3, n), generator=gen, device=ctx.device)
        hit = torch.rand((3, n), generator=gen, device=ctx.device) < 0.05
        sign = torch.where(torch.rand((3, n), generator=gen, device=ctx.device) < 0.5, -1.0, 1.0)
        planes = torch.where(hit, planes + 20.0 * noise[:, None] * sign, planes).reshape(3, size, size).contiguous()
        weight = (torch.rand((size, size), generator=gen, device=ctx.device) < 0.7).float().contiguous()
        sub = {1: planes[:1].contiguous(), 3: planes}
        # the iterate the steps are timed at: the plain fit, and the scales of its residuals on the driver's sample
        G, b = g.normal_equations(weight, planes)
        pen = np.full(m, 1e-6 * np.trace(G) / m)                                 # (a ridge far below the data term: no system is refused)
        a0 = glf.fit_coeffs(G, b, pen)
        fit0, info0 = g.fit_robust(planes, weight, penalty=pen, max_iter=1, return_info=True)
        sigma = info0["sigma"]
        res.update(sigma=[round(float(x), 4) for x in sigma])
        del fit0, info0
        torch.cuda.synchronize()

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(ctx.stream)
            out = fn()
            e1.record(ctx.stream)
            e1.synchronize()
            return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out

        def torch_weights(k):
            # what a caller has to compute between synthesize and normal_equations today (Huber)
            with torch.cuda.stream(ctx.stream):
                r = sub[k] - synth[k]
                q = ((r * inv_sigma[:k, None, None]) ** 2).sum(dim=0)
                return weight * torch.where(q <= 1.345 ** 2, torch.ones_like(q), 1.345 / torch.sqrt(q))

        inv_sigma = torch.from_numpy((1.0 / sigma).astype(np.float32)).to(ctx.device)
        synth = {k: g.synthesize(a0[:k]) for k in (1, 3)}
        weff = {k: torch_weights(k).contiguous() for k in (1, 3)}
        torch.cuda.synchronize()
        calls, iters = {}, {}
        for k in (1, 3):
            for loss in LOSSES:
                calls["step_%s_%d" % (loss, k)] = lambda k=k, loss=loss: g.robust_step(sub[k], a0[:k], loss, sigma=sigma[:k], weight=weight)
            calls["step_huber_%d_outputs" % k] = lambda k=k: g.robust_step(sub[k], a0[:k], "huber", sigma=sigma[:k], weight=weight, want_weights=True,
                                                                         want_residuals=True)
            calls["synthesize_%d" % k] = lambda k=k: g.synthesize(a0[:k])
            calls["normal_w_%d" % k] = lambda k=k: g.normal_equations(weff[k], sub[k])
            calls["torch_weights_%d" % k] = lambda k=k: torch_weights(k)
        calls["fit_1"] = lambda: g.fit(sub[1], weight, penalty=pen)
        for loss in LOSSES:
            calls["fit_robust_%s_1" % loss] = lambda loss=loss: g.fit_robust(sub[1], weight, loss=loss, penalty=pen, return_info=True)
        t = {name: ([], []) for name in calls}
        for rnd in range(warmup + steps):
            for name, fn in calls.items():
                ev, wall, out = timed(fn)
                if name.startswith("fit_robust"):
                    iters[name] = dict(iterations=out[1]["iterations"], converged=out[1]["converged"])
                del out
                if rnd >= warmup:
                    t[name][0].append(ev)
                    t[name][1].append(wall)
        g.close()
    for name in t:
        res[name] = _summary(*t[name])
        res[name].update(iters.get(name, {}))
    for k in (1, 3):
        for loss in LOSSES:
            s = res["step_%s_%d" % (loss, k)]
            nbytes = 2 * n * ld * 4 + 2 * k * n * 4 + 3 * n * 4
            s.update(bytes=nbytes, gb_per_s=round(nbytes / s["ms_median"] / 1e6, 1), hbm_fraction=round(nbytes / s["ms_median"] / 1e6 / HBM_CEILING_GBS, 3))
    # the yardstick: the step against the existing calls that do the same work (and the elementwise pass a caller would add)
    res["yardstick"] = {}
    for k in (1, 3):
        new = res["step_huber_%d" % k]
        old = res["synthesize_%d" % k]["ms_median"] + res["normal_w_%d" % k]["ms_median"]
        spread = res["synthesize_%d" % k]["ms_spread"] + res["normal_w_%d" % k]["ms_spread"] + new["ms_spread"]
        res["yardstick"]["planes_%d" % k] = dict(step_ms=new["ms_median"], synthesize_plus_normal_ms=round(old, 3),
                                                 torch_weights_ms=res["torch_weights_%d" % k]["ms_median"], ratio=round(new["ms_median"] / old, 3),
                                                 spread_ms=round(spread, 3), not_slower_beyond_spread=bool(new["ms_median"] <= old + spread))
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
        sys.exit("graph_robust_time: the run exceeded %d s; nothing more is started" % a.timeout)
    if r.returncode != 0:
        sys.exit("graph_robust_time: the run ended with status %d; nothing more is started" % r.returncode)
    res = dict(size=a.size, steps=a.steps, warmup=a.warmup, grey=json.loads(r.stdout.decode().strip().splitlines()[-1]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
