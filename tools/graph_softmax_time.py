#!/usr/bin/env python3
"""Cost of the softmax read-out on a graph handle (glf_graph_softmax, Graph.softmax) against what a caller paid before the call
existed, on the benchmark workload.

  python tools/graph_softmax_time.py [--size 4096] [--eigvals 64] [--steps 3] [--warmup 1] [--timeout 900]
                                     [--out profiles/graph_softmax_time_cfg4.json]

bench.py's cfg4 (0.5 % sampling, m = ld = 64 at 4096 x 4096) on one GPU, a resident grey graph, in one child process under a time
limit (a run that fails or runs out of time ends there: nothing more is started on the GPU). Two handles of the same image live in
the process, one f32 and one compacted. After a warm-up all calls alternate in one loop, `steps` rounds, K = 2, 8, 32 classes,
without / with K identity planes (the logits of a mean-field step):
  softmax_{prob,entropy,all}_K[_ident]   Graph.softmax wanting the probabilities alone / the entropy alone / all three outputs
  torch_{prob,entropy,all}_K[_ident]     the same result without the call: synthesize(K) into a [K, H, W] tensor, then on the
                                         library's stream torch.softmax(dim=0) for prob alone; where the entropy is wanted, log p
                                         is needed too: torch.log_softmax(dim=0), its exp and minus the sum of their product
                                         (entropy), and torch.logsumexp(dim=0) besides (all)
  synthesize_K[_ident]                   synthesize(K) alone: the floor that the K stores set
  project_wide_K                         Phi^T diag(w) Q of K probability planes: the other half of one mean-field iteration, whose
                                         softmax half is softmax_prob_K_ident
Every call is timed with HIP events on the library's stream and with the host clock; medians, every single time and the spreads are
reported. Bytes by construction (B = 4 or 2 bytes per entry of Phi, I = K identity planes or none):
  softmax prob   N ld B + I N 4 + K N 4        entropy   N ld B + I N 4 + N 4        all   N ld B + I N 4 + (K + 2) N 4
  torch prob     the same + 2 K N 4 (the scores written by synthesize and read by torch.softmax)
`faster_beyond_spread` says whether softmax's median is below the torch route's by more than the two spreads added. ld 32 / 128 / 256
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
CLASSES = (2, 8, 32)
WANTS = {"prob": ("prob",), "entropy": ("entropy",), "all": ("prob", "lse", "entropy")}


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
    kmax = max(CLASSES)
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
        a = rng.normal(size=(kmax, m)) / (np.sqrt(m) * float(g32.phi[:, :m].abs().max()))
        ident, plane = np.ones(kmax, dtype=np.float32), np.arange(kmax, dtype=np.int32)
        with torch.cuda.stream(ctx.stream):
            gen = torch.Generator(device=ctx.device)
            gen.manual_seed(0)
            planes = torch.randn((kmax, size, size), generator=gen, device=ctx.device, dtype=torch.float32)
            y = torch.empty((kmax, size, size), dtype=torch.float32, device=ctx.device)
            weight = torch.ones((size, size), dtype=torch.float32, device=ctx.device)
            weight.view(-1)[torch.from_numpy(g32.samples().astype(np.int64)).to(ctx.device)] = 0
        last = {}

        def softmax(g, k, want, with_ident):
            def run():
                last["softmax"] = g.softmax(a[:k], ident[:k], plane[:k], planes[:k], want=want) if with_ident else g.softmax(a[:k], want=want)
            return run

        def synth(g, k, with_ident):
            if with_ident:
                g.synthesize(a[:k], ident[:k], plane[:k], planes[:k], out=y[:k])
            else:
                g.synthesize(a[:k], out=y[:k])

        def torch_route(g, k, which, with_ident):
            def run():
                synth(g, k, with_ident)
                with torch.cuda.stream(ctx.stream):
                    if which == "prob":
                        out = dict(prob=torch.softmax(y[:k], dim=0))
                    else:
                        lp = torch.log_softmax(y[:k], dim=0)
                        out = dict(prob=lp.exp())
                        out["entropy"] = -(out["prob"] * lp).sum(dim=0)
                    if which == "all":
                        out["lse"] = torch.logsumexp(y[:k], dim=0)
                    last["torch"] = out
            return run

        calls = {}
        for side, g in (("f32", g32), ("compact", g16)):
            for k in CLASSES:
                calls["project_wide_%d|%s" % (k, side)] = (lambda g=g, k=k: g.project_wide(planes[:k], weight))
                for with_ident in (False, True):
                    tag = "%d%s|%s" % (k, "_ident" if with_ident else "", side)
                    calls["synthesize_" + tag] = (lambda g=g, k=k, w=with_ident: synth(g, k, w))
                    for which, want in WANTS.items():
                        calls["softmax_%s_%s" % (which, tag)] = softmax(g, k, want, with_ident)
                        calls["torch_%s_%s" % (which, tag)] = torch_route(g, k, which, with_ident)
        tm = {key: ([], []) for key in calls}
        for rnd in range(warmup + steps):
            for key, fn in calls.items():
                ev, wall = timed(fn)
                if rnd >= warmup:
                    tm[key][0].append(ev)
                    tm[key][1].append(wall)
                last.clear()
        # the two routes on the same scores (compact handle, 32 classes with identity planes)
        calls["softmax_all_%d_ident|compact" % kmax]()
        ours = dict(last["softmax"])
        calls["torch_all_%d_ident|compact" % kmax]()
        with torch.cuda.stream(ctx.stream):
            res["max_abs_difference_to_torch"] = {key: float((ours[key] - last["torch"][key]).abs().max()) for key in ("prob", "lse", "entropy")}
        g32.close()
        g16.close()
    res["calls"] = {}
    for side, elem in (("f32", 4), ("compact", 2)):
        phi = n * ld * elem
        for k in CLASSES:
            pw = _summary(*tm["project_wide_%d|%s" % (k, side)])
            for with_ident in (False, True):
                tag = "%d%s|%s" % (k, "_ident" if with_ident else "", side)
                idb = k * n * 4 if with_ident else 0
                sy = _summary(*tm["synthesize_" + tag])
                sy.update(bytes=phi + idb + k * n * 4, hbm_fraction=round((phi + idb + k * n * 4) / sy["ms_median"] / 1e6 / HBM_CEILING_GBS, 3))
                entry = dict(synthesize=sy)
                for which, nout in (("prob", k), ("entropy", 1), ("all", k + 2)):
                    q, ys = _summary(*tm["softmax_%s_%s" % (which, tag)]), _summary(*tm["torch_%s_%s" % (which, tag)])
                    qb = phi + idb + nout * n * 4
                    q.update(bytes=qb, gb_per_s=round(qb / q["ms_median"] / 1e6, 1), hbm_fraction=round(qb / q["ms_median"] / 1e6 / HBM_CEILING_GBS, 3),
                             time_ratio=round(q["ms_median"] / ys["ms_median"], 3), spread_ms=round(q["ms_spread"] + ys["ms_spread"], 3),
                             faster_beyond_spread=bool(q["ms_median"] + q["ms_spread"] + ys["ms_spread"] < ys["ms_median"]),
                             ratio_to_synthesize=round(q["ms_median"] / sy["ms_median"], 3))
                    entry["softmax_" + which] = q
                    entry["torch_" + which] = ys
                if with_ident:
                    sm = entry["softmax_prob"]
                    entry["mean_field_iteration"] = dict(project_wide=pw, softmax_ms_median=sm["ms_median"],
                                                         ms_median_sum=round(pw["ms_median"] + sm["ms_median"], 3))
                res["calls"]["k" + tag] = entry
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
        sys.exit("graph_softmax_time: the run exceeded %d s; nothing more is started" % a.timeout)
    if r.returncode != 0:
        sys.exit("graph_softmax_time: the run ended with status %d; nothing more is started" % r.returncode)
    res = dict(size=a.size, eigvals=a.eigvals, steps=a.steps, warmup=a.warmup, grey=json.loads(r.stdout.decode().strip().splitlines()[-1]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
