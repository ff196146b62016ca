#!/usr/bin/env python3
"""Cost of the label read-out on a graph handle (glf_graph_classify, Graph.classify) against what a caller paid before the call
existed, on the benchmark workload.

  python tools/graph_classify_time.py [--size 4096] [--eigvals 64] [--steps 3] [--warmup 1] [--timeout 900]
                                      [--out profiles/graph_classify_time_cfg4.json]

bench.py's cfg4 (0.5 % sampling, m = ld = 64 at 4096 x 4096) on one GPU, a resident grey graph, in one child process under a time
limit (a run that fails or runs out of time ends there: nothing more is started on the GPU). Two handles of the same image live in
the process, one f32 and one compacted. After a warm-up all calls alternate in one loop, `steps` rounds, K = 2, 8, 32 classes:
  classify_K_{label,all}[_ident]   Graph.classify wanting the label alone / all three outputs, without / with K identity planes
  yardstick_K[_ident]              the same result without the call: synthesize(K) into a [K, H, W] tensor, then
                                   torch.topk(2, dim=0) and the subtraction on the library's stream (label, best and margin)
  argmax_K[_ident]                 the cheapest route to the label alone: synthesize(K), then torch.argmax(dim=0)
  synthesize_1                     one output with no identity term: where classify without identity planes is expected to sit
Every call is timed with HIP events on the library's stream and with the host clock; medians, every single time and the spreads are
reported. Bytes by construction (B = 4 or 2 bytes per entry of Phi, I = K identity planes or none, O = 1 or 3 outputs):
  classify     N ld B + I N 4 + O N 4
  yardstick    N ld B + I N 4 + K N 4 written + K N 4 read + 3 N 4 at the least (torch's own temporaries not counted)
`faster_beyond_spread` says whether classify's median is below the yardstick's by more than the two spreads added (label alone:
against argmax too). ld 32 / 128 / 256 are not timed. Prints one JSON line. Reads nothing outside the repository."""
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
        last = {}

        def classify(g, k, want, with_ident):
            def run():
                last["classify"] = g.classify(a[:k], ident[:k], plane[:k], planes[:k], want=want) if with_ident else g.classify(a[:k], want=want)
            return run

        def yardstick(g, k, with_ident, top2):
            def run():
                if with_ident:
                    g.synthesize(a[:k], ident[:k], plane[:k], planes[:k], out=y[:k])
                else:
                    g.synthesize(a[:k], out=y[:k])
                with torch.cuda.stream(ctx.stream):
                    if top2:
                        t2 = torch.topk(y[:k], 2, dim=0)
                        last["yardstick"] = dict(label=t2.indices[0], best=t2.values[0], margin=t2.values[0] - t2.values[1])
                    else:
                        last["argmax"] = torch.argmax(y[:k], dim=0)
            return run

        calls = {}
        for side, g in (("f32", g32), ("compact", g16)):
            calls["synthesize_1|%s" % side] = (lambda g=g: g.synthesize(a[:1], out=y[:1]))
            for k in CLASSES:
                for with_ident in (False, True):
                    tag = "%d%s|%s" % (k, "_ident" if with_ident else "", side)
                    calls["classify_label_" + tag] = classify(g, k, ("label",), with_ident)
                    calls["classify_all_" + tag] = classify(g, k, ("label", "best", "margin"), with_ident)
                    calls["yardstick_" + tag] = yardstick(g, k, with_ident, True)
                    calls["argmax_" + tag] = yardstick(g, k, with_ident, False)
        tm = {key: ([], []) for key in calls}
        for rnd in range(warmup + steps):
            for key, fn in calls.items():
                ev, wall = timed(fn)
                if rnd >= warmup:
                    tm[key][0].append(ev)
                    tm[key][1].append(wall)
        # the two routes on the same scores (compact handle, 32 classes with identity planes): the scores have synthesize's bits
        calls["classify_all_%d_ident|compact" % kmax]()
        calls["yardstick_%d_ident|compact" % kmax]()
        with torch.cuda.stream(ctx.stream):
            c, ys = last["classify"], last["yardstick"]
            res["best_equal_bits"] = bool(torch.equal(c["best"].view(torch.int32), ys["best"].view(torch.int32)))
            res["margin_equal_bits"] = bool(torch.equal(c["margin"].view(torch.int32), ys["margin"].view(torch.int32)))
            res["labels_differ"] = int((c["label"].long() != ys["label"]).sum().item())
        g32.close()
        g16.close()
    res["calls"] = {}
    for side, elem in (("f32", 4), ("compact", 2)):
        phi = n * ld * elem
        res["calls"]["synthesize_1|%s" % side] = s1 = _summary(*tm["synthesize_1|%s" % side])
        s1.update(bytes=phi + n * 4, hbm_fraction=round((phi + n * 4) / s1["ms_median"] / 1e6 / HBM_CEILING_GBS, 3))
        for k in CLASSES:
            for with_ident in (False, True):
                tag = "%d%s|%s" % (k, "_ident" if with_ident else "", side)
                idb = k * n * 4 if with_ident else 0
                ys, am = _summary(*tm["yardstick_" + tag]), _summary(*tm["argmax_" + tag])
                yb = phi + idb + 2 * k * n * 4 + 3 * n * 4
                ys.update(bytes_at_least=yb, gb_per_s_at_least=round(yb / ys["ms_median"] / 1e6, 1))
                entry = dict(yardstick=ys, argmax=am)
                for which, nout in (("label", 1), ("all", 3)):
                    q = _summary(*tm["classify_%s_%s" % (which, tag)])
                    qb = phi + idb + nout * n * 4
                    q.update(bytes=qb, gb_per_s=round(qb / q["ms_median"] / 1e6, 1), hbm_fraction=round(qb / q["ms_median"] / 1e6 / HBM_CEILING_GBS, 3),
                             time_ratio=round(q["ms_median"] / ys["ms_median"], 3), spread_ms=round(q["ms_spread"] + ys["ms_spread"], 3),
                             faster_beyond_spread=bool(q["ms_median"] + q["ms_spread"] + ys["ms_spread"] < ys["ms_median"]),
                             ratio_to_synthesize_1=round(q["ms_median"] / s1["ms_median"], 3))
                    if which == "label":
                        q.update(time_ratio_to_argmax=round(q["ms_median"] / am["ms_median"], 3),
                                 faster_than_argmax_beyond_spread=bool(q["ms_median"] + q["ms_spread"] + am["ms_spread"] < am["ms_median"]))
                    entry["classify_" + which] = q
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
        sys.exit("graph_classify_time: the run exceeded %d s; nothing more is started" % a.timeout)
    if r.returncode != 0:
        sys.exit("graph_classify_time: the run ended with status %d; nothing more is started" % r.returncode)
    res = dict(size=a.size, eigvals=a.eigvals, steps=a.steps, warmup=a.warmup, grey=json.loads(r.stdout.decode().strip().splitlines()[-1]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
