#!/usr/bin/env python3
"""Per-layer and whole-step timing of the forms of pad(1) + Conv2d(3x3): "direct" (csrc/conv.hip), "bf16x6" and "bf16"
(csrc/conv_mfma.hip), and torch's F.conv2d on the PRE-PADDED, pre-concatenated input (MIOpen: what the layer costs without the
padding and the cat), in one process.

Layers: every distinct 3x3 convolution shape of C1's UNet at the benchmark's batch (bench.config_table) and of the yaml-width
UNetHPX / MUNetHPX [136, 68, 34] at nside 32, batch 32 (384 faces), as the networks call them (segments, pre_act, act, resid).
Per layer one JSON line: forms alternated call by call, each call between its own pair of HIP events, median of --reps calls
per form with the 10th / 90th percentile as the run-to-run spread.  Every call is followed by a host wait for its stop event,
so the queue is empty when the next call starts: layers of a few microseconds (C1's) show launch latency as much as kernel
time.  Then one line per network with the whole inference step (one model call that makes one step) per form, alternated the
same way, the form set outside the timed interval.

Usage: python tools/bench_conv3x3.py [--reps 25] [--step-reps 20] [--only c1,unethpx,munethpx] [--out profiles/conv3x3_mfma.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dlwp_benchmark_amd import ops  # noqa: E402

DEV = "cuda:0"
GELU = "th.nn.GELU()"
FORMS = ("direct", "bf16x6", "bf16")
HPX = dict(constant_channels=4, prescribed_channels=1, prognostic_channels=3, hidden_channels=[136, 68, 34], activation=GELU,
           context_size=2)


def networks():
    """tag -> (model on the device in eval mode, keyword inputs of one inference step)"""
    import bench
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd.weights import fill_state_dict

    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)

    def c1():
        cls, cfg, batch, _, (h, w), *_ = bench.config_table()["C1"]
        model = getattr(M, cls)(**cfg)
        ctx, cg = cfg["context_size"], cfg["prognostic_channels"]
        return model, dict(prognostic=rnd(batch, ctx + 1, cg, h, w))

    def hpx(cls, **extra):
        cfg = dict(HPX, **extra)
        model = getattr(M, cls)(**cfg)
        ctx, n, b = cfg["context_size"], 32, 32
        return model, dict(constants=rnd(b, 1, cfg["constant_channels"], 12, n, n),
                           prescribed=rnd(b, ctx + 1, cfg["prescribed_channels"], 12, n, n),
                           prognostic=rnd(b, ctx + 1, cfg["prognostic_channels"], 12, n, n))

    makers = {"c1": c1, "unethpx": lambda: hpx("UNetHPX", n_convolutions=2), "munethpx": lambda: hpx("MUNetHPX", norm=False)}
    for tag, make in makers.items():
        model, ins = make()
        fill_state_dict(model, gain=0.7)
        yield tag, model.to(DEV).eval(), ins


def layer_shapes(model, ins):
    """the distinct ops.conv3x3 calls of one step, in model order: run once in a matrix-pipe form (every call then funnels
    through ops.conv3x3) with the op wrapped by a recorder"""
    seen, real = {}, ops.conv3x3

    def recorder(x0, weight, bias, act=0, x1=None, pre_act=0, resid=None, hpx=False, form="direct"):
        key = (bool(hpx), x0.shape[0], x0.shape[2], x0.shape[3], x0.shape[1], 0 if x1 is None else x1.shape[1], weight.shape[0],
               int(pre_act), int(act), resid is not None)
        seen.setdefault(key, 0)
        seen[key] += 1
        return real(x0, weight, bias, act=act, x1=x1, pre_act=pre_act, resid=resid, hpx=hpx, form=form)

    model.set_conv_form("bf16x6")
    ops.conv3x3 = recorder
    try:
        with torch.no_grad():
            model(**ins)
    finally:
        ops.conv3x3 = real
        model.set_conv_form("direct")
    return seen


def alternate(fns, reps, warmup=3, before=None):
    """{name: callable} -> {name: [ms per call]}: names alternated call by call, every call between its own events;
    before(name) runs outside the timed interval"""
    for _ in range(warmup):
        for k, fn in fns.items():
            if before:
                before(k)
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            if before:
                before(k)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return times


def summary(ts):
    q = statistics.quantiles(ts, n=10)
    return dict(ms=round(statistics.median(ts), 4), p10=round(q[0], 4), p90=round(q[-1], 4))


def bench_layer(key, reps):
    hpx, n, h, w, c0, c1, cout, pre, act, has_resid = key
    g = torch.Generator(device=DEV).manual_seed(n + cout)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
    x0, x1 = rnd(n, c0, h, w), (rnd(n, c1, h, w) if c1 else None)
    wt, b = rnd(cout, c0 + c1, 3, 3) / (3.0 * (c0 + c1) ** 0.5), rnd(cout)
    resid = rnd(n, cout, h, w) if has_resid else None
    xcat = x0 if x1 is None else torch.cat([x0, x1], 1)
    xpad = ops.healpix_pad(xcat, 1) if hpx else F.pad(torch.cat([xcat[..., -1:], xcat, xcat[..., :1]], -1), (0, 0, 1, 1))
    fns = {f: (lambda f=f: ops.conv3x3(x0, wt, b, act=act, x1=x1, pre_act=pre, resid=resid, hpx=hpx, form=f)) for f in FORMS}
    fns["conv2d"] = lambda: F.conv2d(xpad, wt, b)
    with torch.no_grad():
        ref = fns["direct"]().double()
        err = {f: float(torch.linalg.vector_norm(fns[f]().double() - ref) / torch.linalg.vector_norm(ref)) for f in FORMS[1:]}
        times = alternate(fns, reps)
    row = dict(kind="layer", hpx=hpx, images=n, H=h, W=w, c0=c0, c1=c1, cout=cout, pre_act=pre, act=act, resid=has_resid,
               reps=reps, gflop=round(2e-9 * n * h * w * (c0 + c1) * cout * 9, 2), rel_l2_vs_direct=err)
    for k, ts in times.items():
        row[k] = summary(ts)
    d = row["direct"]
    for f in FORMS[1:]:
        row[f]["x_direct"] = round(d["ms"] / row[f]["ms"], 2)
        row[f]["x_conv2d"] = round(row["conv2d"]["ms"] / row[f]["ms"], 2)
        # faster than the direct kernel by more than the spread: the slow end of this form against the fast end of direct
        row[f]["faster_beyond_spread"] = row[f]["p90"] < d["p10"]
    return row


def bench_step(tag, model, ins, reps):
    def step():
        with torch.no_grad():
            return model(**ins)

    times = alternate({f: step for f in FORMS}, reps, warmup=2, before=model.set_conv_form)   # the setter is not timed
    model.set_conv_form("direct")
    row = dict(kind="step", tag=tag, cls=type(model).__name__, reps=reps)
    for k, ts in times.items():
        row[k] = summary(ts)
    for f in FORMS[1:]:
        row[f]["x_direct"] = round(row["direct"]["ms"] / row[f]["ms"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--step-reps", type=int, default=20)
    ap.add_argument("--only", default="c1,unethpx,munethpx")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv3x3_mfma.jsonl"))
    args = ap.parse_args()
    if args.reps < 20 or args.step_reps < 20:
        raise SystemExit("at least 20 calls per form")
    only = set(args.only.split(","))
    done = set()
    with open(args.out, "w") as out:
        def emit(row):
            row["device"] = torch.cuda.get_device_name(0)
            line = json.dumps(row)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()

        for tag, model, ins in networks():
            if tag not in only:
                continue
            for key, calls in layer_shapes(model, ins).items():
                if key in done:
                    continue
                done.add(key)
                row = bench_layer(key, args.reps)
                row.update(network=tag, calls_per_step=calls)
                emit(row)
            emit(bench_step(tag, model, ins, args.step_reps))
            del model, ins
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
