#!/usr/bin/env python3
"""Per-layer and whole-step timing of the forms of the U-Net family's non-3x3 convolutions: "direct" (csrc/conv2.hip), "bf16x6"
and "bf16" (csrc/conv_mfma.hip), and torch's F.conv2d / F.conv_transpose2d (MIOpen), in one process.

Layers: every distinct ops.conv2d / ops.conv_transpose2d call of C1's UNet at the benchmark's batch (bench.config_table) and of
the yaml-width UNetHPX / MUNetHPX [136, 68, 34] at nside 32, batch 32 (384 faces), as the networks call them (pre_act, act,
resid).  Per layer one JSON line: forms alternated call by call, each call between its own pair of HIP events and followed by
a host wait, median of --reps calls per form with the 10th / 90th percentile as the run-to-run spread (the method of
tools/bench_conv3x3.py, whose helpers this tool uses).  Then one line per network with the whole inference step under
set_conv_form("bf16x6") alone -- what the 3x3 form gives by itself -- against the same plus set_aux_conv_form("bf16x6") and
plus set_aux_conv_form("bf16"), alternated the same way, the form set outside the timed interval.

Usage: python tools/bench_conv_aux.py [--reps 25] [--step-reps 25] [--only c1,unethpx,munethpx] [--out profiles/conv_aux_mfma.jsonl]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_conv3x3 import DEV, FORMS, alternate, networks, summary  # noqa: E402
from dlwp_benchmark_amd import ops  # noqa: E402

ACT_FN = {0: lambda t: t, 1: F.gelu, 2: torch.tanh, 3: F.relu, 4: F.silu}


def layer_shapes(model, ins):
    """the distinct ops.conv2d / ops.conv_transpose2d calls of one step, in model order, through recorders around the ops"""
    seen, real_c, real_t = {}, ops.conv2d, ops.conv_transpose2d

    def conv2d(x, weight, bias, stride=1, padding=0, pre_act=0, act=0, resid=None, form="direct"):
        key = (False, x.shape[0], x.shape[2], x.shape[3], x.shape[1], weight.shape[0], weight.shape[2], int(stride), int(padding),
               int(pre_act), int(act), resid is not None, bias is not None)
        seen[key] = seen.get(key, 0) + 1
        return real_c(x, weight, bias, stride, padding, pre_act=pre_act, act=act, resid=resid, form=form)

    def conv_transpose2d(x, weight, bias, stride, padding=0, act=0, form="direct"):
        key = (True, x.shape[0], x.shape[2], x.shape[3], x.shape[1], weight.shape[1], weight.shape[2], int(stride), int(padding),
               0, int(act), False, bias is not None)
        seen[key] = seen.get(key, 0) + 1
        return real_t(x, weight, bias, stride, padding, act, form=form)

    ops.conv2d, ops.conv_transpose2d = conv2d, conv_transpose2d
    try:
        with torch.no_grad():
            model(**ins)
    finally:
        ops.conv2d, ops.conv_transpose2d = real_c, real_t
    return seen


def bench_layer(key, reps):
    tr, n, h, w, cin, cout, k, s, p, pre, act, has_resid, has_bias = key
    g = torch.Generator(device=DEV).manual_seed(n + cout)
    rnd = lambda *sh: torch.randn(*sh, device=DEV, generator=g)
    x = rnd(n, cin, h, w)
    wt = rnd(*((cin, cout) if tr else (cout, cin)), k, k) / (k * cin ** 0.5)
    b = rnd(cout) if has_bias else None
    if tr:
        fns = {f: (lambda f=f: ops.conv_transpose2d(x, wt, b, s, p, act, form=f)) for f in FORMS}
        fns["torch"] = lambda: ACT_FN[act](F.conv_transpose2d(x, wt, b, stride=s, padding=p))
    else:
        oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        resid = rnd(n, cout, oh, ow) if has_resid else None
        fns = {f: (lambda f=f: ops.conv2d(x, wt, b, s, p, pre_act=pre, act=act, resid=resid, form=f)) for f in FORMS}
        xa = ACT_FN[pre](x)         # the activated input is given to torch: its time is the bare convolution's

        def torch_conv():
            y = F.conv2d(xa, wt, b, stride=s, padding=p)
            return ACT_FN[act](y if resid is None else y + resid)

        fns["torch"] = torch_conv
    with torch.no_grad():
        ref = fns["direct"]().double()
        err = {f: float(torch.linalg.vector_norm(fns[f]().double() - ref) / torch.linalg.vector_norm(ref)) for f in FORMS[1:]}
        times = alternate(fns, reps)
    oh, ow = ref.shape[2], ref.shape[3]
    taps = k * k // (s * s) if tr else k * k       # per output value
    v = int(ops._lib.load().dlwp_conv2d_mfma_variant(int(tr), n, h, w, cout, k, s, p))
    row = dict(kind="layer", transposed=tr, images=n, H=h, W=w, cin=cin, cout=cout, k=k, stride=s, pad=p, pre_act=pre, act=act,
               resid=has_resid, bias=has_bias, reps=reps, gflop=round(2e-9 * n * oh * ow * cin * cout * taps, 2),
               variant=dict(fragment_width=v // 16, nf=v % 16), rel_l2_vs_direct=err)
    for name, ts in times.items():
        row[name] = summary(ts)
    d = row["direct"]
    for f in FORMS[1:]:
        row[f]["x_direct"] = round(d["ms"] / row[f]["ms"], 2)
        row[f]["x_torch"] = round(row["torch"]["ms"] / row[f]["ms"], 2)
        # faster than the direct kernel by more than the spread: the slow end of this form against the fast end of direct
        row[f]["faster_beyond_spread"] = row[f]["p90"] < d["p10"]
    return row


STEP_FORMS = {"conv_bf16x6": "direct", "conv_bf16x6+aux_bf16x6": "bf16x6", "conv_bf16x6+aux_bf16": "bf16"}


def bench_step(tag, model, ins, reps):
    def step():
        with torch.no_grad():
            return model(**ins)

    model.set_conv_form("bf16x6")
    times = alternate({name: step for name in STEP_FORMS}, reps, warmup=2,
                      before=lambda name: model.set_aux_conv_form(STEP_FORMS[name]))          # the setter is not timed
    model.set_conv_form("direct").set_aux_conv_form("direct")
    row = dict(kind="step", tag=tag, cls=type(model).__name__, reps=reps)
    for name, ts in times.items():
        row[name] = summary(ts)
    base = row["conv_bf16x6"]
    for name in list(STEP_FORMS)[1:]:
        row[name]["x_conv_bf16x6"] = round(base["ms"] / row[name]["ms"], 2)
        row[name]["faster_beyond_spread"] = row[name]["p90"] < base["p10"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--step-reps", type=int, default=25)
    ap.add_argument("--only", default="c1,unethpx,munethpx")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_aux_mfma.jsonl"))
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
