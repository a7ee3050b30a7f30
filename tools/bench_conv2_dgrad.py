"""Times what DLWP_CONV_DGRAD moves in training: the forward and the input gradient of the U-Net family's non-3x3 convolutions
(the 1x1 shortcuts, first layers and heads, the 3x3 stride-2 downsampling, ConvTranspose2d 2x2 s2 and 4x4 s2 p1) at every
distinct layer the networks of tools/bench_conv2_wgrad.py meet, and the whole scripts/train.py-style step of those networks.

Forms, alternated repeat by repeat in one process, the library (MIOpen) warmed up first:
  hip     forward: dlwp_conv2d_mfma_f32 / dlwp_conv_transpose2d_mfma_f32 in the "bf16x6" form (ops.conv2d / ops.conv_transpose2d);
          input gradient: dlwp_conv2d_dgrad_mfma_f32 (ops.conv2d_input_grad), the transposed layer's dlwp_conv2d_mfma_f32
          (ops.conv_transpose2d_input_grad)
  torch   forward: F.conv2d / F.conv_transpose2d; input gradient: training.conv2d_input_grad_torch (aten.convolution_backward)
Steps run under DLWP_CONV_DGRAD=hip and =torch with DLWP_CONV_WGRAD left at its default, so the switch alone moves.
One JSON line per measurement:
  kind "step"   ms_hip / ms_torch   median of --steps steps after --warmup warm-up steps of each, with _lo3 / _hi3 the three
                                    fastest and slowest; mem_<form> peak bytes allocated during a step; samples, map_hw the
                                    leading dimension and the largest map the non-3x3 layers meet (the network's resolution)
  kind "layer"  fwd_ms_<form>, dx_ms_<form>   median per call (events around --inner calls) of --steps repeats, with _lo3 / _hi3;
                fwd_speedup, dx_speedup       torch / hip;  fwd_dev, dx_dev   rel-L2 of hip against torch;
                supported                     whether the kernels take the layer (otherwise only the torch columns)

Usage: python tools/bench_conv2_dgrad.py [--batch 32] [--steps 20] [--warmup 3] [--inner 4] [--only unethpx_n32,unet_c1,...]
                                         [--no-layers] [--no-steps] [--out profiles/conv2_dgrad.jsonl]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_conv2_wgrad as W2  # noqa: E402
import bench_conv_wgrad as W3  # noqa: E402
import bench_hpx_train as HPX  # noqa: E402

FORMS = ("hip", "torch")


def bench_net(tag, args, layers):
    from dlwp_benchmark_amd import training as T

    model, loss_fn = W3.build_cyl(tag, args.batch) if tag in W3.CYL_CASES else HPX.build(tag, args.batch)
    real = T.conv2_wgrad_uses_hip
    env_before = {v: os.environ.get(v) for v in ("DLWP_CONV_DGRAD", "DLWP_TRAIN_TORCH_BACKWARD")}     # HPX.step_ms sets the second
    own = set()

    def recording(batch, cin, cout, h, w, k, stride, padding, transposed):      # every _conv2_backward asks it: the layer list
        own.add((int(batch), int(cin), int(cout), int(h), int(w), int(k), int(stride), int(padding), bool(transposed)))
        return real(batch, cin, cout, h, w, k, stride, padding, transposed)

    def run(form):
        os.environ["DLWP_CONV_DGRAD"] = form
        return HPX.step_ms(model, loss_fn, False)

    T.conv2_wgrad_uses_hip = recording
    try:
        for _ in range(args.warmup):
            for f in FORMS:
                run(f)
        t, mem = {f: [] for f in FORMS}, {f: 0 for f in FORMS}
        for _ in range(args.steps if not args.no_steps else 0):
            for f in FORMS:
                ms, m = run(f)
                t[f].append(ms)
                mem[f] = max(mem[f], m)
    finally:
        T.conv2_wgrad_uses_hip = real
        for var, value in env_before.items():               # as the caller had them
            if value is None:
                os.environ.pop(var, None)
            else:
                os.environ[var] = value
    layers |= own
    del model
    torch.cuda.empty_cache()
    if args.no_steps:
        return None
    big = max(own, key=lambda l: l[3] * l[4]) if own else None
    row = dict(kind="step", tag=tag, batch=args.batch, seq=HPX.SEQ, steps=args.steps,
               samples=big[0] if big else None,             # the leading dimension the layers see (HEALPix: batch * 12 faces)
               map_hw=[big[3], big[4]] if big else None)    # the largest map a non-3x3 layer meets: the network's resolution
    for f in FORMS:
        sp = W3.spread(t[f])
        row.update({f"ms_{f}": sp["med"], f"ms_{f}_lo3": sp["lo3"], f"ms_{f}_hi3": sp["hi3"], f"mem_{f}": mem[f]})
    row["speedup"] = row["ms_torch"] / row["ms_hip"]
    return row


def _time(fns, args):
    t = {f: [] for f in fns}
    for _ in range(args.warmup):
        for f in fns:
            fns[f]()
    for _ in range(args.steps):
        for f in fns:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.inner):
                fns[f]()
            b.record()
            torch.cuda.synchronize()
            t[f].append(a.elapsed_time(b) / args.inner)
    return t


def bench_layer(layer, args):
    from dlwp_benchmark_amd import lib, ops, training as T

    n, cin, cout, h, w, k, s, p, transposed = layer
    oh, ow = ops._conv2d_out_hw(h, w, k, s, p, transposed)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    x, gz = (torch.randn(*shape, device="cuda:0", generator=g) for shape in ((n, cin, h, w), (n, cout, oh, ow)))
    wgt = torch.randn((cin, cout, k, k) if transposed else (cout, cin, k, k), device="cuda:0", generator=g) * (k * k * cin) ** -0.5
    L = lib.load()
    if transposed:
        ok_f = bool(L.dlwp_conv2d_mfma_variant(1, n, h, w, cout, k, s, p))
        ok_d = ops.conv_transpose2d_input_grad_supported(n, cin, cout, oh, ow, k, s, p)
        fwd = dict(hip=lambda: ops.conv_transpose2d(x, wgt, None, s, p, form="bf16x6"),
                   torch=lambda: F.conv_transpose2d(x, wgt, None, stride=s, padding=p))
        dx = dict(hip=lambda: ops.conv_transpose2d_input_grad(gz, wgt, s, p))
    else:
        ok_f = bool(L.dlwp_conv2d_mfma_variant(0, n, h, w, cout, k, s, p))
        ok_d = ops.conv2d_input_grad_supported(n, cin, cout, h, w, k, s, p)
        fwd = dict(hip=lambda: ops.conv2d(x, wgt, None, s, p, form="bf16x6"), torch=lambda: F.conv2d(x, wgt, None, stride=s, padding=p))
        dx = dict(hip=lambda: ops.conv2d_input_grad(gz, wgt, x.shape, s, p))
    dx["torch"] = lambda: T.conv2d_input_grad_torch(gz, x, wgt, s, p, transposed)
    if not ok_f:
        del fwd["hip"]
    if not ok_d:
        del dx["hip"]
    row = dict(kind="layer", n=n, cin=cin, cout=cout, h=h, w=w, k=k, stride=s, pad=p, transposed=transposed, steps=args.steps,
               flops=2.0 * n * min(h * w, oh * ow) * cin * cout * k * k, supported=bool(ok_f and ok_d))
    with torch.no_grad():
        for name, fns in (("fwd", fwd), ("dx", dx)):
            t = _time(fns, args)
            for f in fns:
                sp = W3.spread(t[f])
                row.update({f"{name}_ms_{f}": sp["med"], f"{name}_ms_{f}_lo3": sp["lo3"], f"{name}_ms_{f}_hi3": sp["hi3"]})
            if "hip" in fns:
                a_, b_ = fns["hip"](), fns["torch"]()
                row[f"{name}_dev"] = float((a_ - b_).norm() / b_.norm())
                row[f"{name}_speedup"] = row[f"{name}_ms_torch"] / row[f"{name}_ms_hip"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--no-steps", action="store_true", help="run the networks only to collect their layers")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv2_dgrad.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv2_dgrad.py measures on an MI355X: no GPU found")
    if args.steps < 20:
        print("note: fewer than 20 repeats", file=sys.stderr)
    tags = [t for t in args.only.split(",") if t] or list(W2.NETS)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    layers = set()
    for tag in tags:
        row = bench_net(tag, args, layers)
        if row is not None:
            emit(row)
    if not args.no_layers:
        for layer in sorted(layers):
            emit(bench_layer(layer, args))


if __name__ == "__main__":
    main()
