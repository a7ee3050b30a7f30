"""Times the weight / bias gradient of the U-Net family's non-3x3 convolutions in training (the 1x1 shortcuts, first layers and
heads, the 3x3 stride-2 downsampling, ConvTranspose2d 2x2 s2 and 4x4 s2 p1): the call alone at every distinct layer the
networks meet, and the whole scripts/train.py-style step of the networks of tools/bench_conv_wgrad.py (batch 32; the HEALPix
networks with the faces folded into the batch, UNet / ModernUNet at the BASELINE C1 size).

Forms, alternated repeat by repeat in one process:
  hip     dlwp_conv2d_wgrad_f32 (ops.conv2d_weight_grad): both maps read where they lie, pre-activation at load, db from the
          same pass
  torch   training.conv2d_weight_grad_torch: the pre-activated copy + the library's convolution weight gradient (MIOpen, warmed
          up first) + gz.sum -- what autograd ran for these layers before the kernel existed
  auto    (steps only) DLWP_CONV_WGRAD=auto: the rules of training.conv_wgrad_uses_hip and conv2_wgrad_uses_hip
  try     (steps only, with --try-min-flops X) auto with CONV2_WGRAD_AUTO_MIN_FLOPS = X for the run: a candidate threshold
          against the committed one; the 3x3 layers follow their own rule as under auto
DLWP_CONV_WGRAD governs the 3x3 kernel of tools/bench_conv_wgrad.py as well, so "hip" and "torch" steps move both; "try" against
"auto" isolates this kernel.  One JSON line per measurement:
  kind "step"   ms_<form>          median of --steps steps after --warmup warm-up steps of each; ms_<form>_lo3 / _hi3 the three
                                   fastest and slowest; mem_<form> peak bytes allocated during a step
  kind "layer"  ms_hip / ms_torch  median per call (events around --inner calls) of --steps repeats, with _lo3 / _hi3;
                flops              2 N SH SW cin cout k^2 (training.conv2_wgrad_flops)
                hip_peak_frac      flops / ms_hip against the fp32 matrix peak (157.3 TF);
                slices, auto_hip   what dlwp_conv2d_wgrad_slices and the auto rule say for the layer

Usage: python tools/bench_conv2_wgrad.py [--batch 32] [--steps 20] [--warmup 3] [--inner 4] [--only unethpx_n32,unet_c1,...]
                                         [--try-min-flops X] [--no-layers] [--no-steps] [--out profiles/conv2_wgrad.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_conv_wgrad as W3  # noqa: E402
import bench_hpx_train as HPX  # noqa: E402

NETS = ("unethpx_n32", "munethpx_n32", "munethpx_n64", "diffmunethpx_n32", "unet_c1", "modernunet_c1")


def bench_net(tag, args, layers):
    from dlwp_benchmark_amd import ops, training as T

    model, loss_fn = W3.build_cyl(tag, args.batch) if tag in W3.CYL_CASES else HPX.build(tag, args.batch)
    real, committed = ops.conv2d_weight_grad, T.CONV2_WGRAD_AUTO_MIN_FLOPS
    forms = ("hip", "torch", "auto") + (("try",) if args.try_min_flops is not None else ())

    def recording(x, gz, k, stride, padding, pre_act=0, transposed=False, need_weight=True, need_bias=True):
        layers.add((x.shape[0], x.shape[1], gz.shape[1], x.shape[2], x.shape[3], int(k), int(stride), int(padding),
                    int(pre_act), bool(transposed)))
        return real(x, gz, k, stride, padding, pre_act=pre_act, transposed=transposed, need_weight=need_weight,
                    need_bias=need_bias)

    def run(form):
        os.environ["DLWP_CONV_WGRAD"] = "auto" if form == "try" else form
        T.CONV2_WGRAD_AUTO_MIN_FLOPS = args.try_min_flops if form == "try" else committed
        return HPX.step_ms(model, loss_fn, False)

    ops.conv2d_weight_grad = recording
    try:
        for _ in range(args.warmup):
            for f in forms:
                run(f)
        t, mem = {f: [] for f in forms}, {f: 0 for f in forms}
        for _ in range(args.steps if not args.no_steps else 0):
            for f in forms:
                ms, m = run(f)
                t[f].append(ms)
                mem[f] = max(mem[f], m)
    finally:
        ops.conv2d_weight_grad = real
        T.CONV2_WGRAD_AUTO_MIN_FLOPS = committed
        os.environ.pop("DLWP_CONV_WGRAD", None)
        os.environ.pop("DLWP_TRAIN_TORCH_BACKWARD", None)
    del model
    torch.cuda.empty_cache()
    if args.no_steps:
        return None
    row = dict(kind="step", tag=tag, batch=args.batch, seq=HPX.SEQ, steps=args.steps)
    if args.try_min_flops is not None:
        row["try_min_flops"] = args.try_min_flops
    for f in forms:
        sp = W3.spread(t[f])
        row.update({f"ms_{f}": sp["med"], f"ms_{f}_lo3": sp["lo3"], f"ms_{f}_hi3": sp["hi3"], f"mem_{f}": mem[f]})
    return row


def bench_layer(layer, args):
    from dlwp_benchmark_amd import lib, ops, training as T

    n, cin, cout, h, w, k, s, p, pre_act, transposed = layer
    oh, ow = ops._conv2d_out_hw(h, w, k, s, p, transposed)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    x, dz = (torch.randn(*shape, device="cuda:0", generator=g) for shape in ((n, cin, h, w), (n, cout, oh, ow)))
    fns = dict(hip=lambda: ops.conv2d_weight_grad(x, dz, k, s, p, pre_act=pre_act, transposed=transposed),
               torch=lambda: T.conv2d_weight_grad_torch(x, dz, k, s, p, pre_act, transposed))
    t = {f: [] for f in fns}
    with torch.no_grad():
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
        dev = [float((a_ - b_).norm() / b_.norm()) for a_, b_ in zip(fns["hip"](), fns["torch"]())]
    os.environ["DLWP_CONV_WGRAD"] = "auto"
    auto_hip = T.conv2_wgrad_uses_hip(n, cin, cout, h, w, k, s, p, transposed)
    os.environ.pop("DLWP_CONV_WGRAD", None)
    flops = T.conv2_wgrad_flops(n, cin, cout, h, w, k, s, p, transposed)
    row = dict(kind="layer", n=n, cin=cin, cout=cout, h=h, w=w, k=k, stride=s, pad=p, pre_act=pre_act, transposed=transposed,
               steps=args.steps, flops=flops, auto_hip=auto_hip, dw_dev=dev[0], db_dev=dev[1],
               slices=int(lib.load().dlwp_conv2d_wgrad_slices(n, cin, h, w, cout, k, s, p, int(transposed))))
    for f in fns:
        sp = W3.spread(t[f])
        row.update({f"ms_{f}": sp["med"], f"ms_{f}_lo3": sp["lo3"], f"ms_{f}_hi3": sp["hi3"]})
    row["speedup"] = row["ms_torch"] / row["ms_hip"]
    row["hip_peak_frac"] = flops / (row["ms_hip"] * 1e-3) / W3.FP32_PEAK
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--only", default="")
    ap.add_argument("--try-min-flops", type=float, default=None)
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--no-steps", action="store_true", help="run the networks only to collect their layers")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv2_wgrad.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv2_wgrad.py measures on an MI355X: no GPU found")
    if args.steps < 20:
        print("note: fewer than 20 repeats", file=sys.stderr)
    tags = [t for t in args.only.split(",") if t] or list(NETS)
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
