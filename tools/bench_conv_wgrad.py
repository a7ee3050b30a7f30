"""Times the weight / bias gradient of the 3x3 convolutions in training: the call alone at every distinct layer shape the
networks meet, and the whole scripts/train.py-style step -- batch 32, the HEALPix networks of tools/bench_hpx_train.py (faces
folded into the batch, Bt = 12 B) and UNet / ModernUNet at the BASELINE C1 size (64 x 64 cylinder, hidden [8, 16, 32, 64]).

Forms, alternated repeat by repeat in one process:
  hip     dlwp_conv3x3_wgrad_f32 (ops.conv3x3_weight_grad): segments, pre-activation and padding applied at load, db from the
          same pass
  torch   training.conv3x3_weight_grad_torch: torch.cat + pre-activation + padded copy + torch.nn.grad.conv2d_weight (MIOpen,
          warmed up first) + gz.sum -- the whole composition, which is what the step ran before the kernel existed
  auto    (steps only) DLWP_CONV_WGRAD=auto: the rule of training.conv_wgrad_uses_hip
One JSON line per measurement:
  kind "step"   ms_<form>          median of --steps steps after --warmup warm-up steps of each; ms_<form>_lo3 / _hi3 the three
                                   fastest and slowest; mem_<form> peak bytes allocated during a step
  kind "layer"  ms_hip / ms_torch  median per call (events around --inner calls) of --steps repeats, with _lo3 / _hi3;
                hip_peak_frac      2 N H W Cin Cout 9 FLOPs / ms_hip against the fp32 matrix peak (157.3 TF);
                slices, auto_hip   what dlwp_conv3x3_wgrad_slices and the auto rule say for the shape

Usage: python tools/bench_conv_wgrad.py [--batch 32] [--steps 20] [--warmup 3] [--inner 4] [--only unethpx_n32,unet_c1,...]
                                        [--no-layers] [--out profiles/conv_wgrad.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_hpx_train as HPX  # noqa: E402

FP32_PEAK = 157.3e12
C1 = dict(constant_channels=0, prescribed_channels=0, prognostic_channels=1, hidden_channels=[8, 16, 32, 64],
          activation=HPX.GELU, context_size=1)
CYL_CASES = {       # tag -> (class, ctor kwargs, (H, W))
    "unet_c1": ("UNet", dict(C1, n_convolutions=2), (64, 64)),
    "modernunet_c1": ("ModernUNet", dict(C1), (64, 64)),
}
FORMS = ("hip", "torch", "auto")


def spread(ms):
    s = sorted(ms)
    return dict(med=statistics.median(s), lo3=[round(v, 4) for v in s[:3]], hi3=[round(v, 4) for v in s[-3:]])


def build_cyl(tag, batch):
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd.weights import fill_state_dict
    from oracle.make_golden import rollout_mse

    cls, cfg, (h, w) = CYL_CASES[tag]
    model = getattr(M, cls)(**cfg)
    fill_state_dict(model, gain=0.7)
    model = model.to("cuda:0").train()
    g = torch.Generator(device="cuda:0").manual_seed(0)
    prognostic = torch.randn(batch, HPX.SEQ, cfg["prognostic_channels"], h, w, device="cuda:0", generator=g)

    def loss_fn():
        y = model(constants=None, prescribed=None, prognostic=prognostic)
        return rollout_mse(y, prognostic, cfg["context_size"])
    return model, loss_fn


def bench_net(tag, args, shapes):
    from dlwp_benchmark_amd import ops

    model, loss_fn = build_cyl(tag, args.batch) if tag in CYL_CASES else HPX.build(tag, args.batch)
    real = ops.conv3x3_weight_grad

    def recording(x0, x1, dz, pre_act=0, hpx=False, need_bias=True):
        shapes.add((x0.shape[0], x0.shape[1], x1.shape[1] if x1 is not None else 0, dz.shape[1], x0.shape[2], x0.shape[3],
                    int(pre_act), bool(hpx)))
        return real(x0, x1, dz, pre_act=pre_act, hpx=hpx, need_bias=need_bias)

    def run(form):
        os.environ["DLWP_CONV_WGRAD"] = form
        return HPX.step_ms(model, loss_fn, False)

    ops.conv3x3_weight_grad = recording
    try:
        for _ in range(args.warmup):
            for f in FORMS:
                run(f)
        t, mem = {f: [] for f in FORMS}, {f: 0 for f in FORMS}
        for _ in range(args.steps):
            for f in FORMS:
                ms, m = run(f)
                t[f].append(ms)
                mem[f] = max(mem[f], m)
    finally:
        ops.conv3x3_weight_grad = real
        os.environ.pop("DLWP_CONV_WGRAD", None)
        os.environ.pop("DLWP_TRAIN_TORCH_BACKWARD", None)
    row = dict(kind="step", tag=tag, batch=args.batch, seq=HPX.SEQ, steps=args.steps)
    for f in FORMS:
        sp = spread(t[f])
        row.update({f"ms_{f}": sp["med"], f"ms_{f}_lo3": sp["lo3"], f"ms_{f}_hi3": sp["hi3"], f"mem_{f}": mem[f]})
    del model
    torch.cuda.empty_cache()
    return row


def bench_layer(shape, args):
    from dlwp_benchmark_amd import healpix as H
    from dlwp_benchmark_amd import lib, ops, training as T

    n, c0, c1, cout, h, w, pre_act, hpx = shape
    g = torch.Generator(device="cuda:0").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda:0", generator=g)
    x0, x1, dz = rnd(n, c0, h, w), (rnd(n, c1, h, w) if c1 else None), rnd(n, cout, h, w)
    table = H.device_table(h, w, 1, "cuda:0") if hpx else None
    fns = dict(hip=lambda: ops.conv3x3_weight_grad(x0, x1, dz, pre_act=pre_act, hpx=hpx),
               torch=lambda: T.conv3x3_weight_grad_torch(x0, x1, dz, pre_act, table))
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
    os.environ["DLWP_CONV_WGRAD"] = "auto"
    auto_hip = T.conv_wgrad_uses_hip(n, c0, c1, cout, h, w, hpx)
    os.environ.pop("DLWP_CONV_WGRAD", None)
    row = dict(kind="layer", n=n, c0=c0, c1=c1, cout=cout, h=h, w=w, pre_act=pre_act, hpx=hpx, steps=args.steps,
               slices=int(lib.load().dlwp_conv3x3_wgrad_slices(n, h, w, c0 + c1, cout)), auto_hip=auto_hip)
    for f in fns:
        sp = spread(t[f])
        row.update({f"ms_{f}": sp["med"], f"ms_{f}_lo3": sp["lo3"], f"ms_{f}_hi3": sp["hi3"]})
    row["speedup"] = row["ms_torch"] / row["ms_hip"]
    row["hip_peak_frac"] = 2.0 * n * h * w * (c0 + c1) * cout * 9 / (row["ms_hip"] * 1e-3) / FP32_PEAK
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_wgrad.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_wgrad.py measures on an MI355X: no GPU found")
    if args.steps < 20:
        print("note: fewer than 20 repeats", file=sys.stderr)
    tags = [t for t in args.only.split(",") if t] or list(HPX.CASES) + list(CYL_CASES)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    shapes = set()
    for tag in tags:
        emit(bench_net(tag, args, shapes))
    if not args.no_layers:
        for shape in sorted(shapes):
            emit(bench_layer(shape, args))


if __name__ == "__main__":
    main()
