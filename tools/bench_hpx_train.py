"""Times one scripts/train.py-style training step of the HEALPix backbones: a forward over sequence length 3, the rollout MSE,
`backward()` -- at batch 32 and the widths of the reference yaml configs (unet_inverted.yaml, modernunet_invertedHPX.yaml,
convlstm.yaml, diffusion_modernunet_small_inv.yaml), faces folded into the batch (Bt = 12 B).

Per network, one JSON line: the HIP backward (dlwp_conv3x3_hpx_bwd_data_f32 for dX, dlwp_healpix_pad_f32 + MIOpen for dW)
and the torch recomputation (DLWP_TRAIN_TORCH_BACKWARD=1), alternated step by step in one process:
  ms_hip / ms_torch     median step time over --steps steps after --warmup warm-up steps of each
  mem_hip / mem_torch   peak bytes allocated during a step
With --layers, one line per HEALPix 3x3 convolution shape met in the HIP steps:
  ms_dx                 ops.conv3x3_hpx_backward_data alone (HIP events, median of --reps)
  ms_torch_dx           the recomputation it replaces: autograd of training.conv3x3_torch (int64 gather + MIOpen) for dX
  dx_peak_frac          2 n H W Cin Cout 9 FLOPs / ms_dx against the fp32 peak (157.3 TF)

Usage: python tools/bench_hpx_train.py [--batch 32] [--steps 20] [--warmup 3] [--only unethpx_n32,...] [--layers] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_PEAK = 157.3e12
GELU = "th.nn.GELU()"
# tag -> (class, ctor kwargs, nside); ConvLSTMHPX takes batch_size / height / width, filled in at build time
CASES = {
    "unethpx_n32": ("UNetHPX", dict(constant_channels=4, prescribed_channels=1, prognostic_channels=3,
                                    hidden_channels=[136, 68, 34], n_convolutions=2, activation=GELU, context_size=2), 32),
    "munethpx_n32": ("MUNetHPX", dict(constant_channels=4, prescribed_channels=1, prognostic_channels=3,
                                      hidden_channels=[136, 68, 34], activation=GELU, context_size=2, norm=False), 32),
    "munethpx_n64": ("MUNetHPX", dict(constant_channels=4, prescribed_channels=1, prognostic_channels=3,
                                      hidden_channels=[136, 68, 34], activation=GELU, context_size=2, norm=False), 64),
    "convlstmhpx_n32": ("ConvLSTMHPX", dict(constant_channels=4, prescribed_channels=1, prognostic_channels=8,
                                            hidden_sizes=[16, 16], bias=True, context_size=1), 32),
    "diffmunethpx_n32": ("DiffMUNetHPX", dict(constant_channels=4, prescribed_channels=1, prognostic_channels=3,
                                              hidden_channels=[64, 32, 16], activation=GELU, context_size=2, norm=True,
                                              use_scale_shift_norm=True, num_refinement_step=5, attention=False), 32),
}
SEQ = 3


def build(tag, batch, case=None):
    """the model of CASES[tag] (or of `case`, an entry of the same form) in train mode and a closure that returns its loss"""
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd.weights import fill_state_dict

    cls, cfg, n = case or CASES[tag]
    cfg = dict(cfg)
    if cls == "ConvLSTMHPX":
        cfg.update(batch_size=batch, height=n, width=n)
    model = getattr(M, cls)(**cfg)
    fill_state_dict(model, gain=0.7)
    model = model.to("cuda:0").train()
    g = torch.Generator(device="cuda:0").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda:0", generator=g)
    cc, cp, cg = cfg["constant_channels"], cfg["prescribed_channels"], cfg["prognostic_channels"]
    ins = dict(constants=rnd(batch, 1, cc, 12, n, n), prescribed=rnd(batch, SEQ, cp, 12, n, n),
               prognostic=rnd(batch, SEQ, cg, 12, n, n))
    ctx = cfg["context_size"]
    if cls == "DiffMUNetHPX":
        # train.py:226-271 at a fixed refinement step: single_forward on the noised residual target, MSE
        ins["noised"] = rnd(batch * 12, 1, cg, n, n)
        ins["want"] = rnd(batch * 12, 1, cg, n, n)

        def loss_fn():
            time = torch.full((batch * 12,), 2, device="cuda:0")
            out = model.single_forward(ins["constants"], ins["prescribed"][:, :ctx], ins["prognostic"][:, :ctx],
                                       ins["noised"], time=time).unsqueeze(1)
            return torch.nn.functional.mse_loss(out, ins["want"])
    else:
        from oracle.make_golden import rollout_mse

        def loss_fn():
            y = model(constants=ins["constants"], prescribed=ins["prescribed"], prognostic=ins["prognostic"])
            return rollout_mse(y, ins["prognostic"], ctx)
    return model, loss_fn


def step_ms(model, loss_fn, torch_backward):
    os.environ["DLWP_TRAIN_TORCH_BACKWARD"] = "1" if torch_backward else "0"
    for p in model.parameters():
        p.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    loss_fn().backward()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base


def bench_net(tag, args, shapes):
    from dlwp_benchmark_amd import ops

    model, loss_fn = build(tag, args.batch)
    real = ops.conv3x3_hpx_backward_data

    def recording(dy, weight, cin):
        shapes.add((tuple(dy.shape), int(cin)))
        return real(dy, weight, cin)

    ops.conv3x3_hpx_backward_data = recording
    try:
        for _ in range(args.warmup):
            step_ms(model, loss_fn, False)
            step_ms(model, loss_fn, True)
        hip, tor, mh, mt = [], [], 0, 0
        for _ in range(args.steps):
            t, m = step_ms(model, loss_fn, False)
            hip.append(t); mh = max(mh, m)
            t, m = step_ms(model, loss_fn, True)
            tor.append(t); mt = max(mt, m)
    finally:
        ops.conv3x3_hpx_backward_data = real
        os.environ.pop("DLWP_TRAIN_TORCH_BACKWARD", None)
    cls, _, n = CASES[tag]
    row = dict(kind="step", tag=tag, cls=cls, nside=n, batch=args.batch, faces=12 * args.batch, seq=SEQ, steps=args.steps,
               ms_hip=statistics.median(hip), ms_torch=statistics.median(tor),
               speedup=statistics.median(tor) / statistics.median(hip), mem_hip=mh, mem_torch=mt,
               ms_hip_min=min(hip), ms_torch_min=min(tor))
    del model
    torch.cuda.empty_cache()
    return row


def _event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def bench_layer(shape, cin, reps):
    from dlwp_benchmark_amd import healpix as H
    from dlwp_benchmark_amd import ops, training as T

    n, cout, h, w = shape
    g = torch.Generator(device="cuda:0").manual_seed(1)
    dy = torch.randn(n, cout, h, w, device="cuda:0", generator=g)
    wt = torch.randn(cout, cin, 3, 3, device="cuda:0", generator=g) * (9 * cin) ** -0.5
    x = torch.randn(n, cin, h, w, device="cuda:0", generator=g, requires_grad=True)
    table = H.device_table(h, w, 1, "cuda:0")
    ms = _event_ms(lambda: ops.conv3x3_hpx_backward_data(dy, wt, cin), reps)

    def recompute():
        with torch.enable_grad():
            torch.autograd.grad(T.conv3x3_torch(x, None, wt, None, None, 0, 0, table), x, dy)

    ms_t = _event_ms(recompute, reps)
    flops = 2.0 * n * h * w * cin * cout * 9
    return dict(kind="dx", faces=n, nside=h, cin=cin, cout=cout, ms_dx=ms, ms_torch_dx=ms_t, speedup=ms_t / ms,
                dx_peak_frac=flops / (ms * 1e-3) / FP32_PEAK)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="")
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    tags = [t for t in args.only.split(",") if t] or list(CASES)
    out = open(args.out, "a") if args.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    shapes = set()
    for tag in tags:
        emit(bench_net(tag, args, shapes))
    if args.layers:
        for shape, cin in sorted(shapes):
            emit(bench_layer(shape, cin, args.reps))


if __name__ == "__main__":
    main()
