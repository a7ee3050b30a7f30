"""Times the tail of a training step -- zero_grad + clip_grad_norm_ + AdamW.step (+ EMA update) -- and the loss forward + backward
on the parameter lists and output shapes of the five BASELINE configs C1-C5 (shapes only: random parameters and gradients, no
model runs).

Two forms alternate round by round in one process:
  hip    dlwp_benchmark_amd.optim: FusedAdamW.zero_grad() (storage kept), clip_grad_norm_(optimizer, lr), FusedAdamW.step(),
         ExponentialMovingAverage.update(); losses / ops.mse_loss
  torch  today's behaviour: optimizer.zero_grad() (set_to_none, the gradients are re-attached for the next iteration without
         device work), torch.nn.utils.clip_grad_norm_, torch.optim.AdamW at its defaults (foreach on the GPU); the EMA as the
         per-tensor loop of the usual class; F.mse_loss
Each round times --iters iterations of one form between two events (warm: --warmup iterations first); the figure is the median
over --rounds rounds, with the fastest and slowest beside it.  Launch counts come from torch.profiler (device kernels of one
iteration).  For the HIP tail the same iteration is also captured in a graph and replayed (`hip_graph_us`: the device's time
without the host's enqueue).  For C5, the largest list, step() alone is timed and reported as bytes per second at 28 B per
element (16 read, 12 written) beside the 8 TB/s HBM peak and the 6.3 TB/s copy rate the other tools use.

One JSON per run: profiles/train_step_<tag>.json.
Usage: python tools/bench_train_step.py [--only C1,C5] [--iters 20] [--rounds 7] [--warmup 5] [--tag mi355x]
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

HBM_PEAK = 8.0e12
COPY_RATE = 6.3e12
LR, WD, EMA_DECAY = 1e-3, 1e-5, 0.995
DEV = "cuda:0"


def configs():
    """tag -> (parameter shapes and dtypes, output shape [B, T, C, H, W]) of the BASELINE configs (bench.py: config_table and
    the headline)"""
    import bench
    import dlwp_benchmark_amd.models as M

    out = {}
    table = dict(bench.config_table())
    table["C2"] = ("FNO2DModule", dict(n_modes=[12, 12], constant_channels=0, prescribed_channels=0, prognostic_channels=1,
                                       hidden_channels=32, lifting_channels=256, projection_channels=256, n_layers=4,
                                       context_size=1), 32, 20, (64, 64))
    for tag in ("C1", "C2", "C3", "C4", "C5"):
        cls, cfg, batch, steps, (h, w) = table[tag][:5]
        model = getattr(M, cls)(**cfg)
        shapes = [(tuple(p.shape), p.dtype) for p in model.parameters() if p.requires_grad]     # fp32; complex64 in the FNO
        out[tag] = (shapes, (batch, steps, cfg["prognostic_channels"], h, w))
    return out


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters          # microseconds per iteration


def alternate(forms, iters, rounds, warmup):
    """{name: {"us": median, "lo": min, "hi": max}} with the forms taking turns round by round"""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            times[k].append(timed(fn, iters))
    return {k: {"us": round(statistics.median(v), 2), "lo": round(min(v), 2), "hi": round(max(v), 2)} for k, v in times.items()}


def launches(fn):
    """device kernels of one call of fn, or None where the profiler gives no device events"""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if getattr(e, "device_type", None) == torch.autograd.DeviceType.CUDA
            and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    return n or None


class TorchEma:
    """the usual per-tensor EMA loop (PDE-Refiner form): what ExponentialMovingAverage.update() replaces"""

    def __init__(self, params, decay):
        self.params, self.decay = params, decay
        self.shadow = [p.detach().clone() for p in params]

    def update(self):
        for i, p in enumerate(self.params):
            self.shadow[i] = ((1.0 - self.decay) * p.data + self.decay * self.shadow[i]).clone()


def bench_tail(shapes, args, want_bandwidth):
    from dlwp_benchmark_amd import optim as O

    g = torch.Generator(device=DEV).manual_seed(0)
    make = lambda: [torch.randn(s, device=DEV, generator=g, dtype=d).requires_grad_(True) for s, d in shapes]
    grads = [torch.randn(s, device=DEV, generator=g, dtype=d) * 1e-3 for s, d in shapes]
    p_hip, p_torch = make(), make()
    for p, gr in zip(p_hip, grads):
        p.grad = gr.clone()
    opt_hip = O.FusedAdamW(p_hip, lr=LR, weight_decay=WD)
    opt_torch = torch.optim.AdamW(p_torch, lr=LR, weight_decay=WD)
    holder = torch.nn.ParameterList([torch.nn.Parameter(p.detach()) for p in p_hip])
    ema_hip = O.ExponentialMovingAverage(holder, EMA_DECAY)
    ema_hip.register()
    ema_torch = TorchEma(p_torch, EMA_DECAY)

    def hip_tail():
        opt_hip.zero_grad()
        O.clip_grad_norm_(opt_hip, LR)
        opt_hip.step()

    def torch_tail():
        opt_torch.zero_grad()
        for p, gr in zip(p_torch, grads):          # the next backward's gradients: no device work
            p.grad = gr
        torch.nn.utils.clip_grad_norm_(p_torch, LR)
        opt_torch.step()

    forms = {"hip": hip_tail, "torch": torch_tail, "hip_ema": ema_hip.update, "torch_ema": ema_torch.update}
    res = alternate(forms, args.iters, args.rounds, args.warmup)
    out = {"tensors": len(shapes), "elements": int(sum(O._nfloats(p) for p in p_hip)), "tail": {}}
    for k in forms:
        out["tail"][k] = dict(res[k], launches=launches(forms[k]))
    # the HIP tail as a recorded step: the device's time alone
    opt_hip.sync()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip_tail()
    out["tail"]["hip_graph_us"] = alternate({"g": graph.replay}, args.iters, args.rounds, args.warmup)["g"]["us"]
    if want_bandwidth:
        us = alternate({"step": opt_hip.step}, args.iters, args.rounds, args.warmup)["step"]["us"]
        rate = 28.0 * out["elements"] / (us * 1e-6)
        out["adamw_step"] = {"us": us, "bytes_per_element": 28, "bytes_per_s": rate, "of_hbm_peak": round(rate / HBM_PEAK, 3),
                             "of_copy_rate": round(rate / COPY_RATE, 3), "note": "header kernel and host enqueue included"}
    return out


def bench_loss(shape, args):
    from dlwp_benchmark_amd import ops

    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(shape, device=DEV, generator=g).requires_grad_(True)
    t = torch.randn(shape, device=DEV, generator=g)

    def hip():
        x.grad = None
        ops.mse_loss(x, t).backward()

    def torch_form():
        x.grad = None
        F.mse_loss(x, t).backward()

    forms = {"hip": hip, "torch": torch_form}
    res = alternate(forms, args.iters, args.rounds, args.warmup)
    return {"shape": list(shape), **{k: dict(res[k], launches=launches(forms[k])) for k in forms}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tag", default="mi355x")
    args = ap.parse_args()
    only = [t for t in args.only.split(",") if t]
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": args.iters, "rounds": args.rounds,
              "lr": LR, "weight_decay": WD, "configs": {}}
    for tag, (shapes, out_shape) in configs().items():
        if only and tag not in only:
            continue
        entry = bench_tail(shapes, args, want_bandwidth=tag == "C5")
        entry["loss"] = bench_loss(out_shape, args)
        result["configs"][tag] = entry
        t, l = entry["tail"], entry["loss"]
        print(f"{tag}: {entry['tensors']} tensors, {entry['elements']} elements | tail hip {t['hip']['us']} us "
              f"({t['hip']['launches']} launches, graph {t['hip_graph_us']} us) torch {t['torch']['us']} us "
              f"({t['torch']['launches']}) | ema hip {t['hip_ema']['us']} torch {t['torch_ema']['us']} | loss fwd+bwd hip "
              f"{l['hip']['us']} ({l['hip']['launches']}) torch {l['torch']['us']} ({l['torch']['launches']})", flush=True)
        if "adamw_step" in entry:
            print(f"{tag}: AdamW step {entry['adamw_step']['us']} us = {entry['adamw_step']['bytes_per_s'] / 1e12:.2f} TB/s",
                  flush=True)
    path = os.path.join(ROOT, "profiles", f"train_step_{args.tag}.json")
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
