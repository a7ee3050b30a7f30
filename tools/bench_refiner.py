"""Times the PDE-Refiner noise scheduler: what the refinement loop and the training pair cost around the network.

Two forms alternate round by round in one process:
  today   what the loop does with a torch scheduler (the restated DDPM step as a torch composition): the start noise is
          torch.randn(shape) on the host plus an upload, the step is the elementwise torch expression driven by Python floats,
          its variance noise is drawn on the host with the scheduler's generator and uploaded
  device  schedulers.RefinerScheduler(noise="device"): ops.philox_normal for the start noise, ops.ddpm_step with in-kernel
          variance noise
The scheduler is the reference's: betas of scripts/train.py:76 with configs/training/diffusion.yaml (1000 steps, min_noise_std
4e-4), 5 inference steps (timesteps 800 .. 0).

Measured, each as the median over --rounds rounds of --iters iterations between two events (fastest and slowest beside it):
  step      the scheduler work of ONE refinement step at t > 0 (model output given)
  forecast  the scheduler work of one forecast step: the start noise and the 5 steps (4 with variance noise)
  pair      the training pair (scripts/train.py:228-255: residual, noise, add_noise, v-target) against its torch composition
            with torch.randn_like on the device
on [B, 1, 3, 32, 64] for B in {1, 16, 32} and the HEALPix-folded [12 B, 1, 3, 32, 32] for B in {1, 4}; and
  model     one whole DiffModernUNet forecast step at configs/model/diffusion_modernunet.yaml (batch --model-batch), both ways:
            the share the scheduler had.

One JSON per run: <out>/refiner_<tag>.json (default out: profiles/).
Usage: python tools/bench_refiner.py [--iters 20] [--rounds 7] [--warmup 5] [--tag mi355x] [--no-model] [--out DIR]
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
MODEL_CFG = dict(constant_channels=4, prescribed_channels=1, prognostic_channels=3, hidden_channels=[64, 128, 256, 1024],
                 activation="th.nn.GELU()", context_size=2, norm=True, use_scale_shift_norm=True, num_refinement_step=5)


class TorchScheduler:
    """today's path: the DDPM ancestral step (v-prediction, "fixed_small") as torch elementwise operations with host noise"""

    def __init__(self, ref, seed=0):
        self.ref = ref
        self.timesteps = ref.timesteps
        self._gen = torch.Generator().manual_seed(seed)

    def step(self, model_output, timestep, sample):
        t = int(timestep)
        sa, sb, c0, c1, sigma = self.ref.coefficients(t)
        x0 = sa * sample - sb * model_output
        prev = c0 * x0 + c1 * sample
        if t > 0:
            noise = torch.randn(model_output.shape, generator=self._gen).to(model_output.device)
            prev = prev + sigma * noise
        return SimpleNamespace(prev_sample=prev)


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


def bench_shape(shape, sched, args):
    from dlwp_benchmark_amd import ops  # noqa: F401  (loads the library before the clock starts)

    today = TorchScheduler(sched)
    g = torch.Generator(device=DEV).manual_seed(0)
    pred = torch.randn(shape, device=DEV, generator=g)
    sample = torch.randn(shape, device=DEV, generator=g)
    t_mid = sched.timesteps.tolist()[1]

    def forecast(s, start):
        y = start()
        for k in s.timesteps:
            y = s.step(pred, k, y).prev_sample
        return y

    forms = {
        "step_today": lambda: today.step(pred, t_mid, sample),
        "step_device": lambda: sched.step(pred, t_mid, sample),
        "forecast_today": lambda: forecast(today, lambda: torch.randn(shape).to(device=DEV)),
        "forecast_device": lambda: forecast(sched, lambda: sched.randn(shape, DEV)),
    }
    # the training pair: prognostic [B, 2, C, H, W], target [B, 1, C, H, W] (the folded HEALPix shape enters as lat-lon)
    prog = torch.randn((shape[0], 2) + tuple(shape[2:]), device=DEV, generator=g)
    target = torch.randn(shape, device=DEV, generator=g)
    k = 400
    acp = sched.alphas_cumprod.to(DEV)

    def pair_today():
        res = target - prog[:, 1:2]
        noise_factor = acp[k].view(-1, 1, 1, 1, 1)
        noise = torch.randn_like(res)
        y = (noise_factor ** 0.5) * res + ((1 - noise_factor) ** 0.5) * noise          # DDPMScheduler.add_noise
        return y, (noise_factor ** 0.5) * noise - ((1 - noise_factor) ** 0.5) * res

    forms["pair_today"] = pair_today
    forms["pair_device"] = lambda: sched.training_pair(prog, target, 2, k=k)
    res = alternate(forms, args.iters, args.rounds, args.warmup)
    sched.reseed()
    return {"shape": list(shape), "elements": pred.numel(), **res}


def bench_model(sched, args):
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd import weights as W

    model = M.DiffModernUNet(**MODEL_CFG)
    W.fill_state_dict(model, gain=0.7)
    model = model.to(DEV).eval()
    b, h, w = args.model_batch, 32, 64
    g = torch.Generator(device=DEV).manual_seed(1)
    constants = torch.randn(b, 1, 4, h, w, device=DEV, generator=g)
    prescribed = torch.randn(b, 3, 1, h, w, device=DEV, generator=g)
    prognostic = torch.randn(b, 3, 3, h, w, device=DEV, generator=g)          # context 2: ONE forecast step
    today = TorchScheduler(sched)
    forms = {
        "today": lambda: model(constants=constants, prescribed=prescribed, prognostic=prognostic, noise_scheduler=today),
        "device": lambda: model(constants=constants, prescribed=prescribed, prognostic=prognostic, noise_scheduler=sched),
    }
    res = alternate(forms, max(args.iters // 4, 2), args.rounds, max(args.warmup // 2, 2))
    sched.reseed()
    return {"batch": b, "grid": [h, w], "refinement_steps": 5, **res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tag", default="mi355x")
    ap.add_argument("--model-batch", type=int, default=16)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    from dlwp_benchmark_amd.schedulers import RefinerScheduler

    sched = RefinerScheduler.pde_refiner(1000, 4e-4, noise="device", seed=0)
    sched.set_timesteps(5)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": args.iters, "rounds": args.rounds,
              "timesteps": sched.timesteps.tolist(), "unit": "microseconds, median over rounds (lo, hi: fastest, slowest round)",
              "shapes": []}
    shapes = [(b, 1, 3, 32, 64) for b in (1, 16, 32)] + [(12 * b, 1, 3, 32, 32) for b in (1, 4)]
    for shape in shapes:
        entry = bench_shape(shape, sched, args)
        result["shapes"].append(entry)
        print(f"{list(shape)}: step today {entry['step_today']['us']} device {entry['step_device']['us']} | forecast today "
              f"{entry['forecast_today']['us']} device {entry['forecast_device']['us']} | pair today {entry['pair_today']['us']} "
              f"device {entry['pair_device']['us']} us", flush=True)
    if not args.no_model:
        result["model"] = bench_model(sched, args)
        m = result["model"]
        print(f"DiffModernUNet forecast step, batch {m['batch']}: today {m['today']['us']} device {m['device']['us']} us", flush=True)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"refiner_{args.tag}.json")
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
