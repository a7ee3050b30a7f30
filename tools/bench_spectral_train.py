"""A/B timing of the spectral weight gradient: `training.spectral_weight_grad` (two full rfft2 + gathers + einsum, the path
before the HIP entry) against dlwp_spectral_conv2d_wgrad_f32, alternated in one process on the same seeded inputs.

  wgrad   SpectralOperator.backward_weight alone
  op      SpectralConv2d forward + backward (dL/dx and both weight gradients)
  step    one FNO2DModule training step: 4-frame rollout, MSE, backward

Every shape is warmed on both paths, outputs of the two paths are compared at the timed sizes, and each figure is the
median over `--repeats` blocks of `--iters` calls between device events, with the spread (max - min) / median of the
blocks beside it.  For `wgrad` the bytes the three launches must move follow from the shape (x and grad_y read once,
grad_w written once, both kept spectra written and read once) and are stated against the 6.29 TB/s copy rate
tools/bench_fno_width.py uses.  Prints one JSON document; --out writes it to a file as well."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dlwp_benchmark_amd import training as T  # noqa: E402

COPY_BYTES_PER_S = 6.29e12
DEV = "cuda:0"
OP_SHAPES = [(16, 16), (32, 32), (64, 64), (128, 128), (256, 256), (64, 192)]   # Ci, Co at B = 32, 64 x 64, 12 x 12 modes
B, H, W, M1, M2 = 32, 64, 64, 12, 12
_HIP_WGRAD = T.SpectralOperator.backward_weight
PATHS = ["torch", "hip"]      # --hip-only drops "torch": the run a kernel trace of the HIP path alone is taken from


def _torch_wgrad(self, x, gy):
    return T.spectral_weight_grad(x.float(), gy.float(), self.rows_in, self.rows_out, self.n_cols, self.fwd_scale,
                                  self.inv_scale)


def use(path):
    T.SpectralOperator.backward_weight = _torch_wgrad if path == "torch" else _HIP_WGRAD


def block_ms(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def ab(fn, iters, repeats, warm=3):
    """fn() under both paths, alternated block by block; -> {path: (median ms, spread)}"""
    for path in PATHS:
        use(path)
        for _ in range(warm):
            fn()
    ms = {path: [] for path in PATHS}
    for _ in range(repeats):
        for path in PATHS:
            use(path)
            ms[path].append(block_ms(fn, iters))
    use("hip")
    out = {}
    for path, v in ms.items():
        med = statistics.median(v)
        out[path] = dict(ms=med, spread=(max(v) - min(v)) / med)
    return out


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def wgrad_bytes(ci, co, b, h, w, nr, nc):
    return 4 * b * (ci + co) * h * w + 8 * ci * co * nr * nc + 2 * 8 * nr * nc * b * (ci + co)


def bench_ops(iters, repeats):
    from dlwp_benchmark_amd.models import SpectralConv2d

    rows_out = []
    for ci, co in OP_SHAPES:
        gen = torch.Generator().manual_seed(ci * 1000 + co)
        x = torch.randn(B, ci, H, W, generator=gen).to(DEV)
        gy = torch.randn(B, co, H, W, generator=gen).to(DEV)
        rows, _ = T.pde_arena_rows(H, M1)
        op = T.SpectralOperator(ci, H, W, rows, rows, M2, 1.0, 1.0 / (H * W), DEV, out_channels=co)
        row = dict(ci=ci, co=co, batch=B, grid=[H, W], modes=[M1, M2])
        if "torch" in PATHS:
            use("torch")
            want = op.backward_weight(x, gy)
            use("hip")
            row["wgrad_rel_l2_hip_vs_torch"] = rel(op.backward_weight(x, gy), want)
            del want
        row["wgrad"] = ab(lambda: op.backward_weight(x, gy), iters, repeats)
        nbytes = wgrad_bytes(ci, co, B, H, W, 2 * M1, M2)
        t = row["wgrad"]["hip"]["ms"] * 1e-3
        row["wgrad_bytes"] = nbytes
        row["wgrad_hip_bytes_per_s"] = nbytes / t
        row["wgrad_hip_fraction_of_copy_rate"] = nbytes / t / COPY_BYTES_PER_S
        mod = SpectralConv2d(ci, co, M1, M2).to(DEV).train()
        xg = x.clone().requires_grad_(True)

        def fb():
            mod.zero_grad(set_to_none=True)
            xg.grad = None
            (mod(xg) * gy).sum().backward()

        row["op"] = ab(fb, iters, repeats)
        rows_out.append(row)
        print(json.dumps(row), flush=True)
        del op, mod, x, gy, xg
        torch.cuda.empty_cache()
    return rows_out


def bench_steps(iters, repeats):
    from dlwp_benchmark_amd.models import FNO2DModule
    from dlwp_benchmark_amd.synthetic import navier_stokes

    out = []
    for hidden in (32, 64):
        torch.manual_seed(hidden)
        net = FNO2DModule(n_modes=[12, 12], constant_channels=0, prescribed_channels=0, prognostic_channels=1,
                          hidden_channels=hidden, lifting_channels=256, projection_channels=256, n_layers=4,
                          context_size=1).to(DEV).train()
        prog = navier_stokes(B, 4, H, W, seed=5)[2].to(DEV)
        target = navier_stokes(B, 3, H, W, seed=6)[2].to(DEV)

        def step():
            net.zero_grad(set_to_none=True)
            torch.nn.functional.mse_loss(net(prognostic=prog), target).backward()

        grads = {}
        for path in PATHS:
            use(path)
            step()
            grads[path] = torch.cat([torch.view_as_real(p.grad).flatten() if p.grad.is_complex() else p.grad.flatten()
                                     for p in net.parameters()])
        row = dict(hidden=hidden, batch=B, frames=4, grid=[H, W], step=ab(step, iters, repeats))
        if "torch" in grads:
            row["grad_rel_l2_hip_vs_torch"] = rel(grads["hip"], grads["torch"])
        out.append(row)
        print(json.dumps(row), flush=True)
        del net
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", choices=["ops", "steps"], default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hip-only", action="store_true", help="time the HIP path alone (for a kernel trace of it)")
    a = ap.parse_args()
    if a.hip_only:
        PATHS.remove("torch")
    res = dict(tool="bench_spectral_train", device=torch.cuda.get_device_name(0), iters=a.iters, repeats=a.repeats,
               copy_bytes_per_s=COPY_BYTES_PER_S)
    if a.only in (None, "ops"):
        res["ops"] = bench_ops(a.iters, a.repeats)
    if a.only in (None, "steps"):
        res["steps"] = bench_steps(a.iters, a.repeats)
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
