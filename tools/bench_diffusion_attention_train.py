"""Times a training step (forward + backward) of the diffusion U-Net's AttentionBlock at every encoder level of
configs/model/diffusion_modernunet.yaml (hidden_channels [64, 128, 256, 1024], 4 heads, d_k = C) on the 32 x 64 lat-lon grid
(B = 32) and on HEALPix nside 32 (faces folded into the batch: Bt = 12 B) -- the shapes of tools/bench_diffusion_attention.py --
and the nside-64 level-0 shape at the training batch of configs/training/diffusion.yaml (B = 32: Bt = 384, 64 x 64 faces,
N = 4096), where only the HIP path runs: the torch composition would need about 300 GB.

For each block row, one JSON line:
  ms_hip          m(x).backward(gy) on the training path of AttentionBlock: the two Linears (torch), dlwp_global_attn_f32,
                  dlwp_global_attn_bwd_f32
  ms_torch        the same step through the reference composition in fp32 torch on the same GPU (autograd of Linear,
                  einsum, softmax(dim=1), einsum, Linear, + x)
  ms_core_bwd     the attention backward alone (ops.global_attention_backward, three launches), HIP events
  flops_core_bwd  16 N^2 d per (sample, head): S three times, dP twice, dV, dK, dQ
  core_bwd_peak_frac   flops_core_bwd / ms_core_bwd against the fp32 matrix peak (157.3 TF, v_mfma_f32_16x16x4_f32)
  mem_hip / mem_torch  peak bytes allocated above the inputs during the step
  rel_l2_dx_vs_torch   the input gradients of the two paths
With --network, two more lines per mesh: DiffModernUNet single_forward + MSE + backward at the yaml widths (B = 32 lat-lon),
attention off and on.

Usage: python tools/bench_diffusion_attention_train.py [--batch 32] [--hpx-batch 4] [--reps 10] [--network]
       [--only latlon:0,healpix:0,nside64:0] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_MATRIX_PEAK = 157.3e12
HIDDEN = [64, 128, 256, 1024]
HEADS = 4


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def _peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def torch_block(m, x):
    """the reference arithmetic (modern_unet.py:551-585) as fp32 torch operators"""
    b, c, h, w = x.shape
    t = x.reshape(b, c, h * w).permute(0, 2, 1)
    qkv = torch.nn.functional.linear(t, m.projection.weight, m.projection.bias).view(b, h * w, m.n_heads, 3 * m.d_k)
    q, k, v = torch.chunk(qkv, 3, dim=-1)
    attn = torch.einsum("bihd,bjhd->bijh", q, k) * m.scale
    attn = attn.softmax(dim=1)
    res = torch.einsum("bijh,bjhd->bihd", attn, v).reshape(b, h * w, m.n_heads * m.d_k)
    res = torch.nn.functional.linear(res, m.output.weight, m.output.bias) + t
    return res.permute(0, 2, 1).reshape(b, c, h, w)


def block_row(mesh, c, bt, hw, reps, dev, with_torch=True):
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd.models.diffusion import AttentionBlock
    from dlwp_benchmark_amd.weights import fill_state_dict

    m = AttentionBlock(c)
    fill_state_dict(m)
    m = m.to(dev).train()
    h, w = hw
    n, d = h * w, m.d_k
    x = torch.randn(bt, c, h, w, device=dev).requires_grad_(True)
    gy = torch.randn(bt, c, h, w, device=dev)
    row = dict(op="AttentionBlock.train_step", mesh=mesh, channels=c, heads=HEADS, d=d, batch=bt, grid=[h, w], tokens=n)

    def hip_step():
        x.grad = None
        m(x).backward(gy)

    def torch_step():
        x.grad = None
        torch_block(m, x).backward(gy)

    row["ms_hip"] = _time(hip_step, reps)
    row["mem_hip"] = _peak(hip_step)
    dx_hip = x.grad.clone()
    with torch.no_grad():
        qkv = ops.linear_any(x.detach().reshape(bt, c, n).transpose(1, 2).contiguous(), m.projection)
        _, stats = ops.global_attention(qkv, HEADS, d, return_stats=True)
        go = torch.randn(bt, n, HEADS * d, device=dev)
        row["ms_core_bwd"] = _time(lambda: ops.global_attention_backward(qkv, stats, go, HEADS, d), reps)
    del qkv, stats, go
    row["ms_torch"] = row["mem_torch"] = None
    if with_torch:
        try:
            row["ms_torch"] = _time(torch_step, reps)
            row["mem_torch"] = _peak(torch_step)
            row["rel_l2_dx_vs_torch"] = float(torch.linalg.vector_norm((dx_hip - x.grad).double()) /
                                              torch.linalg.vector_norm(x.grad.double()))
        except torch.cuda.OutOfMemoryError:
            row["ms_torch"] = row["mem_torch"] = None
    x.grad = None
    torch.cuda.empty_cache()
    row["flops_core_bwd"] = 16.0 * n * n * d * bt * HEADS
    row["core_bwd_tflops"] = row["flops_core_bwd"] / (row["ms_core_bwd"] * 1e-3) / 1e12
    row["core_bwd_peak_frac"] = row["core_bwd_tflops"] * 1e12 / FP32_MATRIX_PEAK
    row["peak"] = "fp32 matrix 157.3 TF (v_mfma_f32_16x16x4_f32)"
    if row["ms_torch"]:
        row["speedup_vs_torch"] = row["ms_torch"] / row["ms_hip"]
        row["mem_ratio_torch_over_hip"] = row["mem_torch"] / row["mem_hip"]
    return row


def network_rows(batch, reps, dev):
    from dlwp_benchmark_amd.models import DiffModernUNet
    from dlwp_benchmark_amd.weights import fill_state_dict

    rows = []
    shape = (32, 64)
    for attention in (False, True):
        m = DiffModernUNet(hidden_channels=HIDDEN, attention=attention)
        fill_state_dict(m, gain=0.7)
        m = m.to(dev).train()
        consts = torch.randn(batch, 1, 4, *shape, device=dev)
        prog = torch.randn(batch, 1, 1, *shape, device=dev)
        y = torch.randn(batch, 1, 1, *shape, device=dev)
        want = torch.randn(batch, 1, *shape, device=dev)
        t = torch.full((batch,), 3, dtype=torch.long, device=dev)

        def step():
            m.zero_grad(set_to_none=True)
            torch.nn.functional.mse_loss(m.single_forward(consts, None, prog, y, t), want).backward()

        ms = _time(step, reps)
        mem = _peak(step)
        rows.append(dict(op="DiffModernUNet.single_forward+backward", attention=attention, batch=batch, grid=list(shape),
                         hidden=HIDDEN, ms=ms, mem=mem))
        del m
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hpx-batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--network", action="store_true")
    ap.add_argument("--only", default="", help="comma-separated mesh:level rows, e.g. nside64:0 (default: every row)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffusion_attention_train.jsonl"))
    a = ap.parse_args()
    dev = "cuda:0"
    only = set(filter(None, a.only.split(",")))
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    for mesh, bt, grid in (("latlon", a.batch, (32, 64)), ("healpix", 12 * a.hpx_batch, (32, 32))):
        for lvl, c in enumerate(HIDDEN):
            if not only or f"{mesh}:{lvl}" in only:
                emit(block_row(mesh, c, bt, (grid[0] >> lvl, grid[1] >> lvl), a.reps, dev))
    if not only or "nside64:0" in only:
        emit(block_row("healpix_nside64", HIDDEN[0], 12 * a.batch, (64, 64), max(2, a.reps // 5), dev, with_torch=False))
    if a.network:
        for r in network_rows(a.batch, a.reps, dev):
            emit(r)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
