"""Writes tests/golden/spectral_wgrad_*.npz: gradients of the REAL reference SpectralConv2d (models/unet/unet.py:19-69,
imported through oracle.ref_import) on the CPU, at shapes the two fixtures of oracle/make_golden.py `gen_spectral` do not
reach -- the conventions of tools/make_golden_hpx_grad.py.  Inputs, weights and the probe come from
dlwp_benchmark_amd.weights.normal under the tags below, L = sum(y * r); only outputs are stored, never inputs or weights:
each file carries the input SHA, so a test regenerates the rest with `case_tensors`.

  tag                      Ci, Co   H x W    m1 x m2  B    reaches
  c24x40_32x64_m8x6_b3     24, 40   32 x 64  8 x 6    3    rectangular, Ci < Co, counts that are no multiples of 16
  c12x4_16x16_m4_b2        12, 4    16 x 16  4 x 4    2    rectangular, Ci > Co, the smallest padded geometry
  c5x2_12x20_m3x11_b2      5, 2     12 x 20  3 x 11   2    the Nyquist column kept (c_k = 1 there), H and W padded to 16
  c32_32x64_m8x6_b40       32, 32   32 x 64  8 x 6    40   the specialised-forward shape, more samples than one 32-chunk

`gw1` and `gw2` are stored in full.  No committed file may exceed 1 MiB and the weight gradients of the first and last
case take 0.7 MiB on their own, so `gx` and `y` are stored in full only up to GX_FULL_MAX values (the two small cases);
every file holds the norm of `gx`, its projection on a fixed probe, and the first four channels of sample 0 of `gx` and `y`.

Runs where the reference tree is available:  python tools/make_golden_spectral_grad.py [tag ...]"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dlwp_benchmark_amd import weights as W  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
GX_FULL_MAX = 1 << 15          # gx up to this many values is stored in full

# tag -> (Ci, Co, H, W, m1, m2, B)
CASES = {
    "c24x40_32x64_m8x6_b3": (24, 40, 32, 64, 8, 6, 3),
    "c12x4_16x16_m4_b2": (12, 4, 16, 16, 4, 4, 2),
    "c5x2_12x20_m3x11_b2": (5, 2, 12, 20, 3, 11, 2),
    "c32_32x64_m8x6_b40": (32, 32, 32, 64, 8, 6, 40),
}


def case_tensors(tag):
    """x, weights1, weights2, r of one case (the same on every machine)"""
    ci, co, h, w, m1, m2, b = CASES[tag]
    x = W.normal(f"golden/spectral_wgrad/{tag}/x", (b, ci, h, w), 1.0)
    w1 = W.normal(f"golden/spectral_wgrad/{tag}/w1", (ci, co, m1, m2, 2), 1.0 / ci)
    w2 = W.normal(f"golden/spectral_wgrad/{tag}/w2", (ci, co, m1, m2, 2), 1.0 / ci)
    r = W.normal(f"golden/spectral_wgrad/{tag}/r", (b, co, h, w), 1.0)
    return x, w1, w2, r


def gx_probe(tag):
    """fixed direction dL/dx is projected on where it is not stored in full"""
    ci, _, h, w, _, _, b = CASES[tag]
    return W.normal(f"golden/spectral_wgrad/{tag}/probe_gx", (b, ci, h, w), 1.0)


def tensor_sha(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    from oracle import ref_import

    if not ref_import.reference_available():
        raise SystemExit("reference tree not available: these fixtures can only be regenerated where it is")
    cls = ref_import.load_reference()["unet"].SpectralConv2d
    os.makedirs(GOLDEN, exist_ok=True)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for tag in (sys.argv[1:] or CASES):
        ci, co, h, w, m1, m2, b = CASES[tag]
        x, w1, w2, r = case_tensors(tag)
        mod = cls(ci, co, m1, m2)
        with torch.no_grad():
            mod.weights1.copy_(w1)
            mod.weights2.copy_(w2)
        xg = x.clone().requires_grad_(True)
        y = mod(xg)
        (y * r).sum().backward()
        gx = xg.grad.detach()
        out = dict(gw1=mod.weights1.grad.numpy().astype(np.float32), gw2=mod.weights2.grad.numpy().astype(np.float32),
                   y_norm=np.array(float(y.detach().double().norm())),
                   y_head=y.detach()[0, :4].numpy().astype(np.float32),
                   gx_norm=np.array(float(gx.double().norm())),
                   gx_proj=np.array(float((gx.double() * gx_probe(tag).double()).sum())),
                   gx_head=gx[0, :4].numpy().astype(np.float32),
                   case=np.array([ci, co, h, w, m1, m2, b]), sha=np.array(tensor_sha(x, w1, w2, r)))
        if gx.numel() <= GX_FULL_MAX:
            out["gx"] = gx.numpy().astype(np.float32)
            out["y"] = y.detach().numpy().astype(np.float32)
        path = os.path.join(GOLDEN, f"spectral_wgrad_{tag}.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
