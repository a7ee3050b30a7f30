"""Writes tests/golden/grad_hpx_*.npz and tests/golden/healpix_pad_grad_p*.npz: gradients of the HEALPix backbones and of
HEALPixPadding, run by the REAL reference classes on the CPU (oracle.ref_import) with the filler weights of
dlwp_benchmark_amd.weights -- the conventions of oracle/make_golden.py `gen_grads` and
tools/make_golden_diffusion_attention_grad.py.  Only outputs are stored, never weights or inputs: each file carries the weight
SHA and the case, so a test regenerates the rest.

  network cases  the configs and inputs of oracle/make_golden.py HPX_*_CASES (hpx_inputs); loss = rollout MSE
                 (train.py:263-271, make_golden.rollout_mse); per parameter the gradient norm and its projection on a fixed
                 probe, and the full gradient of the parameters up to FULL_MAX values
  padding cases  HEALPixPadding(p) on x [B*12, C, n, n]; loss = sum(pad(x) * r) for a fixed probe r; dL/dx = pad^T r

Runs where the reference tree is available:  python tools/make_golden_hpx_grad.py [nets] [pad]"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dlwp_benchmark_amd import weights as W  # noqa: E402
from oracle import ref_import  # noqa: E402
from oracle.make_golden import (HPX_CONVLSTM_CASES, HPX_MODEL_CASES, HPX_MUNET_CASES, hpx_inputs,  # noqa: E402
                                rollout_mse)

GOLDEN = os.path.join(ROOT, "tests", "golden")
FULL_MAX = 4096              # parameters up to this size are stored in full

# fixture tag -> (reference module key, class, base case tag, (ctor kwargs, (batch, frames), (H, W)))
NET_CASES = {
    "unethpx_h4_8x8": ("unet", "UNetHPX", "unethpx_h4_8x8", HPX_MODEL_CASES["unethpx_h4_8x8"]),
    "munethpx_h16_8_norm": ("unet", "MUNetHPX", "munethpx_h16_8_norm", HPX_MUNET_CASES["munethpx_h16_8_norm"]),
    "munethpx_h8_16": ("unet", "MUNetHPX", "munethpx_h8_16", HPX_MUNET_CASES["munethpx_h8_16"]),
    "convlstmhpx_h8_8x8": ("convlstm", "ConvLSTMHPX", "convlstmhpx_h8_8x8", HPX_CONVLSTM_CASES["convlstmhpx_h8_8x8"]),
}

# padding cases: p -> (samples, channels, nside)
PAD_CASES = {1: (2, 3, 8), 2: (2, 3, 8), 4: (1, 2, 4)}


def grad_probe(tag, name, shape):
    """fixed pseudo-random direction a parameter gradient is projected on (same on every machine)"""
    return W.normal(f"golden/grad_hpx/{tag}/probe/{name}", tuple(shape), 1.0)


def pad_names(p):
    """weights.normal names of a padding case's input and probe"""
    return f"golden/hpxpad_grad/p{p}/x", f"golden/hpxpad_grad/p{p}/probe"


def _save(name, **arrays):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


def gen_nets(ref):
    for tag, (key, cls, base, (cfg, (batch, frames), hw)) in NET_CASES.items():
        m = getattr(ref[key], cls)(**cfg)
        sha = W.fill_state_dict(m, gain=1.0)     # the HPX model fixtures' gain; MUNetHPX zero-initialises: fill everything
        constants, prescribed, prognostic = hpx_inputs(base, cfg, batch, frames, hw)
        with contextlib.redirect_stdout(io.StringIO()):     # the reference MUNetHPX forward prints shapes
            y = m(constants=constants, prescribed=prescribed, prognostic=prognostic)
        loss = rollout_mse(y, prognostic, cfg["context_size"])
        loss.backward()
        names, norms, projs, full = [], [], [], {}
        for name, p_ in m.named_parameters():
            if p_.grad is None:
                continue
            g = p_.grad.detach().double()
            names.append(name)
            norms.append(float(g.norm()))
            projs.append(float((g * grad_probe(tag, name, g.shape).double()).sum()))
            if p_.numel() <= FULL_MAX:
                full["grad::" + name] = p_.grad.detach().numpy().astype(np.float32)
        case = dict(cls=cls, base=base, batch=batch, frames=frames, hw=list(hw))
        _save(f"grad_hpx_{tag}", names=np.array(json.dumps(names)), norms=np.array(norms), projs=np.array(projs),
              loss=np.array(float(loss.detach())), sha=np.array(sha), case=np.array(json.dumps(case)), **full)


def gen_pad(ref):
    pad_cls = ref["utils"].HEALPixPadding
    for p, (b, c, n) in PAD_CASES.items():
        xn, rn = pad_names(p)
        x = W.normal(xn, (b * 12, c, n, n), 1.0).requires_grad_(True)
        r = W.normal(rn, (b * 12, c, n + 2 * p, n + 2 * p), 1.0)
        loss = (pad_cls(padding=p)(x) * r).sum()
        loss.backward()
        _save(f"healpix_pad_grad_p{p}", grad_x=x.grad.numpy().astype(np.float32), loss=np.array(float(loss.detach())),
              shape=np.array([b * 12, c, n, n]))


def main():
    if not ref_import.reference_available():
        raise SystemExit("reference tree not available: these fixtures can only be regenerated where it is")
    ref = ref_import.load_reference()
    os.makedirs(GOLDEN, exist_ok=True)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    only = set(sys.argv[1:])
    if not only or "nets" in only:
        gen_nets(ref)
    if not only or "pad" in only:
        gen_pad(ref)


if __name__ == "__main__":
    main()
