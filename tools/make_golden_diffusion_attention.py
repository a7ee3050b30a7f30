"""Writes tests/golden/diffattn_*.npz: the diffusion U-Net's AttentionBlock (reference modern_unet.py:520-585) and the
PDE-Refiner networks built with attention=True, run by the REAL reference classes (oracle.ref_import), with the filler
weights of dlwp_benchmark_amd.weights and the restated DDPM scheduler -- the conventions of oracle/make_golden.py
`gen_diffusion`.  Only outputs are stored, never weights: each file carries the weight SHA, the parameter / state-dict specs,
the case's constructor kwargs and the weights.normal names and shapes of its inputs as JSON, so a test regenerates
everything else itself.  Runs where the reference tree is available:  python tools/make_golden_diffusion_attention.py"""
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
from oracle.restate.ddpm import DDPMSchedulerRestated  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 2024          # torch.manual_seed before a network forward: the start noise comes from the host's global generator

# AttentionBlock alone: tag -> (ctor kwargs, input shape [B, C, H, W])
OP_CASES = {
    "c8": (dict(in_channels=8), (2, 8, 4, 8)),                      # tiny config width
    "c32": (dict(in_channels=32), (1, 32, 16, 32)),                 # N = 512
    "c64_l0": (dict(in_channels=64), (2, 64, 32, 64)),              # level 0 of the yaml config, N = 2048
    "c1024": (dict(in_channels=1024), (1, 1024, 4, 8)),             # level 3 of the yaml config, d = 1024
    "c48_dk16": (dict(in_channels=48, d_k=16), (2, 48, 5, 7)),      # odd N, non-default d_k
}

# networks: tag -> (class, ctor kwargs, (batch, frames), (H, W) [faces implied for HPX], betas, inference steps)
NET_CASES = {
    "diffmunet_h32_64": ("DiffModernUNet", dict(constant_channels=2, prescribed_channels=1, prognostic_channels=2,
                                                hidden_channels=[32, 64], context_size=1, norm=True, attention=True,
                                                num_refinement_step=2), (1, 3), (16, 32), [0.4, 0.2, 0.1], 2),
    "diffmunethpx_h32_64": ("DiffMUNetHPX", dict(constant_channels=1, prescribed_channels=1, prognostic_channels=2,
                                                 hidden_channels=[32, 64], context_size=1, norm=True, attention=True,
                                                 num_refinement_step=2), (1, 2), (8, 8), [0.4, 0.2, 0.1], 2),
    "diffmunet_h8_16": ("DiffModernUNet", dict(constant_channels=0, prescribed_channels=0, prognostic_channels=2,
                                               hidden_channels=[8, 16], context_size=1, norm=False, use_scale_shift_norm=False,
                                               attention=True, num_refinement_step=2), (1, 3), (8, 16), [0.4, 0.2, 0.1], 2),
}


def _specs(m):
    spec = [(k, list(v.shape)) for k, v in m.named_parameters()]
    full = [(k, list(v.shape), str(v.dtype).replace("torch.", "")) for k, v in m.state_dict().items()]
    return json.dumps(spec), json.dumps(full)


def _save(name, **arrays):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


def _inputs(tag, cls, cfg, batch, frames, hw):
    """[(argument, weights.normal name, shape)] of a network case's inputs (None-valued arguments left out)."""
    h, w = hw
    face = (12,) if cls.endswith("HPX") else ()
    cc, cp, cg = cfg["constant_channels"], cfg["prescribed_channels"], cfg["prognostic_channels"]
    out = []
    if cc:
        out.append(("constants", f"golden/diffattn/{tag}/constants", (batch, 1, cc) + face + (h, w)))
    if cp:
        out.append(("prescribed", f"golden/diffattn/{tag}/prescribed", (batch, frames, cp) + face + (h, w)))
    out.append(("prognostic", f"golden/diffattn/{tag}/prognostic", (batch, frames, cg) + face + (h, w)))
    return out


def gen_ops(mod):
    for tag, (kw, shape) in OP_CASES.items():
        m = mod.AttentionBlock(**kw).eval()
        sha = W.fill_state_dict(m, gain=1.0)
        name = f"golden/diffattn/op/{tag}/x"
        x = W.normal(name, shape, 1.0)
        with torch.no_grad():
            y = m(x.clone())
        spec, full = _specs(m)
        _save(f"diffattn_op_{tag}", y=y.numpy().astype(np.float32), sha=np.array(sha), param_spec=np.array(spec),
              state_spec=np.array(full), kwargs=np.array(json.dumps(kw)),
              inputs=np.array(json.dumps([["x", name, list(shape)]])))


def gen_nets(mod):
    for tag, (cls, cfg, (batch, frames), hw, betas, nsteps) in NET_CASES.items():
        m = getattr(mod, cls)(**cfg).eval()
        sha = W.fill_state_dict(m, gain=0.7)      # the reference zero-initialises conv2 / output_layer: fill everything
        ins = _inputs(tag, cls, cfg, batch, frames, hw)
        args = {a: W.normal(n, s, 1.0) for a, n, s in ins}
        sched = DDPMSchedulerRestated(betas, seed=7)
        sched.set_timesteps(nsteps)
        torch.manual_seed(SEED)
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):   # the reference forward prints its progress
            y = m(constants=args.get("constants"), prescribed=args.get("prescribed"), prognostic=args["prognostic"],
                  noise_scheduler=sched, target=None)
        spec, full = _specs(m)
        case = dict(cls=cls, kwargs=cfg, betas=betas, nsteps=nsteps, seed=SEED, scheduler_seed=7)
        _save(f"diffattn_model_{tag}", y=y.numpy().astype(np.float32), sha=np.array(sha), param_spec=np.array(spec),
              state_spec=np.array(full), kwargs=np.array(json.dumps(case)),
              inputs=np.array(json.dumps([[a, n, list(s)] for a, n, s in ins])))


def main():
    if not ref_import.reference_available():
        raise SystemExit("reference tree not available: these fixtures can only be regenerated where it is")
    mod = ref_import.load_reference_diffusion()
    os.makedirs(GOLDEN, exist_ok=True)
    only = set(sys.argv[1:])
    if not only or "ops" in only:
        gen_ops(mod)
    if not only or "nets" in only:
        gen_nets(mod)


if __name__ == "__main__":
    main()
