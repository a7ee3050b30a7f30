"""Writes tests/golden/diffattn_grad_*.npz: gradients of the diffusion U-Net's AttentionBlock (reference modern_unet.py:520-585)
and of one diffusion training step of the PDE-Refiner networks built with attention=True (reference scripts/train.py:226-271:
fixed refinement step k, fixed noise, `single_forward`, MSE, `backward()`), run by the REAL reference classes on the CPU
(oracle.ref_import), with the filler weights of dlwp_benchmark_amd.weights -- the conventions of
tools/make_golden_diffusion_attention.py.  Only outputs are stored, never weights or inputs: each file carries the weight SHA,
the parameter spec, the case and the weights.normal names and shapes of its inputs as JSON, so a test regenerates the rest.

  op cases   loss, dL/dx and dL/dparameter in full; a parameter of more than FULL_MAX values (the 1024-channel block's
             projection) gets its norm and its projection on a fixed probe instead, as oracle/make_golden.py `gen_grads`
  net cases  loss, per-parameter norms and probe projections (gen_grads), and the full gradient of the small parameters

Runs where the reference tree is available:  python tools/make_golden_diffusion_attention_grad.py [ops] [nets]"""
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

GOLDEN = os.path.join(ROOT, "tests", "golden")
FULL_MAX = 1 << 16           # parameters up to this size are stored in full

# AttentionBlock alone: tag -> (ctor kwargs, input shape [B, C, H, W]); the op tags of make_golden_diffusion_attention.py
OP_CASES = {
    "c8": (dict(in_channels=8), (2, 8, 4, 8)),
    "c32": (dict(in_channels=32), (1, 32, 16, 32)),
    "c1024": (dict(in_channels=1024), (1, 1024, 4, 8)),
    "c48_dk16": (dict(in_channels=48, d_k=16), (2, 48, 5, 7)),
}

# networks: tag -> (class, ctor kwargs, batch, (H, W) [faces implied for HPX], betas, refinement step k)
NET_CASES = {
    "diffmunet_h32_64": ("DiffModernUNet", dict(constant_channels=2, prescribed_channels=1, prognostic_channels=2,
                                                hidden_channels=[32, 64], context_size=1, norm=True, attention=True,
                                                num_refinement_step=2), 2, (16, 32), [0.4, 0.2, 0.1], 1),
    "diffmunethpx_h32_64": ("DiffMUNetHPX", dict(constant_channels=1, prescribed_channels=1, prognostic_channels=2,
                                                 hidden_channels=[32, 64], context_size=1, norm=True, attention=True,
                                                 num_refinement_step=2), 1, (8, 8), [0.4, 0.2, 0.1], 1),
}


def op_names(tag):
    """weights.normal names of an op case's input and MSE target"""
    return f"golden/diffattn_grad/op/{tag}/x", f"golden/diffattn_grad/op/{tag}/target"


def grad_probe(tag, name, shape):
    """fixed pseudo-random direction a parameter gradient is projected on (same on every machine)"""
    return W.normal(f"golden/diffattn_grad/{tag}/probe/{name}", tuple(shape), 1.0)


def net_inputs(tag, cls, cfg, batch, hw):
    """[(argument, weights.normal name, shape)]: constants / prescribed / prognostic of the context and the target frame"""
    h, w = hw
    face = (12,) if cls.endswith("HPX") else ()
    cc, cp, cg, ctx = cfg["constant_channels"], cfg["prescribed_channels"], cfg["prognostic_channels"], cfg["context_size"]
    out = []
    if cc:
        out.append(("constants", f"golden/diffattn_grad/{tag}/constants", (batch, 1, cc) + face + (h, w)))
    if cp:
        out.append(("prescribed", f"golden/diffattn_grad/{tag}/prescribed", (batch, ctx, cp) + face + (h, w)))
    out.append(("prognostic", f"golden/diffattn_grad/{tag}/prognostic", (batch, ctx, cg) + face + (h, w)))
    out.append(("target", f"golden/diffattn_grad/{tag}/target", (batch, 1, cg) + face + (h, w)))
    return out


def train_step_loss(model, args, case):
    """scripts/train.py:226-271 for one batch: the noised residual target at refinement step k, `single_forward`, the MSE
    against (noise_factor^0.5 noise - signal_factor^0.5 target_res).  The noise is weights.normal data, not th.randn_like."""
    ctx = case["kwargs"]["context_size"]
    prog, target = args["prognostic"], args["target"]
    if prog.ndim == 6:                                   # einops "b t c f h w -> (b f) t c h w"
        fold = lambda t: t.permute(0, 3, 1, 2, 4, 5).reshape(t.shape[0] * t.shape[3], *t.shape[1:3], *t.shape[4:])
        input_prog, input_target = fold(prog), fold(target)
    else:
        input_prog, input_target = prog, target
    target_res = input_target - input_prog[:, ctx - 1:ctx]
    k = int(case["k"])
    acp = torch.cumprod(1.0 - torch.tensor(case["betas"], dtype=torch.float64), dim=0)
    noise_factor = float(acp[k])
    signal_factor = 1.0 - noise_factor
    noise = W.normal(case["noise"], tuple(target_res.shape), 1.0).to(target_res.device)
    y_noised = noise_factor ** 0.5 * target_res + (1.0 - noise_factor) ** 0.5 * noise      # DDPMScheduler.add_noise
    time = torch.full((input_prog.shape[0],), k, device=prog.device)
    prescribed = args.get("prescribed")
    out = model.single_forward(args.get("constants"), prescribed[:, 0:ctx] if prescribed is not None else None,
                               prog[:, 0:ctx], y_noised, time=time).unsqueeze(1)
    want = noise_factor ** 0.5 * noise - signal_factor ** 0.5 * target_res
    return torch.nn.functional.mse_loss(out, want)


def _save(name, **arrays):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


def _grads(tag, m, full_max):
    names, norms, projs, full = [], [], [], {}
    for name, p in m.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.detach().double()
        names.append(name)
        norms.append(float(g.norm()))
        projs.append(float((g * grad_probe(tag, name, g.shape).double()).sum()))
        if p.numel() <= full_max:
            full["grad::" + name] = p.grad.detach().numpy().astype(np.float32)
    return dict(names=np.array(json.dumps(names)), norms=np.array(norms), projs=np.array(projs), **full)


def gen_ops(mod):
    for tag, (kw, shape) in OP_CASES.items():
        m = mod.AttentionBlock(**kw)
        sha = W.fill_state_dict(m, gain=1.0)
        xn, tn = op_names(tag)
        x = W.normal(xn, shape, 1.0).requires_grad_(True)
        target = W.normal(tn, shape, 1.0)
        loss = torch.nn.functional.mse_loss(m(x), target)
        loss.backward()
        spec = json.dumps([(k, list(v.shape)) for k, v in m.named_parameters()])
        _save(f"diffattn_grad_op_{tag}", loss=np.array(loss.item()), grad_x=x.grad.numpy().astype(np.float32),
              sha=np.array(sha), param_spec=np.array(spec), kwargs=np.array(json.dumps(kw)),
              inputs=np.array(json.dumps([["x", xn, list(shape)], ["target", tn, list(shape)]])), **_grads(tag, m, FULL_MAX))


def gen_nets(mod):
    for tag, (cls, cfg, batch, hw, betas, k) in NET_CASES.items():
        m = getattr(mod, cls)(**cfg)
        sha = W.fill_state_dict(m, gain=0.7)      # the reference zero-initialises conv2 / output_layer: fill everything
        ins = net_inputs(tag, cls, cfg, batch, hw)
        args = {a: W.normal(n, s, 1.0) for a, n, s in ins}
        case = dict(cls=cls, kwargs=cfg, betas=betas, k=k, noise=f"golden/diffattn_grad/{tag}/noise")
        loss = train_step_loss(m, args, case)
        loss.backward()
        spec = json.dumps([(k_, list(v.shape)) for k_, v in m.named_parameters()])
        _save(f"diffattn_grad_net_{tag}", loss=np.array(loss.item()), sha=np.array(sha), param_spec=np.array(spec),
              kwargs=np.array(json.dumps(case)), inputs=np.array(json.dumps([[a, n, list(s)] for a, n, s in ins])),
              **_grads(tag, m, 4096))


def main():
    if not ref_import.reference_available():
        raise SystemExit("reference tree not available: these fixtures can only be regenerated where it is")
    mod = ref_import.load_reference_diffusion()
    os.makedirs(GOLDEN, exist_ok=True)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    only = set(sys.argv[1:])
    if not only or "ops" in only:
        gen_ops(mod)
    if not only or "nets" in only:
        gen_nets(mod)


if __name__ == "__main__":
    main()
