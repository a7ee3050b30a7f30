"""The PDE-Refiner backbones driven by schedulers.RefinerScheduler: the golden trajectories of tests/test_diffusion_gpu.py with
the fused step fed host noise (noise="host"), the device noise mode against a loop written out here, and one training step
from training_pair's outputs."""
import json

import pytest
import torch
import torch.nn.functional as F

from helpers import load_golden, per_step_rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = "diffmunet_h8_16_bias"


def _cases():
    from oracle.make_golden import DIFFUSION_CASES

    return list(DIFFUSION_CASES)


def _model_and_inputs(tag, train=False):
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd.weights import fill_by_spec
    from oracle.make_golden import DIFFUSION_CASES, diffusion_inputs

    cls, cfg, (batch, frames), hw, betas, nsteps = DIFFUSION_CASES[tag]
    g = load_golden(f"model_{tag}")
    sd, sha = fill_by_spec(json.loads(str(g["param_spec"])), gain=0.7)
    assert sha == str(g["sha"])
    model = getattr(M, cls)(**cfg)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and not missing
    model = model.to(DEV)
    model = model.train() if train else model.eval()
    inputs = [t.to(DEV) if t is not None else None for t in diffusion_inputs(tag, cls, cfg, batch, frames, hw)]
    return model, inputs, cfg, betas, nsteps, g


@pytest.mark.parametrize("tag", _cases())
def test_goldens_with_the_fused_step(tag):
    """noise="host" draws what the restated scheduler draws (the start noise from torch's global generator, the variance
    noise from a CPU generator seeded with 7) and feeds it to the fused kernel: the reference trajectories under the bound
    of tests/test_diffusion_gpu.py"""
    from dlwp_benchmark_amd.schedulers import RefinerScheduler
    from oracle.make_golden import DIFFUSION_SEED
    from oracle.restate.ddpm import DDPMSchedulerRestated

    model, (constants, prescribed, prognostic), _, betas, nsteps, g = _model_and_inputs(tag)
    want = torch.from_numpy(g["y"])
    errs = {}
    for name, sched in (("fused", RefinerScheduler(trained_betas=betas, noise="host", seed=7)),
                        ("restated", DDPMSchedulerRestated(betas, seed=7))):
        sched.set_timesteps(nsteps)
        torch.manual_seed(DIFFUSION_SEED)
        got = model(constants=constants, prescribed=prescribed, prognostic=prognostic, noise_scheduler=sched)
        torch.cuda.synchronize()
        assert got.shape == want.shape
        errs[name] = per_step_rel_l2(got, want)
    print(f"{tag}: per-step rel L2 against the golden: fused step {['%.2e' % e for e in errs['fused']]}, restated scheduler "
          f"{['%.2e' % e for e in errs['restated']]}")
    assert max(errs["fused"]) <= 1e-5, f"{tag}: per-step rel L2 {['%.2e' % e for e in errs['fused']]}"


def test_device_noise_mode():
    """noise="device" on the smallest case: reproducible after reseed(), another seed differs, torch's generator is left alone,
    and the output is bitwise the loop below -- single_forward, ops.philox_normal at the documented offsets (every draw takes
    its element count rounded up to 4: the start noise of a forecast step, then one draw per refinement step with t > 0) and
    the explicit-noise step"""
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd.schedulers import RefinerScheduler

    model, (constants, prescribed, prognostic), cfg, betas, nsteps, _ = _model_and_inputs(SMALL)
    assert constants is None and prescribed is None and cfg["context_size"] == 1
    sched = RefinerScheduler(trained_betas=betas, noise="device", seed=3)
    sched.set_timesteps(nsteps)
    state = torch.get_rng_state()
    run = lambda: model(prognostic=prognostic, noise_scheduler=sched)
    a = run()
    used = sched.offset
    sched.reseed()
    b = run()
    assert torch.equal(a, b) and sched.offset == used
    assert torch.equal(torch.get_rng_state(), state), "the forward drew from torch's host generator"
    sched.reseed(4)
    assert not torch.equal(run(), a)
    # the loop, written out (context_size 1: the input of a forecast step is the frame before it)
    seed, offset = 3, 0
    frames = prognostic.shape[1]
    shape = tuple(prognostic[:, 1:2].shape)
    n = prognostic[:, 1:2].numel()
    draw = (n + 3) // 4 * 4
    outs = []
    with torch.no_grad():
        last = prognostic[:, 0:1]
        for _ in range(1, frames):
            y = ops.philox_normal(shape, seed, offset, device=DEV)
            offset += draw
            for k in sched.timesteps.tolist():
                time = torch.full((last.shape[0],), k, dtype=torch.long, device=DEV)
                pred = model.single_forward(None, None, last, y, time=time).unsqueeze(1)
                coef = sched.coefficients(k)
                if k > 0:
                    z = ops.philox_normal(shape, seed, offset, device=DEV)
                    offset += draw
                    y = ops.ddpm_step(y, pred, coef, noise=z)
                else:
                    y = ops.ddpm_step(y, pred, coef)
            outs.append(last[:, -1] + y.flatten(1, 2))
            last = outs[-1].unsqueeze(1)
    want = torch.stack(outs, dim=1)
    assert offset == used
    assert torch.equal(a, want)
    assert bool(torch.isfinite(a).all())


def test_training_step_from_training_pair():
    """training_pair's outputs through single_forward and F.mse_loss (scripts/train.py:228-271) against the torch composition
    of the same lines fed the same explicit noise: the loss within 1e-5 relative (the two differ by fp32 roundings of the
    network's input and of the target), and backward() runs.  With the scheduler's own device noise the pair is the explicit
    one of ops.philox_normal."""
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd.schedulers import RefinerScheduler

    model, (_, _, prognostic), cfg, betas, _, _ = _model_and_inputs(SMALL, train=True)
    ctx = cfg["context_size"]
    prog, target = prognostic[:, 0:ctx], prognostic[:, ctx:ctx + 1]
    sched = RefinerScheduler(trained_betas=betas, noise="device", seed=5)
    noise = ops.philox_normal(tuple(target.shape), 5, 0, device=DEV)
    k = 1
    y_noised, v_target, time, k_out = sched.training_pair(prog, target, ctx, k=k)
    assert k_out == k and sched.offset == (target.numel() + 3) // 4 * 4
    y_explicit, v_explicit, _, _ = sched.training_pair(prog, target, ctx, k=k, noise=noise)
    assert torch.equal(y_noised, y_explicit) and torch.equal(v_target, v_explicit)

    def loss_of(y, want, time):
        model.zero_grad(set_to_none=True)
        out = model.single_forward(None, None, prog, y, time=time).unsqueeze(1)
        assert out.shape == want.shape
        loss = F.mse_loss(out, want)
        loss.backward()
        torch.cuda.synchronize()
        grads = [p.grad for p in model.parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
        return float(loss.detach())

    got = loss_of(y_noised, v_target, time)
    # the reference's lines in torch
    target_res = target - prog[:, ctx - 1:ctx]
    noise_factor = sched.alphas_cumprod.to(DEV)[k].view(-1, 1, 1, 1, 1)
    signal_factor = 1 - noise_factor
    y_ref = (noise_factor ** 0.5) * target_res + ((1 - noise_factor) ** 0.5) * noise          # DDPMScheduler.add_noise
    want_ref = (noise_factor ** 0.5) * noise - (signal_factor ** 0.5) * target_res
    ref = loss_of(y_ref, want_ref, torch.full((prog.shape[0],), k, device=DEV))
    print(f"training step loss: training_pair {got:.8e}, torch composition {ref:.8e}, relative difference "
          f"{abs(got - ref) / abs(ref):.2e}")
    assert abs(got - ref) <= 1e-5 * abs(ref)
    # k not given: drawn on the host
    sched.reseed()
    _, _, time2, k2 = sched.training_pair(prog, target, ctx)
    assert 0 <= k2 < sched.num_train_timesteps - 1 and time2.tolist() == [k2] * prog.shape[0]
