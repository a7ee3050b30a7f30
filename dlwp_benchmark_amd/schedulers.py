"""The noise scheduler of the PDE-Refiner backbones (DiffModernUNet, DiffMUNetHPX) on the HIP kernels of csrc/refiner.hip.

The reference scripts build `diffusers.DDPMScheduler` for `forward(..., noise_scheduler=...)` (scripts/train.py:76-83,
scripts/evaluate.py:194-202).  `RefinerScheduler` takes the same constructor arguments and offers the part of that interface
the reference uses, so the one-line replacement in those scripts is

    noise_scheduler = RefinerScheduler(num_train_timesteps=..., trained_betas=betas, prediction_type="v_prediction",
                                       clip_sample=False)
"""
import math
from types import SimpleNamespace

import torch

from . import lib as _lib
from . import ops as _ops


def _ceil4(n: int) -> int:
    return (int(n) + 3) // 4 * 4


class RefinerScheduler:
    """DDPM ancestral sampling as the reference configures it: `trained_betas`, prediction_type "v_prediction",
    clip_sample False, and diffusers' defaults otherwise (variance_type "fixed_small" clamped at 1e-20, timestep_spacing
    "leading", steps_offset 0).  Anything else raises DlwpError.

    `diffusers` is a third-party dependency that is absent from the reference tree, and the reference pins no version of it:
    this scheduler is PARITY UNPINNED.  It states the published DDPM ancestral step (Ho et al. 2020, eq. 6-7, with the
    v-parameterisation of Salimans & Ho 2022); the networks it drives are pinned to the reference, the scheduler is pinned
    to that statement only.

    Interface as diffusers': betas, alphas, alphas_cumprod (float32 CPU tensors), num_train_timesteps, num_inference_steps,
    timesteps, set_timesteps(n), step(model_output, timestep, sample, generator=None, noise=None).prev_sample,
    add_noise(original, noise, timesteps).  Beyond it: coefficients(t), randn(shape, device), training_pair(...), seed,
    offset, reseed(seed=None), and for ensembles set_members(count, first=0), members, first_member (rollout.ensemble_chunks
    and rollout.ensemble_forecast drive them).

    Noise.  noise="device" (the default): every draw is a range of ONE counter-based stream (ops.philox_normal: Philox4x32-10
    and Box-Muller, a pure function of (seed, element index)).  The scheduler keeps `offset`, the index of the next unused
    element, and advances it by the draw's element count rounded up to a multiple of 4 -- in randn(), in step() at t > 0 and
    in training_pair().  The start noise and the variance noise are generated inside the kernels that consume them; torch's
    host generator is never touched and nothing is uploaded.  noise="host": randn() is torch.randn(shape).to(device) from
    the global generator (what the reference's diffusion_forward does) and the step noise comes from the scheduler's own CPU
    generator seeded with `seed`, drawn only at t > 0; both are then fed to the same fused kernels as explicit noise.  This
    mode exists so that the fused step can be compared with trajectories recorded with host noise.
    """

    def __init__(self, num_train_timesteps=None, trained_betas=None, prediction_type="v_prediction", clip_sample=False, *,
                 noise="device", seed=0):
        if trained_betas is None:
            raise _lib.DlwpError("RefinerScheduler needs trained_betas: the reference configures no beta schedule by name")
        if prediction_type != "v_prediction":
            raise _lib.DlwpError(f"RefinerScheduler: prediction_type {prediction_type!r} is not supported (v_prediction only)")
        if clip_sample:
            raise _lib.DlwpError("RefinerScheduler: clip_sample=True is not supported")
        if noise not in ("device", "host"):
            raise _lib.DlwpError(f"RefinerScheduler: noise must be 'device' or 'host' (got {noise!r})")
        self.betas = torch.tensor([float(b) for b in trained_betas], dtype=torch.float32)
        if self.betas.ndim != 1 or self.betas.numel() == 0:
            raise _lib.DlwpError("RefinerScheduler: trained_betas must be a non-empty list")
        if num_train_timesteps is not None and int(num_train_timesteps) != self.betas.numel():
            raise _lib.DlwpError(f"RefinerScheduler: num_train_timesteps {num_train_timesteps} against {self.betas.numel()} betas")
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self._abar = [float(a) for a in self.alphas_cumprod.tolist()]          # the fp32 values, as Python floats
        self.num_train_timesteps = int(self.betas.numel())
        self.num_inference_steps = None
        self.timesteps = torch.arange(self.num_train_timesteps - 1, -1, -1)
        self.prediction_type, self.clip_sample, self.noise = prediction_type, False, noise
        self.init_noise_sigma = 1.0
        self.seed = 0
        self.offset = 0
        self._members, self._first_member = 1, 0
        self.reseed(seed)

    @classmethod
    def pde_refiner(cls, num_refinement_steps: int, min_noise_std: float, **kw):
        """the beta list of scripts/train.py:76 / evaluate.py:188: min_noise_std ** (k / N) for k = N .. 0"""
        n = int(num_refinement_steps)
        betas = [min_noise_std ** (k / n) for k in reversed(range(n + 1))]
        return cls(num_train_timesteps=n + 1, trained_betas=betas, **kw)

    # ---- noise state --------------------------------------------------------------------------------------------------
    def reseed(self, seed=None):
        """back to the start of the stream (of `seed` when given): offset 0 and fresh host generators"""
        if seed is not None:
            self.seed = int(seed)
        self.offset = 0
        self._gen = torch.Generator().manual_seed(self.seed)          # step noise of noise="host"
        self._k_gen = torch.Generator().manual_seed(self.seed)        # the refinement index of training_pair
        return self

    def _take(self, n: int) -> int:
        """the offset of a draw of n elements; the stream advances past it"""
        at = self.offset
        self.offset = at + _ceil4(n)
        return at

    # ---- ensemble members ----------------------------------------------------------------------------------------------
    @property
    def members(self) -> int:
        return self._members

    @property
    def first_member(self) -> int:
        return self._first_member

    def set_members(self, count: int, first: int = 0):
        """Member mode, for ensembles of one initial condition: with count > 1 or first > 0, randn() and step() treat dim 0 of
        their tensors as member-major [count * B, ...] and member m of them draws from the stream normal(seed, first + m, .)
        (ops.philox_normal_members); the offset advances by ONE member's element count rounded up to 4, which is what a
        single-member run of the per-member shape uses.  So member m's noise is a function of (seed, first + m, the per-member
        shape, the call order) only: a large ensemble run in groups is bitwise the same ensemble.  (1, 0), the default, is the
        scheduler without members, call for call.  training_pair is not concerned."""
        count, first = int(count), int(first)
        if count < 1 or first < 0 or first + count > 1 << 31:
            raise _lib.DlwpError(f"set_members: count = {count}, first = {first} must name members within [0, 2^31)")
        if self.noise == "host" and (count, first) != (1, 0):
            raise _lib.DlwpError("set_members: noise='host' draws from torch's generators, which have no member streams")
        self._members, self._first_member = count, first
        return self

    def _per_member(self, shape, what: str) -> int:
        """elements of one member of a member-major tensor of `shape`"""
        if len(shape) < 1 or shape[0] % self._members:
            raise _lib.DlwpError(f"{what}: dim 0 of {tuple(shape)} is not divisible by the {self._members} members")
        return math.prod(shape) // self._members

    def randn(self, shape, device):
        """the start noise of a forecast step (modern_unet.py:184)"""
        shape = tuple(int(s) for s in shape)
        if self.noise == "host":
            return torch.randn(shape).to(device=device)
        if (self._members, self._first_member) != (1, 0):
            at = self._take(self._per_member(shape, "randn"))
            return _ops.philox_normal_members(shape, self.seed, self._members, self._first_member, at, device=device)
        return _ops.philox_normal(shape, self.seed, self._take(math.prod(shape)), device=device)

    # ---- sampling -----------------------------------------------------------------------------------------------------
    def set_timesteps(self, num_inference_steps: int, device=None):
        n = int(num_inference_steps)
        if n > self.num_train_timesteps:
            raise ValueError(f"{n} inference steps against {self.num_train_timesteps} training steps")
        if n <= 0:
            raise ValueError("num_inference_steps must be positive")
        self.num_inference_steps = n
        ratio = self.num_train_timesteps // n
        self.timesteps = (torch.arange(0, n) * ratio).round().flip(0).long()          # "leading" spacing, steps_offset 0

    def previous_timestep(self, t: int) -> int:
        return int(t) - self.num_train_timesteps // (self.num_inference_steps or self.num_train_timesteps)

    def coefficients(self, timestep):
        """(sa, sb, c0, c1, sigma) of the step at `timestep` as Python floats (float64 algebra on the fp32 alphas_cumprod):
          x0 = sa sample - sb model_output;  prev = c0 x0 + c1 sample + sigma z
        sa = sqrt(abar_t), sb = sqrt(1 - abar_t), c0 = sqrt(abar_prev) beta_t' / (1 - abar_t), c1 = sqrt(alpha_t')
        (1 - abar_prev) / (1 - abar_t) with alpha_t' = abar_t / abar_prev, beta_t' = 1 - alpha_t'; sigma^2 =
        max((1 - abar_prev) / (1 - abar_t) beta_t', 1e-20) for t > 0 and sigma = 0 at t = 0."""
        t = int(timestep)
        if not 0 <= t < self.num_train_timesteps:
            raise _lib.DlwpError(f"timestep {t} outside [0, {self.num_train_timesteps})")
        prev_t = self.previous_timestep(t)
        a_t = self._abar[t]
        a_prev = self._abar[prev_t] if prev_t >= 0 else 1.0
        b_t, b_prev = 1.0 - a_t, 1.0 - a_prev
        cur_a = a_t / a_prev
        cur_b = 1.0 - cur_a
        sa, sb = a_t ** 0.5, b_t ** 0.5
        c0 = a_prev ** 0.5 * cur_b / b_t
        c1 = cur_a ** 0.5 * b_prev / b_t
        sigma = max(b_prev / b_t * cur_b, 1e-20) ** 0.5 if t > 0 else 0.0
        return sa, sb, c0, c1, sigma

    def step(self, model_output, timestep, sample, generator=None, noise=None):
        """one ancestral step on ops.ddpm_step; `.prev_sample` is a new tensor.  `noise` (or a torch `generator` to draw it
        from) overrides the scheduler's own noise for this step; neither advances the stream."""
        t = int(timestep)
        coef = self.coefficients(t)
        offset = 0
        by_member = (self._members, self._first_member) != (1, 0)
        if t > 0 and noise is None:
            if generator is not None:
                noise = torch.randn(model_output.shape, generator=generator, device=generator.device).to(model_output.device)
            elif self.noise == "host":
                noise = torch.randn(model_output.shape, generator=self._gen).to(model_output.device)
            elif by_member:
                offset = self._take(self._per_member(tuple(model_output.shape), "step"))
            else:
                offset = self._take(model_output.numel())
        if t == 0:
            noise = None
        if by_member:
            prev = _ops.ddpm_step(sample, model_output, coef, noise=noise, seed=self.seed, offset=offset, members=self._members,
                                  first_member=self._first_member)
        else:
            prev = _ops.ddpm_step(sample, model_output, coef, noise=noise, seed=self.seed, offset=offset)
        return SimpleNamespace(prev_sample=prev.view(sample.shape))

    # ---- training -----------------------------------------------------------------------------------------------------
    def _sqrt_pair(self, k: int):
        a = self._abar[k]
        return a ** 0.5, (1.0 - a) ** 0.5

    def add_noise(self, original_samples, noise, timesteps):
        """sqrt(abar_t) original + sqrt(1 - abar_t) noise with the two factors rounded to fp32 from float64, the values
        training_pair's kernel uses.  `timesteps`: an int, or an integer tensor with one entry or one entry per sample."""
        if isinstance(timesteps, torch.Tensor) and timesteps.numel() > 1:
            ts = timesteps.reshape(-1).tolist()
        else:
            ts = [int(timesteps)]
        if any(not 0 <= int(t) < self.num_train_timesteps for t in ts):
            raise _lib.DlwpError(f"add_noise: timesteps {ts} outside [0, {self.num_train_timesteps})")
        pairs = [self._sqrt_pair(int(t)) for t in ts]
        view = (-1,) + (1,) * (original_samples.dim() - 1)
        sa = torch.tensor([p[0] for p in pairs], dtype=torch.float32).to(original_samples.device).view(view)
        sb = torch.tensor([p[1] for p in pairs], dtype=torch.float32).to(original_samples.device).view(view)
        return sa * original_samples + sb * noise

    def training_pair(self, prognostic, target, context_size, k=None, noise=None):
        """The inputs of one PDE-Refiner training step (scripts/train.py:228-255) on ops.refiner_pair:
          (y_noised, v_target, time_tensor, k)
        with res = target - prognostic[:, context_size - 1 : context_size], y_noised = add_noise(res, eps, k), v_target =
        sqrt(abar_k) eps - sqrt(1 - abar_k) res and time_tensor = full((batch,), k); HEALPix inputs come back with the faces
        folded into the batch.  `k` not given: drawn from [0, num_train_timesteps - 1) with the scheduler's own CPU
        generator -- no device randint, no .item().  eps: `noise` when given, else the scheduler's."""
        if k is None:
            k = int(torch.randint(0, max(self.num_train_timesteps - 1, 1), (1,), generator=self._k_gen))
        k = int(k)
        if not 0 <= k < self.num_train_timesteps:
            raise _lib.DlwpError(f"training_pair: k = {k} outside [0, {self.num_train_timesteps})")
        _lib.require_cuda_tensor(prognostic, "prognostic")
        _lib.require_cuda_tensor(target, "target")
        sa, sb = self._sqrt_pair(k)
        offset = 0
        if noise is None:
            faces = target.shape[3] if target.dim() == 6 else 1
            if self.noise == "host":
                shape = (target.shape[0] * faces, 1, target.shape[2]) + tuple(target.shape[-2:])
                noise = torch.randn(shape, generator=self._gen).to(target.device)
            else:
                offset = self._take(target.numel())
        y_noised, v_target = _ops.refiner_pair(prognostic, target, context_size, sa, sb, noise=noise, seed=self.seed,
                                               offset=offset)
        time_tensor = torch.full((y_noised.shape[0],), k, dtype=torch.long, device=y_noised.device)
        return y_noised, v_target, time_tensor, k
