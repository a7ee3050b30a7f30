"""Synthetic inputs of the shapes the reference dataset hands to model.forward.

No dataset is available offline (reference dlwpbench/README.md:10-49), so benchmarks and
parity tests use the seeded generators of SURVEY.md section 8d:

* Navier-Stokes 64x64 (BASELINE configs C1/C2): band-limited periodic Gaussian random field,
  spectrum ~ (k^2 + tau^2)^-alpha, tau=7, alpha=2.5, standardised; no constants / prescribed.
* WeatherBench-like (C3-C5): constants = {orography-like, land mask, lat2d, lon2d},
  prescribed = analytic insolation, prognostic = smooth unit-variance fields; the tuple layout
  follows WeatherBenchDataset.__getitem__ (reference data/datasets/datasets.py:330-416):
  constants [B,1,Cc,H,W], prescribed [B,T,Cp,H,W], prognostic [B,T,Cg,H,W], fp32.
"""
import math

import numpy as np
import torch


def _grf(rng: np.random.Generator, n: int, h: int, w: int, tau: float = 7.0, alpha: float = 2.5) -> np.ndarray:
    ky = np.fft.fftfreq(h, d=1.0 / h)[:, None]
    kx = np.fft.rfftfreq(w, d=1.0 / w)[None, :]
    amp = (kx * kx + ky * ky + tau * tau) ** (-alpha / 2.0)
    amp[0, 0] = 0.0
    coef = (rng.standard_normal((n, h, w // 2 + 1)) + 1j * rng.standard_normal((n, h, w // 2 + 1))) * amp
    f = np.fft.irfft2(coef, s=(h, w))
    f -= f.mean(axis=(-2, -1), keepdims=True)
    f /= f.std(axis=(-2, -1), keepdims=True) + 1e-12
    return f.astype(np.float32)


def navier_stokes(batch: int, steps: int, h: int = 64, w: int = 64, channels: int = 1, seed: int = 1234):
    """Returns (constants=None, prescribed=None, prognostic [B, T, C, H, W])."""
    rng = np.random.default_rng(seed)
    f = _grf(rng, batch * steps * channels, h, w).reshape(batch, steps, channels, h, w)
    return None, None, torch.from_numpy(f)


def weatherbench(batch: int, steps: int, h: int, w: int, prognostic_channels: int = 3,
                 constant_channels: int = 4, prescribed_channels: int = 1, seed: int = 1234):
    """Returns (constants [B,1,Cc,H,W], prescribed [B,T,Cp,H,W], prognostic [B,T,Cg,H,W])."""
    rng = np.random.default_rng(seed)
    lat = np.linspace(-90.0 + 90.0 / h, 90.0 - 90.0 / h, h, dtype=np.float64)
    lon = np.linspace(0.0, 360.0 - 360.0 / w, w, dtype=np.float64)
    lat2d, lon2d = np.meshgrid(lat, lon, indexing="ij")
    oro = _grf(rng, 1, h, w, tau=3.0, alpha=2.0)[0]
    lsm = (oro > 0.3).astype(np.float32)
    cons = [oro, lsm, (lat2d / 90.0).astype(np.float32), ((lon2d - 180.0) / 180.0).astype(np.float32)]
    while len(cons) < constant_channels:
        cons.append(_grf(rng, 1, h, w)[0])
    constants = np.stack(cons[:constant_channels], 0)[None, None].repeat(batch, 0) if constant_channels else None
    prescribed = None
    if prescribed_channels:
        t = np.arange(steps, dtype=np.float64)[:, None, None]
        omega = 2.0 * math.pi / 4.0  # one revolution per four 6-hourly steps
        sol = np.cos(np.deg2rad(lat2d))[None] * np.maximum(0.0, np.cos(np.deg2rad(lon2d)[None] - omega * t))
        sol = (sol - sol.mean()) / (sol.std() + 1e-12)
        prescribed = np.broadcast_to(sol[None, :, None].astype(np.float32),
                                     (batch, steps, prescribed_channels, h, w)).copy()
    prog = _grf(rng, batch * steps * prognostic_channels, h, w, tau=4.0, alpha=2.0)
    prog = prog.reshape(batch, steps, prognostic_channels, h, w)
    tt = torch.from_numpy
    return (tt(constants.astype(np.float32)) if constants is not None else None,
            tt(prescribed) if prescribed is not None else None, tt(prog))


class NavierStokes2D:
    """Fields with dynamics in them: trajectories of the 2-D incompressible Navier-Stokes equations in vorticity form on the
    unit torus -- the data law of Li et al. 2020 ("Fourier Neural Operator for Parametric PDEs": Gaussian random initial
    vorticity, fixed low-mode forcing, pseudo-spectral Crank-Nicolson steps) -- generated on the device: the initial condition by
    ops.gaussian_random_field, the integration by ops.navier_stokes_2d, one LDS-resident workgroup per trajectory
    (csrc/navier_stokes.hip).  A frame is `substeps` sub-steps of length `dt` after the one before it.
    Unlike navier_stokes() above, frame t + 1 follows from frame t.  Draws are counter-based: `draw` d of a batch of B uses the
    stream elements [d B n^2, (d + 1) B n^2) of `seed`, so equal (seed, batch, draw) give equal bits."""

    def __init__(self, n: int = 64, viscosity: float = 1e-3, dt: float = 1e-3, substeps: int = 250, forcing="li2020",
                 tau: float = 7.0, alpha: float = 2.5, seed: int = 0, device="cuda"):
        self.n, self.viscosity, self.dt, self.substeps = int(n), float(viscosity), float(dt), int(substeps)
        self.forcing, self.tau, self.alpha, self.seed = forcing, float(tau), float(alpha), int(seed)
        self.device = torch.device(device)

    def initial(self, batch: int, draw: int = 0) -> torch.Tensor:
        """[batch, n, n]: Gaussian random initial vorticity, draw `draw` of this batch size"""
        from . import ops
        per_draw = -(-int(batch) * self.n * self.n // 4) * 4
        return ops.gaussian_random_field((int(batch), self.n, self.n), self.seed, offset=int(draw) * per_draw, tau=self.tau,
                                         alpha=self.alpha, device=self.device)

    def solve(self, w0: torch.Tensor, frames: int) -> torch.Tensor:
        """[B, frames, n, n]: frame 0 is w0 (band-limited), frame t the vorticity t * substeps * dt later"""
        from . import ops
        return ops.navier_stokes_2d(w0, frames, self.substeps, self.dt, self.viscosity, forcing=self.forcing)

    def trajectories(self, batch: int, frames: int, draw: int = 0, scale=None):
        """(constants=None, prescribed=None, prognostic [B, frames, 1, n, n]) -- the tuple layout of navier_stokes(); with `scale`
        the field is divided by it"""
        prog = self.solve(self.initial(batch, draw), frames).unsqueeze(2)
        if scale is not None:
            prog = prog / scale
        return None, None, prog

    @staticmethod
    def windows(prognostic: torch.Tensor, sequence_length: int, context_size: int):
        """Every window of `sequence_length` consecutive frames of every trajectory of prognostic [B, F, C, n, n], as the
        training loop hands them on: (prognostic_in [B (F - L + 1), L, C, n, n] for model(prognostic=...), target = its frames
        from `context_size` on, what the loss compares the model's output with)"""
        b, f, c, h, w = prognostic.shape
        length, ctx = int(sequence_length), int(context_size)
        if not 1 <= ctx < length <= f:
            raise ValueError(f"windows: 1 <= context_size {ctx} < sequence_length {length} <= frames {f} is needed")
        win = prognostic.unfold(1, length, 1)                 # [B, F - L + 1, C, n, n, L]
        win = win.permute(0, 1, 5, 2, 3, 4).reshape(b * (f - length + 1), length, c, h, w).contiguous()
        return win, win[:, ctx:].contiguous()
