"""SFNO2DModule -- drop-in for reference models/fno/fno.py:149-259 on MI355X: same class name, constructor kwargs and
defaults (fno.py:155-177), `_prepare_inputs` and rollout (fno.py:202-259), forward(constants, prescribed, prognostic).

The reference builds `torch_harmonics.examples.sfno.SphericalFourierNeuralOperatorNet` (fno.py:183-200); that third-party
module is not part of the reference tree and not installable here, so `self.sfno` below is a RESTATEMENT of it from recollection
of its 0.6-era source -- PARITY UNPINNED at this boundary, exactly as `models/fno.py` stands to
neuralop.  Module names follow the library as far as recalled (`sfno.encoder`, `sfno.pos_embed`,
`sfno.blocks.{i}.filter.filter.weight`, `.inner_skip`, `.mlp.fwd.{0,2}`, `sfno.decoder`); checkpoint compatibility with the
library is NOT claimed.  What IS pinned: the spherical harmonic transforms and the Driscoll-Healy mix, by float64 restatements
and by mathematics (exact round trips, orthonormality, closed-form harmonics; tests/test_sphere_cpu.py, tests/test_sht_gpu.py),
and the network below against its float64 restatement (tests/sht_ref.py, tests/test_sfno_gpu.py).

One step: every 1x1 convolution runs through ops.conv2d with its fused bias / activation / residual, the transforms and the
channel mix through csrc/sht.hip -- the inference step holds no torch convolution, FFT or einsum.  The rollout is device
resident (rollout.rollout_into; no per-step `.cpu()`, fno.py:257, and no O(T^2) `stack`, :246) and does not reproduce the
reference's crash on the second step (`.to()` on a list, fno.py:244-247).

Left out (NotImplementedError names the key): operator_type other than "driscoll-healy", factorization, spectral_transform
other than "sht", normalization layers, grid "lobatto", a scale_factor that leaves an odd inner width.
"""
import torch
from torch import nn

from .. import lib as _lib
from .. import ops
from ._base import StepBackbone

_ACTIVATIONS = ("gelu", "relu")


class _Transform:
    """one grid of the network: (nlat, nlon, grid) and the truncation every transform of the network shares"""

    def __init__(self, nlat: int, nlon: int, grid: str, modes: int):
        self.nlat, self.nlon, self.grid, self.modes = int(nlat), int(nlon), grid, int(modes)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.sht(x, self.grid, self.modes, self.modes)

    def inverse(self, c: torch.Tensor) -> torch.Tensor:
        return ops.isht(c, self.grid, self.nlat, self.nlon)

    def same_grid(self, other: "_Transform") -> bool:
        return (self.nlat, self.nlon) == (other.nlat, other.nlon)


class _SpectralConv(nn.Module):
    """`filter.filter`: the Driscoll-Healy weight, one complex [in, out] matrix per degree, stored as (re, im) pairs"""

    def __init__(self, channels: int, modes: int):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(channels, channels, modes, 2))


class _Filter(nn.Module):
    def __init__(self, channels: int, modes: int):
        super().__init__()
        self.filter = _SpectralConv(channels, modes)


class _BlockMlp(nn.Module):
    """1x1 convolutions E -> 2E -> E; `fwd.1` is the activation (no parameters)"""

    def __init__(self, channels: int):
        super().__init__()
        self.fwd = nn.ModuleDict({"0": nn.Conv2d(channels, 2 * channels, 1), "2": nn.Conv2d(2 * channels, channels, 1)})


class _Block(nn.Module):
    def __init__(self, channels: int, modes: int, use_mlp: bool):
        super().__init__()
        self.filter = _Filter(channels, modes)
        self.inner_skip = nn.Conv2d(channels, channels, 1)
        if use_mlp:
            self.mlp = _BlockMlp(channels)
        self.use_mlp = bool(use_mlp)


class _SFNO(nn.Module):
    def __init__(self, in_chans, out_chans, img_size, grid, num_layers, scale_factor, embed_dim, hard_thresholding_fraction,
                 big_skip, pos_embed, use_mlp, activation_function):
        super().__init__()
        H, W = int(img_size[0]), int(img_size[1])
        h, w = H // int(scale_factor), W // int(scale_factor)
        if w % 2 or W % 2:
            raise NotImplementedError(f"scale_factor={scale_factor} leaves an odd width ({W} -> {w}): the transforms take an even "
                                      "number of longitudes")
        modes = min(int(h * hard_thresholding_fraction), int((w // 2) * hard_thresholding_fraction))
        if modes < 1:
            raise _lib.DlwpError(f"hard_thresholding_fraction={hard_thresholding_fraction} keeps no mode of a {h} x {w} grid")
        self.img_size, self.inner_size, self.modes = (H, W), (h, w), modes
        self.big_skip, self.act = bool(big_skip), ops.ACTS[activation_function]
        self.trans_down = _Transform(H, W, grid, modes)
        self.itrans_up = _Transform(H, W, grid, modes)
        self.trans = _Transform(h, w, "legendre-gauss", modes)
        self.itrans = self.trans
        self.encoder = nn.ModuleDict({"0": nn.Conv2d(in_chans, embed_dim, 1), "2": nn.Conv2d(embed_dim, embed_dim, 1, bias=False)})
        if pos_embed:
            self.pos_embed = nn.Parameter(torch.zeros(1, embed_dim, H, W))
        else:
            self.pos_embed = None
        self.blocks = nn.ModuleList([_Block(embed_dim, modes, use_mlp) for _ in range(int(num_layers))])
        self.decoder = nn.ModuleDict({"0": nn.Conv2d(embed_dim + (in_chans if big_skip else 0), embed_dim, 1),
                                      "2": nn.Conv2d(embed_dim, out_chans, 1, bias=False)})
        # ops.CONV_FORMS of the 1x1 convolutions (HipBackbone.set_aux_conv_form).  Not the family default "direct": these are
        # E x E and E x 2E channel GEMMs, which the one-thread-per-output kernel runs 20x slower than the fp32-grade matrix-pipe
        # form at the config's width (53.2 against 2.61 ms per step, profiles/sht_mi355x.json)
        self.aux_conv_form = "bf16x6"

    def _conv(self, m: nn.Conv2d, x, act=0, resid=None):
        return ops.conv2d(x, m.weight, m.bias, act=act, resid=resid, form=self.aux_conv_form)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        grad = torch.is_grad_enabled()       # autograd may record: nothing in place, the library's cat
        x = x.contiguous()
        if tuple(x.shape[2:]) != self.img_size:
            raise _lib.DlwpError(f"input grid {tuple(x.shape[2:])} does not match the model's {self.img_size}")
        y = self._conv(self.encoder["2"], self._conv(self.encoder["0"], x, act=self.act))
        if self.pos_embed is not None:
            y = y + self.pos_embed if grad else y.add_(self.pos_embed)
        last = len(self.blocks) - 1
        for i, blk in enumerate(self.blocks):
            fwd = self.trans_down if i == 0 else self.trans
            inv = self.itrans_up if i == last else self.itrans
            c = fwd.forward(y)
            r = y if fwd.same_grid(inv) else inv.inverse(c)       # the residual lives on the grid the block writes
            wt = blk.filter.filter.weight
            f = inv.inverse(ops.sph_mix(c, torch.view_as_complex(wt), owner=wt))      # (the pack is cached on the Parameter)
            z = self._conv(blk.inner_skip, r, act=self.act, resid=f)                 # act(filter + inner_skip(r))
            if blk.use_mlp:
                y = self._conv(blk.mlp.fwd["2"], self._conv(blk.mlp.fwd["0"], z, act=self.act), resid=r)
            else:
                y = z + r if grad else z.add_(r)
        if self.big_skip:
            y = torch.cat([y, x], dim=1) if grad else ops.concat_channels([y, x])
        return self._conv(self.decoder["2"], self._conv(self.decoder["0"], y, act=self.act))


class SFNO2DModule(StepBackbone):
    def __init__(self, constant_channels: int = 4, prescribed_channels: int = 1, prognostic_channels: int = 8,
                 spectral_transform='sht', grid="legendre-gauss", num_layers=4, scale_factor=3, embed_dim=256,
                 operator_type='driscoll-healy', context_size: int = 1, height: int = 32, width: int = 64,
                 hard_thresholding_fraction: float = 1.0, factorization: str = None, rank: float = 1.0, big_skip: bool = False,
                 pos_embed: bool = False, use_mlp: bool = False, normalization_layer: str = None,
                 activation_function: str = "gelu", **kwargs):
        super().__init__()
        if spectral_transform != "sht":
            raise NotImplementedError(f"spectral_transform={spectral_transform!r}: only 'sht' is on the HIP path")
        if operator_type != "driscoll-healy":
            raise NotImplementedError(f"operator_type={operator_type!r}: only 'driscoll-healy' is on the HIP path")
        if factorization is not None:
            raise NotImplementedError(f"factorization={factorization!r}: only dense spectral weights (None) are on the HIP path")
        if normalization_layer not in (None, "none"):
            raise NotImplementedError(f"normalization_layer={normalization_layer!r}: only 'none' / None is on the HIP path")
        if grid == "lobatto":
            raise NotImplementedError("grid='lobatto' is not supported (no shipped config uses it)")
        if grid not in ("legendre-gauss", "equiangular"):
            raise _lib.DlwpError(f"unknown grid {grid!r}")
        if activation_function not in _ACTIVATIONS:
            raise _lib.DlwpError(f"activation_function={activation_function!r} (one of {_ACTIVATIONS})")
        self.context_size = int(context_size)
        self.constant_channels, self.prescribed_channels = int(constant_channels), int(prescribed_channels)
        self.prognostic_channels = int(prognostic_channels)
        self.in_channels = self.constant_channels + (self.prescribed_channels + self.prognostic_channels) * self.context_size
        self.rank = rank          # accepted and unused without a factorization, as in the library
        self.sfno = _SFNO(in_chans=self.in_channels, out_chans=self.prognostic_channels, img_size=(height, width), grid=grid,
                          num_layers=num_layers, scale_factor=scale_factor, embed_dim=int(embed_dim),
                          hard_thresholding_fraction=float(hard_thresholding_fraction), big_skip=big_skip, pos_embed=pos_embed,
                          use_mlp=use_mlp, activation_function=activation_function)
        self._init_compute_precision(kwargs)

    def one_step(self, x_t: torch.Tensor) -> torch.Tensor:
        """`self.sfno(x_t)` of fno.py:256 (no residual): [B, in, H, W] -> [B, out, H, W], on the device"""
        _lib.require_cuda_tensor(x_t, "x_t")
        if x_t.dim() != 4 or x_t.shape[1] != self.in_channels:
            raise _lib.DlwpError(f"x_t {tuple(x_t.shape)}: the model expects [B, {self.in_channels}, H, W]")
        return self.sfno(x_t)
