"""PDE-Refiner style diffusion backbones -- drop-in for reference
models/diffusion_models/modern_unet/modern_unet.py (`DiffModernUNet` :46-293, `DiffMUNetHPX` :295-327, registered in the
reference registry, models/__init__.py:15; configs/model/diffusion_modernunet*.yaml): a time-conditioned ModernUNet evaluated
`num_refinement_step` times per forecast step inside the autoregressive rollout ("the same rollout
wrapped in denoising iterations").  Same constructor kwargs, module tree / state-dict names and
`forward(constants, prescribed, prognostic, noise_scheduler, target)` signature.

The network runs on the hand-written kernels of the U-Net family: every `pad -> Conv2d(3x3)` is one dlwp_conv3x3_ex_f32 launch
(CylinderPad or HEALPixPadding inside the kernel, the activation in front of it applied while its input is staged, the shortcut
added in the epilogue), GroupNorm(+GELU) is dlwp_groupnorm_act_f32, the stride-2 / transposed / 1x1 convolutions are
dlwp_conv2d_f32 / dlwp_conv_transpose2d_f32.  What stays in torch: the sinusoidal time embedding and its two tiny Linears
([B, 64] operands), the AdaGN affine `h * (1 + scale) + shift` (one elementwise pass) and the noise scheduler itself, which the
caller supplies (the reference scripts pass diffusers' DDPMScheduler, scripts/evaluate.py:186-202; any object with `.timesteps`
and `.step(pred, k, sample).prev_sample` works).  The reference draws the start noise with `th.randn(shape)` on the host and
moves it to the device (:186); so does this mirror, so a seeded run sees the same noise.  A scheduler that offers
`randn(shape, device)` -- schedulers.RefinerScheduler, whose step and noise run on csrc/refiner.hip -- supplies the start noise
itself; every other scheduler object takes the host line.

`attention=True` (modern_unet.py:54, the PDE-Refiner paper's attention experiment; both reference configs run without it) adds
an `AttentionBlock` after the residual block of every ENCODER level: global multi-head self-attention over the whole feature map
(per HEALPix face, faces being folded into the batch), its core one dlwp_global_attn_f32 launch pair that never forms the N x N
score tensor, its two Linears on dlwp_linear_f32.  `DiffModernUNet` / `DiffMUNetHPX` pass the flag to the encoder only, as the
reference does (:94-121): the middle block and the decoder keep their Identity slots.  `MiddleBlock` and `ModernUNetDecoder`
constructed directly with attention=True build blocks too.  The encoder and decoder reassign `self.attn` per level, so
`attn` is the LAST level's block under a second name, registered before `layers` -- the state dict lists it twice
(`encoder.attn.*`, `encoder.layers.{L-1}.{i}.*`), named_parameters() once."""
import math
from typing import Optional

import torch
from torch import nn

from .. import lib as _lib
from .. import ops
from .. import training as _T
from ._base import HipBackbone, fold_faces
from .unet import CylinderPad, HEALPixPadding, _resolve_activation


def fourier_embedding(timesteps: torch.Tensor, dim: int, max_period: int = 10000) -> torch.Tensor:
    """modern_unet.py:10-31 (sinusoidal timestep embedding, cos | sin halves)."""
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32) / half).to(timesteps.device)
    args = timesteps[:, None].float() * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1)
    return emb


def _zero_module(m: nn.Module) -> nn.Module:
    for p in m.parameters():
        p.detach().zero_()
    return m


class AttentionBlock(nn.Module):
    """modern_unet.py:520-585: multi-head self-attention over all H W tokens of a [B, C, H, W] map, `projection` Linear
    C -> heads * 3 d_k (per head q | k | v contiguous), softmax over the QUERY axis (dim=1 of attn[b, i, j, h]: every key's
    weights over all queries sum to one), `output` Linear heads d_k -> C, skip `+ x`.  d_k defaults to C, not C / heads.
    Forward: ops.attention_block (HIP).  With gradients wanted: tokens by a torch transpose, the attention through
    training.global_attention (HIP forward and backward, no N x N tensor), the two Linears as the modules themselves: the
    HIP GEMM's weight gradient reduces over all Bt N tokens, which it does slower than torch here and refuses at nside 64
    with batch 32 (its 32-bit tile offsets), DESIGN.md section 12.  _torch_forward is the same block composed from torch
    operators, kept as the cross-check."""

    def __init__(self, in_channels: int, n_heads: int = 4, d_k: Optional[int] = None):
        super().__init__()
        self.in_channels = in_channels
        self.n_heads = n_heads
        self.d_k = d_k if d_k is not None else in_channels
        self.projection = nn.Linear(in_channels, n_heads * self.d_k * 3)
        self.output = nn.Linear(n_heads * self.d_k, in_channels)
        self.scale = self.d_k ** -0.5

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if _T.wants_grad(x, *self.parameters()):
            # a CPU tensor keeps the torch composition it always had with gradients; on the device the HIP kernels run
            return self._train_forward(x) if x.is_cuda else self._torch_forward(x)
        return ops.attention_block(x, self.projection, self.output, self.n_heads, self.d_k, self.scale)

    def _train_forward(self, x: torch.Tensor) -> torch.Tensor:
        b, c, h, w = x.shape
        if c != self.in_channels:
            raise _lib.DlwpError(f"AttentionBlock: x has {c} channels, the block {self.in_channels}")
        t = x.reshape(b, c, h * w).transpose(1, 2)
        qkv = self.projection(t)
        res = _T.global_attention(qkv, self.n_heads, self.d_k, self.scale)
        return (self.output(res) + t).transpose(1, 2).reshape(b, c, h, w)

    def _torch_forward(self, x: torch.Tensor) -> torch.Tensor:
        b, c, h, w = x.shape
        t = x.reshape(b, c, h * w).transpose(1, 2)
        q, k, v = self.projection(t).view(b, h * w, self.n_heads, 3, self.d_k).unbind(3)
        p = torch.softmax(torch.einsum("bihd,bjhd->bhij", q, k) * self.scale, dim=2)     # over the queries i
        res = torch.einsum("bhij,bjhd->bihd", p, v).reshape(b, h * w, self.n_heads * self.d_k)
        return (self.output(res) + t).transpose(1, 2).reshape(b, c, h, w)


class ResidualBlock(nn.Module):
    """modern_unet.py:560-650: conditioned wide residual block.  `use_scale_shift_norm` (AdaGN): the embedding gives a
    per-(sample, channel) scale and shift applied between the two convolutions; otherwise it is added as a bias."""

    def __init__(self, in_channels: int, out_channels: int, cond_channels: int, activation=None, norm: bool = False,
                 n_groups: int = 4, use_scale_shift_norm: bool = True, kernel_size=3, padding=1, mesh=None):
        super().__init__()
        if kernel_size != 3:
            raise NotImplementedError("only 3x3 residual blocks have a fused kernel")
        activation = _resolve_activation(activation) if activation is not None else nn.GELU()
        if not isinstance(activation, nn.GELU):
            raise NotImplementedError("ResidualBlock: only GELU (the reference default) is wired to the fused kernels")
        self.activation = activation
        self.use_scale_shift_norm = use_scale_shift_norm
        self.mesh = mesh
        self.conv_form = "direct"       # ops.CONV_FORMS, set through HipBackbone.set_conv_form / set_compute_precision
        self.aux_conv_form = "direct"   # ops.CONV_FORMS of the 1x1 shortcut, set through HipBackbone.set_aux_conv_form
        self.cylinder_pad = HEALPixPadding(padding=1) if mesh == "healpix" else CylinderPad(padding)
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=3, padding=0)
        self.conv2 = _zero_module(nn.Conv2d(out_channels, out_channels, kernel_size=3, padding=0))
        self.shortcut = nn.Conv2d(in_channels, out_channels, kernel_size=(1, 1)) if in_channels != out_channels else nn.Identity()
        self.norm1 = nn.GroupNorm(n_groups, in_channels) if norm else nn.Identity()
        self.norm2 = nn.GroupNorm(n_groups, out_channels) if norm else nn.Identity()
        self.cond_emb = nn.Linear(cond_channels, 2 * out_channels if use_scale_shift_norm else out_channels)

    def forward(self, x: torch.Tensor, emb: torch.Tensor) -> torch.Tensor:
        """modern_unet.py:620-650.  `emb` [B', cond]: B' = the leading dimension of x (on the HEALPix mesh the caller has
        already repeated it per face -- the reference cannot broadcast [B, C] against [(B 12), C, h, w] either)."""
        gelu = ops.act_code(self.activation)
        hpx, form = self.mesh == "healpix", self.conv_form
        x = x.contiguous()
        short = x if isinstance(self.shortcut, nn.Identity) else \
            ops.conv2d(x, self.shortcut.weight, self.shortcut.bias, form=self.aux_conv_form)
        n1, n2 = self.norm1, self.norm2
        if isinstance(n1, nn.Identity):
            h = ops.conv3x3(x, self.conv1.weight, self.conv1.bias, pre_act=gelu, hpx=hpx, form=form)
        else:
            h = ops.groupnorm_act(x, n1.weight, n1.bias, n1.num_groups, n1.eps, gelu)
            h = ops.conv3x3(h, self.conv1.weight, self.conv1.bias, hpx=hpx, form=form)
        emb_out = self.cond_emb(emb)[:, :, None, None]
        if not isinstance(n2, nn.Identity) and self.use_scale_shift_norm:
            h = ops.groupnorm_act(h, n2.weight, n2.bias, n2.num_groups, n2.eps, 0)
        if self.use_scale_shift_norm:
            scale, shift = torch.chunk(emb_out, 2, dim=1)
            h = torch.addcmul(shift, h, 1 + scale)                     # norm2(h) * (1 + scale) + shift
            return ops.conv3x3(h, self.conv2.weight, self.conv2.bias, pre_act=gelu, resid=short, hpx=hpx, form=form)
        h = h + emb_out
        if isinstance(n2, nn.Identity):
            return ops.conv3x3(h, self.conv2.weight, self.conv2.bias, pre_act=gelu, resid=short, hpx=hpx, form=form)
        h = ops.groupnorm_act(h, n2.weight, n2.bias, n2.num_groups, n2.eps, gelu)
        return ops.conv3x3(h, self.conv2.weight, self.conv2.bias, resid=short, hpx=hpx, form=form)


class ConditionalHEALPixLayer(nn.Module):
    """utils/healpix.py:117-162 around a ResidualBlock: `layers.0` is the block (it pads inside its kernels)."""

    def __init__(self, layer=ResidualBlock, **kwargs):
        super().__init__()
        if layer is not ResidualBlock:
            raise NotImplementedError("ConditionalHEALPixLayer: only ResidualBlock is used by the reference networks")
        self.layers = nn.Sequential(layer(**kwargs))

    def forward(self, x, emb=None):
        return self.layers[0](x, emb)


class MiddleBlock(nn.Module):
    """modern_unet.py:679-733 (res1, attn, res2; attn an AttentionBlock only when constructed with attention=True --
    DiffModernUNet never asks for one)."""

    def __init__(self, in_channels: int, time_embed_dim: int, attention: bool = False, activation=None, norm: bool = False,
                 use_scale_shift_norm: bool = True, mesh=None):
        super().__init__()
        kw = dict(cond_channels=time_embed_dim, activation=activation, norm=norm, use_scale_shift_norm=use_scale_shift_norm, mesh=mesh)
        self.res1 = ResidualBlock(in_channels, in_channels, **kw)
        self.attn = AttentionBlock(in_channels) if attention else nn.Identity()
        self.res2 = ResidualBlock(in_channels, in_channels, **kw)

    def forward(self, x, emb):
        x = self.res1(x, emb)
        if isinstance(self.attn, AttentionBlock):
            x = self.attn(x)
        return self.res2(x, emb)


def _cond_layer(c_in, c_out, time_embed_dim, mesh, use_scale_shift_norm):
    if mesh == "healpix":    # (the reference does not forward use_scale_shift_norm here: the block's default, True, applies)
        return ConditionalHEALPixLayer(layer=ResidualBlock, in_channels=c_in, out_channels=c_out, cond_channels=time_embed_dim,
                                       kernel_size=3, padding=1, mesh=mesh)
    return ResidualBlock(in_channels=c_in, out_channels=c_out, cond_channels=time_embed_dim, kernel_size=3, padding=1,
                         use_scale_shift_norm=use_scale_shift_norm)


class ModernUNetEncoder(nn.Module):
    """modern_unet.py:325-406: per level [Conv2d(3x3, stride 2) below the top], conditioned ResidualBlock, then the
    level's AttentionBlock (attention=True) or Identity; `attn` is the last level's."""

    def __init__(self, in_channels=2, hidden_channels=(64, 128, 256, 1024), time_embed_dim=1024, activation=None,
                 attention: bool = False, mesh: str = "equirectangular", use_scale_shift_norm=True):
        super().__init__()
        channels = [in_channels] + list(hidden_channels)
        layers = []
        for i in range(len(channels) - 1):
            self.attn = AttentionBlock(channels[i + 1]) if attention else nn.Identity()   # reassigned per level, as :352-355
            layer = []
            if i > 0:
                layer.append(nn.Conv2d(channels[i], channels[i], (3, 3), (2, 2), (1, 1)))
            layer.append(_cond_layer(channels[i], channels[i + 1], time_embed_dim, mesh, use_scale_shift_norm))
            layer.append(self.attn)
            layers.append(nn.Sequential(*layer))
        self.layers = nn.ModuleList(layers)
        self.aux_conv_form = "direct"

    def forward(self, x, emb):
        outs = []
        for layer in self.layers:
            for m in layer:
                if isinstance(m, nn.Conv2d):
                    x = ops.small_module(m, x, form=self.aux_conv_form)
                elif isinstance(m, AttentionBlock):
                    x = m(x)
                elif not isinstance(m, nn.Identity):
                    x = m(x, emb)
            outs.append(x)
        return outs


class ModernUNetDecoder(nn.Module):
    """modern_unet.py:408-497: per level conditioned ResidualBlock (on cat([skip, x]) below the bottom), Identity,
    [ConvTranspose2d(4, 2, 1) above the top]; then GroupNorm(4) -> activation -> 1x1 output convolution.  With attention=True
    the Identity of every level is that level's AttentionBlock, `attn` the last level's (DiffModernUNet never asks for it)."""

    def __init__(self, hidden_channels=(64, 128, 256, 1024), out_channels=2, time_embed_dim=1024, activation=None,
                 attention: bool = False, mesh: str = "equirectangular", use_scale_shift_norm=True):
        super().__init__()
        hidden = list(hidden_channels)[::-1]
        self.activation = _resolve_activation(activation) if activation is not None else nn.GELU()
        layers = []
        for i, c in enumerate(hidden):
            self.attn = AttentionBlock(c) if attention else nn.Identity()                 # reassigned per level, as :438-441
            layer = [_cond_layer(c if i == 0 else 2 * c, c, time_embed_dim, mesh, use_scale_shift_norm), self.attn]
            if i < len(hidden) - 1:
                layer.append(nn.ConvTranspose2d(c, hidden[i + 1], (4, 4), (2, 2), (1, 1)))
            layers.append(nn.Sequential(*layer))
        self.layers = nn.ModuleList(layers)
        self.output_layer = _zero_module(nn.Conv2d(hidden[-1], out_channels, kernel_size=1))
        self.final_norm = nn.GroupNorm(4, hidden[-1])
        self.aux_conv_form = "direct"

    def forward(self, x, skips, emb):
        for i, layer in enumerate(self.layers):
            if i > 0:
                x = torch.cat([skips[i], x], dim=1)
            for m in layer:
                if isinstance(m, nn.ConvTranspose2d):
                    x = ops.small_module(m, x, form=self.aux_conv_form)
                elif isinstance(m, AttentionBlock):
                    x = m(x)
                elif not isinstance(m, nn.Identity):
                    x = m(x, emb)
        fn = self.final_norm
        x = ops.groupnorm_act(x, fn.weight, fn.bias, fn.num_groups, fn.eps, ops.act_code(self.activation))
        return ops.small_module(self.output_layer, x, form=self.aux_conv_form)


class DiffModernUNet(HipBackbone):
    """modern_unet.py:46-293.  A HipBackbone for its precision knobs (`compute_precision`, set_conv_form); the denoising
    loop below is its own, no step graph is captured."""

    def __init__(self, constant_channels: int = 4, prescribed_channels: int = 0, prognostic_channels: int = 1,
                 hidden_channels=(64, 128, 256, 1024), activation=None, context_size: int = 1, mesh: str = "equirectangular",
                 attention: bool = False, norm: bool = False, use_scale_shift_norm=True, predict_diff=True,
                 num_refinement_step=5, **kwargs):
        super().__init__()
        activation = _resolve_activation(activation) if activation is not None else nn.GELU()
        self.context_size = context_size
        self.mesh = mesh
        self.hidden_channels = list(hidden_channels)
        time_embed_dim = self.hidden_channels[0] * 4
        self.activation = activation
        self.predict_diff = predict_diff
        self.num_refinement_step = num_refinement_step
        self.time_embed = nn.Sequential(nn.Linear(self.hidden_channels[0], time_embed_dim), self.activation,
                                        nn.Linear(time_embed_dim, time_embed_dim))
        in_channels = constant_channels + (prescribed_channels + prognostic_channels) * context_size + prognostic_channels * context_size
        self.encoder = ModernUNetEncoder(in_channels=in_channels, hidden_channels=self.hidden_channels,
                                         time_embed_dim=time_embed_dim, activation=activation, attention=attention, mesh=mesh,
                                         use_scale_shift_norm=use_scale_shift_norm)
        # the flag reaches the encoder only (:94-121): middle block and decoder keep their Identity slots
        self.middle = MiddleBlock(in_channels=self.hidden_channels[-1], time_embed_dim=time_embed_dim, norm=norm,
                                  activation=activation, use_scale_shift_norm=use_scale_shift_norm, mesh=mesh)
        self.decoder = ModernUNetDecoder(hidden_channels=self.hidden_channels, out_channels=prognostic_channels,
                                         time_embed_dim=time_embed_dim, activation=activation, mesh=mesh,
                                         use_scale_shift_norm=use_scale_shift_norm)
        self._init_compute_precision(kwargs)

    def set_step_graphs(self, on: bool = True):
        """The denoising loop draws host noise and steps a host scheduler between network calls: there is no `one_step` to
        capture, so asking for step graphs is an error rather than a silent no-op."""
        if on:
            raise _lib.DlwpError(f"{type(self).__name__} has no captured step: its refinement loop runs on the host")
        return super().set_step_graphs(False)

    # ---- modern_unet.py:120-139
    def _prepare_inputs(self, constants=None, prescribed=None, prognostic=None) -> torch.Tensor:
        tensors = []
        if constants is not None:
            tensors.append(constants[:, 0])
        if prescribed is not None:
            tensors.append(prescribed.flatten(1, 2))
        if prognostic is not None:
            tensors.append(prognostic.flatten(1, 2))
        return torch.cat(tensors, dim=1)

    # ---- modern_unet.py:141-176
    def single_forward(self, constants, prescribed, prognostic, y_noised, time):
        time = time * (1000 / self.num_refinement_step)
        if prognostic.ndim == 6:
            prognostic = fold_faces(prognostic)
        if y_noised.ndim == 5:
            y_noised = y_noised.expand(-1, prognostic.shape[1], -1, -1, -1)
        elif y_noised.ndim == 6:
            y_noised = fold_faces(y_noised.expand(-1, prognostic.shape[1], -1, -1, -1, -1))
        prognostic_t = torch.cat([prognostic, y_noised], dim=2)
        x_t = self._prepare_inputs(constants=constants, prescribed=prescribed, prognostic=prognostic_t).contiguous()
        emb = self.time_embed(fourier_embedding(time, self.hidden_channels[0]))
        enc = self.encoder(x_t, emb)
        mid = self.middle(enc[-1], emb)
        return self.decoder(mid, enc[::-1], emb)

    # ---- modern_unet.py:178-211
    def diffusion_forward(self, constants, prescribed, prognostic, noise_scheduler, target_shape):
        if prognostic.ndim == 6:
            prognostic = fold_faces(prognostic)
        if len(target_shape) == 6:
            b, t, c, f, h, w = target_shape
            target_shape = (b * f, t, c, h, w)
        device_randn = getattr(noise_scheduler, "randn", None)      # schedulers.RefinerScheduler: the start noise is its draw
        if device_randn is not None:
            y_noised = device_randn(tuple(target_shape), prognostic.device)
        else:
            y_noised = torch.randn(target_shape).to(device=prognostic.device)      # host RNG, as the reference (:186)
        for k in noise_scheduler.timesteps:
            k_tensor = torch.full((prognostic.shape[0],), int(k), dtype=torch.long, device=prognostic.device)
            pred = self.single_forward(constants, prescribed, prognostic, y_noised, time=k_tensor).unsqueeze(1)
            y_noised = noise_scheduler.step(pred, k, y_noised).prev_sample
        return y_noised.to(prognostic.device).flatten(1, 2)

    # ---- modern_unet.py:214-293
    def forward(self, constants: Optional[torch.Tensor] = None, prescribed: Optional[torch.Tensor] = None,
                prognostic: torch.Tensor = None, noise_scheduler=None, target: Optional[torch.Tensor] = None) -> torch.Tensor:
        if prognostic is None or noise_scheduler is None:
            raise _lib.DlwpError("prognostic and noise_scheduler are required")
        _lib.require_cuda_tensor(prognostic, "prognostic")
        prescribed_input = prescribed
        if self.mesh == "healpix":
            bsz, nf = prognostic.shape[0], prognostic.shape[3]
        outs = []
        with torch.no_grad():
            for t in range(self.context_size, prognostic.shape[1]):
                t_start = max(0, t - self.context_size)
                if t == self.context_size:
                    prognostic_t = prognostic[:, t_start:t]
                    prescribed = prescribed[:, t_start:t] if prescribed is not None else None
                else:
                    prognostic_t = torch.cat([prognostic[:, t_start:self.context_size],
                                              torch.stack(outs, dim=1)[:, -self.context_size:]], dim=1)
                    prescribed = prescribed_input[:, t - self.context_size:t] if prescribed_input is not None else None
                tshape = prognostic[:, t].unsqueeze(1).shape
                out = self.diffusion_forward(constants, prescribed, prognostic_t, noise_scheduler, tshape)
                if self.mesh == "healpix":
                    out = out.reshape(bsz, nf, *out.shape[1:]).permute(0, 2, 1, 3, 4)
                outs.append(prognostic_t[:, -1] + out)      # the network predicts the residual (:289)
        return torch.stack(outs, dim=1)


class DiffMUNetHPX(DiffModernUNet):
    """modern_unet.py:295-327: the same network on [.., 12, h, w] HEALPix data, faces folded into the batch dimension."""

    def __init__(self, constant_channels: int = 4, prescribed_channels: int = 0, prognostic_channels: int = 1,
                 hidden_channels=(64, 128, 256, 1024), activation=None, context_size: int = 1, mesh: str = "healpix",
                 attention: bool = False, norm: bool = False, use_scale_shift_norm=True, predict_diff=True,
                 num_refinement_step=5, **kwargs):
        super().__init__(constant_channels=constant_channels, prescribed_channels=prescribed_channels,
                         prognostic_channels=prognostic_channels, hidden_channels=hidden_channels, activation=activation,
                         context_size=context_size, mesh="healpix", attention=attention, norm=norm,
                         use_scale_shift_norm=use_scale_shift_norm, predict_diff=predict_diff,
                         num_refinement_step=num_refinement_step, **kwargs)

    def _prepare_inputs(self, constants=None, prescribed=None, prognostic=None) -> torch.Tensor:
        """:314-327: [(B F), (T C), H, W]."""
        fold = lambda t: fold_faces(t).flatten(1, 2)

        tensors = []
        if constants is not None:
            tensors.append(fold(constants[:, :1]))
        if prescribed is not None:
            tensors.append(fold(prescribed))
        if prognostic is not None:
            tensors.append(fold(prognostic) if prognostic.ndim == 6 else prognostic.flatten(1, 2))
        return torch.cat(tensors, dim=1)
