"""The hot kernels under autograd (reference scripts/train.py:263-271 runs `loss.backward()` through the
backbone): one autograd Function per kernel family, each with a HIP forward and a HIP backward, and the entry points the
ops call when a gradient is wanted (`wants_grad`).  First the spectral convolution, then window and global attention,
the AFNO filter, HEALPix padding, the cylinder / HEALPix 3x3 convolution, Conv2d and ConvTranspose2d, the ConvLSTM cell,
GroupNorm, Linear, MeshGraphNet and GraphCastNet.

Every family but the spectral one also has a torch form: the same operator in plain torch operators (a restatement of
the reference arithmetic that imports nothing from the oracle).  Autograd of that form is the cross-check of the HIP
backward (`DLWP_TRAIN_TORCH_BACKWARD=1`, tests/test_training_gpu.py and the per-kernel tests) and the fallback for shapes
outside a backward kernel's envelope: a Function's backward differentiates it through `_grad_of_torch_form`; Conv2d,
ConvTranspose2d, GroupNorm and Linear leave the plain composition in the graph instead of their Function.

The spectral convolutions (models/unet/unet.py:46-69 `SpectralConv2d`, and neuralop's SpectralConv inside
`FNO2DModule`, fno.py:38-47): the reference's autograd differentiates rfft2 / einsum / irfft2.  Here

  forward        y  = S_W(x)                           dlwp_spectral_conv2d_f32 (pruned-DFT MFMA kernels)
  backward-data  dx = S_{W^H}(dy)                      the SAME kernels: rows_in/rows_out swapped, weights
                                                       conjugate-transposed on the device (exact adjoint: the
                                                       Hermitian weights of the half spectrum cancel per column)
  backward-weight dW[i,o,r,k] = sum_b conj(fwd * X[b,i,rows_in[r],k]) * inv * c_k * DY[b,o,rows_out[r],k]
                                                       dlwp_spectral_conv2d_wgrad_f32: the pruned forward transform of x
                                                       and of grad_y at the kept modes, one fp32 contraction kernel, one transpose
                                                       (csrc/spectral_any.hip; no rocFFT plan, no torch GEMM)

with c_k = 1 for k = 0 and the Nyquist column, 2 otherwise.  The identities are checked against autograd of
the reference operator in tests (CPU, double) and against reference gradients on the GPU.  `spectral_weight_grad` below
is the same formula in plain torch on any device: the checker of the kernel and the timing baseline, not what the GPU
path calls.

Everything pointwise around the spectral operator (1x1 convolutions, GELU, residuals) stays in torch ops on
the GPU in training mode.
"""
import ctypes
import functools
import math
import os
from typing import Optional, Sequence

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import healpix as _hpx
from . import lib as _lib
from . import ops       # called as ops.name(...), the attribute tests and tools replace; ops imports this module lazily


def spectral_weight_grad(x, grad_y, rows_in, rows_out, n_cols: int, fwd_scale: float, inv_scale: float):
    """dL/dW as the real view [Ci, Co, n_rows, n_cols, 2] (formula in the module docstring); plain torch, any device."""
    w = x.shape[-1]
    ck = torch.full((n_cols,), 2.0, device=x.device, dtype=x.dtype)
    ck[0] = 1.0
    if w % 2 == 0 and n_cols == w // 2 + 1:
        ck[-1] = 1.0
    ri = torch.as_tensor(list(rows_in), device=x.device)
    ro = torch.as_tensor(list(rows_out), device=x.device)
    xf = torch.fft.rfft2(x)[:, :, ri, :n_cols]
    gf = torch.fft.rfft2(grad_y)[:, :, ro, :n_cols]
    gw = torch.einsum("bixy,boxy->ioxy", xf.conj() * fwd_scale, gf * (ck * inv_scale))
    return torch.view_as_real(gw).contiguous()


class SpectralOperator:
    """Forward + adjoint plans of one mode-truncated spectral convolution geometry, `channels` -> `out_channels`
    (square when `out_channels` is omitted); the adjoint plan is `out_channels` -> `channels` with the row lists swapped.
    32 -> 32 channels on a width that is a multiple of 64 with at most 16 kept columns run the specialised kernels;
    every other shape up to 512 channels (width a multiple of 4) the width-generic ones (csrc/spectral_any.hip).

    The weight gradient has the width-generic form only (Ci, Co <= 512, width a multiple of 4, the [H16][2 n_cols16 + 1]
    fp32 LDS image of one plane within 128 KB).  The specialised forward's shapes lie inside that domain up to about 990
    rows; a taller 32-channel grid runs forward and backward-data but `backward_weight` raises DlwpError.  There is no
    torch fallback."""

    def __init__(self, channels: int, height: int, width: int, rows_in: Sequence[int], rows_out: Sequence[int],
                 n_cols: int, fwd_scale: float, inv_scale: float, device, out_channels: Optional[int] = None):
        self.channels, self.h, self.w = int(channels), height, width
        self.out_channels = self.channels if out_channels is None else int(out_channels)
        self.rows_in = [int(r) for r in rows_in]
        self.rows_out = [int(r) for r in rows_out]
        self.n_cols = int(n_cols)
        self.fwd_scale, self.inv_scale = float(fwd_scale), float(inv_scale)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DlwpError(f"SpectralOperator runs HIP kernels on an MI355X device, got {self.device}: "
                                 "the HIP path has no CPU fallback")
        n = len(self.rows_in)
        ri = (ctypes.c_int32 * n)(*self.rows_in)
        ro = (ctypes.c_int32 * n)(*self.rows_out)
        ci, co = self.channels, self.out_channels
        self._fwd, self._adj = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.launch("dlwp_spectral_conv2d_plan_create_ex", self.device, ctypes.byref(self._fwd), ci, co, height, width, n,
                    self.n_cols, ri, ro, self.fwd_scale, self.inv_scale)
        _lib.launch("dlwp_spectral_conv2d_plan_create_ex", self.device, ctypes.byref(self._adj), co, ci, height, width, n,
                    self.n_cols, ro, ri, self.fwd_scale, self.inv_scale)
        self._ws = {}         # device -> kernel workspaces, kept when they grow (lib.kept_workspace)

    def __del__(self):
        try:
            lib = _lib.load()
            for p in (self._fwd, self._adj):
                if p:
                    lib.dlwp_spectral_conv2d_plan_destroy(p)
        except Exception:
            pass

    def _workspace(self, nbytes: int, device) -> torch.Tensor:
        return _lib.kept_workspace(self._ws, nbytes, device, floor=256)

    def _run(self, plan, x: torch.Tensor, weight_real: torch.Tensor, adjoint: bool) -> torch.Tensor:
        _lib.require_cuda_tensor(x, "x")
        x = x.contiguous().float()
        w = weight_real.detach().contiguous().float()
        b, c, h, wd = x.shape
        n = len(self.rows_in)
        ci, co = self.channels, self.out_channels
        c_in, c_out = (co, ci) if adjoint else (ci, co)
        if (c, h, wd) != (c_in, self.h, self.w) or tuple(w.shape) != (ci, co, n, self.n_cols, 2):
            raise _lib.DlwpError(f"spectral operator built for {ci}->{co} channels on {self.h}x{self.w}, "
                                 f"{n}x{self.n_cols} modes; got x {tuple(x.shape)}, weight {tuple(w.shape)}"
                                 + (" (adjoint)" if adjoint else ""))
        nbytes = _lib.load().dlwp_spectral_conv2d_workspace_bytes(plan, b)
        ws = self._workspace(nbytes, x.device)
        y = torch.empty(b, c_out, h, wd, device=x.device, dtype=torch.float32)
        _lib.launch("dlwp_spectral_conv2d_set_weights_dev", x.device, plan, w, 1 if adjoint else 0)
        _lib.launch("dlwp_spectral_conv2d_f32", x.device, plan, x, y, b, ws, nbytes)
        return y

    def forward(self, x, weight_real):
        return self._run(self._fwd, x, weight_real, False)

    def backward_data(self, grad_y, weight_real):
        return self._run(self._adj, grad_y, weight_real, True)

    def backward_weight(self, x, grad_y):
        """[Ci, Co, n_rows, n_cols, 2] gradient of the real view of the weights: dlwp_spectral_conv2d_wgrad_f32 on the
        forward plan (four launches on the current stream; bitwise repeatable)."""
        _lib.require_cuda_tensor(x, "x")
        _lib.require_cuda_tensor(grad_y, "grad_y")
        x = x.detach().contiguous().float()
        grad_y = grad_y.detach().contiguous().float()
        b = x.shape[0]
        ci, co = self.channels, self.out_channels
        if tuple(x.shape) != (b, ci, self.h, self.w) or tuple(grad_y.shape) != (b, co, self.h, self.w):
            raise _lib.DlwpError(f"spectral operator built for {ci}->{co} channels on {self.h}x{self.w}; "
                                 f"got x {tuple(x.shape)}, grad_y {tuple(grad_y.shape)}")
        nbytes = _lib.load().dlwp_spectral_conv2d_wgrad_workspace_bytes(self._fwd, b)
        ws = self._workspace(nbytes, x.device)
        gw = torch.empty(ci, co, len(self.rows_in), self.n_cols, 2, device=x.device, dtype=torch.float32)
        _lib.launch("dlwp_spectral_conv2d_wgrad_f32", x.device, self._fwd, x, grad_y, gw, b, ws, nbytes)
        return gw


class _SpectralConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight_real, op: SpectralOperator):
        ctx.op = op
        ctx.save_for_backward(x, weight_real)
        return op.forward(x, weight_real)

    @staticmethod
    def backward(ctx, grad_y):
        x, weight_real = ctx.saved_tensors
        op = ctx.op
        grad_y = grad_y.contiguous()
        gx = op.backward_data(grad_y, weight_real) if ctx.needs_input_grad[0] else None
        gw = op.backward_weight(x, grad_y) if ctx.needs_input_grad[1] else None
        return gx, gw, None


def spectral_conv(x: torch.Tensor, weight_real: torch.Tensor, op: SpectralOperator) -> torch.Tensor:
    """Differentiable mode-truncated spectral convolution; weight_real [Ci, Co, n_rows, n_cols, 2]."""
    return _SpectralConvFn.apply(x, weight_real, op)


def pde_arena_rows(height: int, modes1: int):
    """Kept rows of reference unet.py:60-65 (`[:m1]` with weights1, `[-m1:]` with weights2)."""
    rows = list(range(modes1)) + list(range(height - modes1, height))
    return rows, rows


# =====================================================================================================================
# Training through the other hot kernels (reference scripts/train.py:263-271 `loss.backward()`)
#
# Each Function below runs the inference kernels forward (Conv2d / ConvTranspose2d: the library's) and a HIP kernel
# backward.  Beside each stands its torch form (`*_torch`), the operator restated in torch operators, which
# `_grad_of_torch_form` differentiates where the backward kernel answers "unsupported" and everywhere under
# DLWP_TRAIN_TORCH_BACKWARD=1.  What the Functions share comes first.
# =====================================================================================================================
_ACT_FNS = {0: lambda t: t, 1: F.gelu, 2: torch.tanh, 3: F.relu, 4: F.silu}     # the activation codes of ops.ACTS


def _torch_backward_selected() -> bool:
    """DLWP_TRAIN_TORCH_BACKWARD=1: every operator's gradient comes from autograd of its torch form, none from a HIP
    backward (the cross-check the tests and benches use).  Read at every call."""
    return os.environ.get("DLWP_TRAIN_TORCH_BACKWARD", "0") == "1"


def _grad_of_torch_form(fn, inputs, needs, grad_outs, params=(), zero_fill: bool = False):
    """The backward of a Function by autograd of its torch form.  fn is called under enable_grad on detached `inputs`
    (tensors or None) that require a gradient where the matching flag of `needs` is set; its output -- a tensor, or a tuple
    of which the entries whose `grad_outs` is None are left out -- is differentiated in one torch.autograd.grad call with
    respect to the needed inputs and to `params`, the live Parameters fn closes over.  Returns a list: one gradient per input
    (None for a None or unneeded one), then one per parameter.  A tensor the outputs do not depend on gets None, or zeros
    under zero_fill (a Parameter's .grad is then a tensor whether or not this layer reached it)."""
    with torch.enable_grad():
        ins = [t.detach().requires_grad_(bool(need)) if t is not None else None for t, need in zip(inputs, needs)]
        outs = fn(*ins)
        if isinstance(outs, torch.Tensor):
            outs, grad_outs = (outs,), (grad_outs,)
        pairs = [(o, g.reshape(o.shape).contiguous()) for o, g in zip(outs, grad_outs) if g is not None]
        wrt = [t for t in ins if t is not None and t.requires_grad] + list(params)
        grads = torch.autograd.grad([o for o, _ in pairs], wrt, [g for _, g in pairs], allow_unused=True) if wrt else ()
    if zero_fill:
        grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, wrt)]
    grads = iter(grads)
    return [next(grads) if t is not None and t.requires_grad else None for t in ins] + list(grads)


# Two activation derivatives, because two things must be reproduced.  _act_backward runs torch's own backward kernel of the
# activation, so the convolution Functions return the bits autograd gives for the plain composition.  _act_grad_torch is the
# closed form dlwp_groupnorm_act_bwd_f32 evaluates: the term-by-term reference of that kernel's arithmetic
# (groupnorm_act_backward_torch).
def _act_backward(v, grad, act: int):
    """grad * act'(v) by autograd of the torch activation (the kernel the plain composition's backward runs)"""
    if act == 0:
        return grad
    with torch.enable_grad():
        v_ = v.detach().requires_grad_(True)
        g, = torch.autograd.grad(_ACT_FNS[act](v_), v_, grad)
    return g


def _act_grad_torch(v: torch.Tensor, act: int) -> torch.Tensor:
    """act'(v) for the activation codes of ops.ACTS (0 identity, 1 exact-erf GELU, 2 tanh, 3 ReLU, 4 SiLU)"""
    if act == 1:
        return 0.5 * (1.0 + torch.erf(v * 0.7071067811865476)) + v * torch.exp(-0.5 * v * v) * 0.3989422804014327
    if act == 2:
        return 1.0 - torch.tanh(v) ** 2
    if act == 3:
        return (v > 0).to(v.dtype)
    if act == 4:
        s = torch.sigmoid(v)
        return s * (1.0 + v * (1.0 - s))
    if act != 0:
        raise _lib.DlwpError(f"unknown activation {act}")
    return torch.ones_like(v)


@functools.lru_cache(maxsize=64)
def _window_tables(grid, padded, pad_lead, window, shift_fwd, use_mask, mask_b1, mask_b2, bias_mode, device_str):
    """bias index [N, N] (long) and region ids [n_pl, n_lat, n_lon, N] of one window geometry, on the device."""
    dev = torch.device(device_str)
    wpl, wlat, wlon = window
    n = wpl * wlat * wlon
    z = torch.arange(n)
    zlon, zlat, zpl = z % wlon, (z // wlon) % wlat, z // (wlon * wlat)
    q, k = slice(None), slice(None)
    if bias_mode == 0:
        idx = (zlat[:, None] - zlat[None, :] + wlat - 1) * (2 * wlon - 1) + (zlon[:, None] - zlon[None, :] + wlon - 1)
    else:   # earth-specific (utils/earth_position_index.py): query coordinate + window * key coordinate, relative longitude
        idx = ((zpl[:, None] + zpl[None, :] * wpl) * wlat * wlat + (zlat[:, None] + zlat[None, :] * wlat)) * (2 * wlon - 1) + \
              (zlon[:, None] - zlon[None, :] + wlon - 1)
    npl, nlat, nlon = padded[0] // wpl, padded[1] // wlat, padded[2] // wlon
    region = None
    if use_mask:
        P = (torch.arange(npl)[:, None] * wpl + zpl[None, :])          # [npl, N]
        A = (torch.arange(nlat)[:, None] * wlat + zlat[None, :])
        O = (torch.arange(nlon)[:, None] * wlon + zlon[None, :])
        rp = (P >= mask_b1[0]).long() + (P >= mask_b2[0]).long()
        ra = (A >= mask_b1[1]).long() + (A >= mask_b2[1]).long()
        ro = (O >= mask_b1[2]).long() + (O >= mask_b2[2]).long()
        region = ((rp[:, None, None, :] * 3 + ra[None, :, None, :]) * 3 + ro[None, None, :, :]).to(dev)
    return idx.to(dev), region


def window_attention_torch(qkv: torch.Tensor, qkv_bias, table: torch.Tensor, spec) -> torch.Tensor:
    """What dlwp_window_attn_f32 computes, with torch operators (differentiable in qkv, qkv_bias, table):
    swin_transformer.py:217-251 + :122-154 (bias_mode 0) / panguweather.py:285-316 + :176-211 (bias_mode 1)."""
    b, l, c3 = qkv.shape
    heads, d = spec.heads, spec.head_dim
    c = heads * d
    pl, lat, lon = spec.grid
    ppl, plat, plon = spec.padded
    wpl, wlat, wlon = spec.window
    x = qkv.view(b, pl, lat, lon, c3)
    f, t, lft = spec.pad_lead
    pads = (0, 0, lft, plon - lon - lft, t, plat - lat - t, f, ppl - pl - f)
    if any(pads):
        # zero-padded tokens enter the qkv Linear as zeros: their q, k, v are the bias
        x = F.pad(x - qkv_bias, pads) + qkv_bias if qkv_bias is not None else F.pad(x, pads)
    sf = tuple(int(s) for s in spec.shift_fwd)
    if any(sf):
        x = torch.roll(x, shifts=(-sf[0], -sf[1], -sf[2]), dims=(1, 2, 3))
    npl, nlat, nlon = ppl // wpl, plat // wlat, plon // wlon
    n = wpl * wlat * wlon
    x = x.view(b, npl, wpl, nlat, wlat, nlon, wlon, 3, heads, d).permute(0, 1, 3, 5, 7, 8, 2, 4, 6, 9)
    x = x.reshape(b, npl, nlat, nlon, 3, heads, n, d)
    q, k, v = x[:, :, :, :, 0] * spec.scale, x[:, :, :, :, 1], x[:, :, :, :, 2]
    idx, region = _window_tables(tuple(spec.grid), tuple(spec.padded), tuple(spec.pad_lead), tuple(spec.window), sf,
                                 bool(spec.use_mask), tuple(int(v_) for v_ in spec.mask_b1),
                                 tuple(int(v_) for v_ in spec.mask_b2), int(spec.bias_mode), str(qkv.device))
    attn = q @ k.transpose(-1, -2)                                      # [b, npl, nlat, nlon, heads, N, N]
    if spec.bias_mode == 0:
        bias = table[idx.reshape(-1)].view(n, n, heads).permute(2, 0, 1)                    # [heads, N, N]
        attn = attn + bias
    else:
        types = npl * nlat
        bias = table[idx.reshape(-1)].view(n, n, types, heads).permute(2, 3, 0, 1)          # [types, heads, N, N]
        attn = attn + bias.view(npl, nlat, 1, heads, n, n)
    if spec.use_mask:
        diff = region.unsqueeze(-1) != region.unsqueeze(-2)                                  # [npl, nlat, nlon, N, N]
        attn = attn + torch.where(diff, -100.0, 0.0).to(attn.dtype).unsqueeze(3)
    attn = torch.softmax(attn, dim=-1)
    o = attn @ v                                                       # [b, npl, nlat, nlon, heads, N, d]
    o = o.view(b, npl, nlat, nlon, heads, wpl, wlat, wlon, d).permute(0, 1, 5, 2, 6, 3, 7, 4, 8)
    o = o.reshape(b, ppl, plat, plon, c)
    sb = tuple(int(s) for s in spec.shift_back)
    if any(sb):
        o = torch.roll(o, shifts=sb, dims=(1, 2, 3))
    o = o[:, f:f + pl, t:t + lat, lft:lft + lon]
    return o.reshape(b, l, c)


class _WindowAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, qkv_bias, table, spec, precision):
        ctx.spec = spec
        ctx.save_for_backward(qkv, qkv_bias, table)
        with torch.no_grad():
            return ops.window_attention(qkv.detach(), qkv_bias.detach() if qkv_bias is not None else None,
                                        table.detach(), spec, precision=precision)

    @staticmethod
    def backward(ctx, grad_out):
        """HIP backward (dlwp_window_attn_bwd_f32): scores recomputed tile by tile, no [B, heads, N, N] tensor.  Descriptors the
        kernel does not cover (a bias column that does not fit LDS) and DLWP_TRAIN_TORCH_BACKWARD=1 (the cross-check the tests
        use) differentiate window_attention_torch; any other error raises."""
        qkv, qkv_bias, table = ctx.saved_tensors
        needs = ctx.needs_input_grad[:3]
        if not _torch_backward_selected():
            try:
                gq, gb, gt = ops.window_attention_backward(qkv, qkv_bias, table, ctx.spec, grad_out)
                if qkv_bias is not None and gb is None:
                    gb = torch.zeros_like(qkv_bias) if needs[1] else None
                return (gq if needs[0] else None, gb if needs[1] else None, gt if needs[2] else None, None, None)
            except _lib.DlwpError as e:
                if e.status != _lib.ERR_UNSUPPORTED:
                    raise
        return (*_grad_of_torch_form(lambda q, b, t: window_attention_torch(q, b, t, ctx.spec), (qkv, qkv_bias, table), needs,
                                     grad_out), None, None)


def window_attention(qkv, qkv_bias, table, spec, precision="fp32"):
    """differentiable window attention: HIP forward and HIP backward"""
    return _WindowAttentionFn.apply(qkv, qkv_bias, table, spec, precision)


def global_attention_torch(qkv: torch.Tensor, heads: int, d_k: int, scale: float) -> torch.Tensor:
    """What dlwp_global_attn_f32 computes, with torch operators (differentiable in qkv): modern_unet.py:558-571 between the
    two Linears, qkv [Bt, N, heads 3 d_k] -> [Bt, N, heads d_k], softmax over the queries.  Forms the N x N scores."""
    bt, n = qkv.shape[:2]
    q, k, v = qkv.reshape(bt, n, heads, 3, d_k).unbind(3)
    p = torch.softmax(torch.einsum("bihd,bjhd->bhij", q, k) * scale, dim=2)
    return torch.einsum("bhij,bjhd->bihd", p, v).reshape(bt, n, heads * d_k)


class _GlobalAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, heads, d_k, scale):
        with torch.no_grad():
            out, stats = ops.global_attention(qkv.detach(), heads, d_k, scale, return_stats=True)
        ctx.cfg = (heads, d_k, scale)
        ctx.save_for_backward(qkv, stats)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        """HIP backward (dlwp_global_attn_bwd_f32) from the forward's per-key statistics: no N x N tensor.  DLWP_ERR_UNSUPPORTED
        (head_dim above 1024) and DLWP_TRAIN_TORCH_BACKWARD=1 (the cross-check the tests use) differentiate
        global_attention_torch; any other error raises."""
        qkv, stats = ctx.saved_tensors
        heads, d_k, scale = ctx.cfg
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        if not _torch_backward_selected():
            try:
                return ops.global_attention_backward(qkv, stats, grad_out, heads, d_k, scale), None, None, None
            except _lib.DlwpError as e:
                if e.status != _lib.ERR_UNSUPPORTED:
                    raise
        g, = _grad_of_torch_form(lambda q: global_attention_torch(q, heads, d_k, scale), (qkv,), (True,), grad_out)
        return g, None, None, None


def global_attention(qkv, heads: int, d_k: int, scale: float):
    """differentiable global attention of the diffusion AttentionBlock: HIP forward and HIP backward"""
    return _GlobalAttentionFn.apply(qkv, heads, d_k, scale)


def afno_filter_torch(x_cf, w1, b1, w2, b2, num_blocks: int, sparsity_threshold: float, hard_thresholding_fraction: float):
    """fourcastnet.py:85-124 on a CHANNELS-FIRST field (without the `+ bias` of :127), torch operators."""
    b, c, h, w = x_cf.shape
    bs = c // num_blocks
    xf = torch.fft.rfft2(x_cf.float(), norm="ortho")                               # [b, c, h, wf]
    xf = xf.permute(0, 2, 3, 1).reshape(b, h, w // 2 + 1, num_blocks, bs)
    total = h // 2 + 1
    kept = int(total * hard_thresholding_fraction)
    rows = slice(max(total - kept, 0), min(total + kept, h))
    xr, xi = xf.real[:, rows, :kept], xf.imag[:, rows, :kept]
    ein = lambda a, m: torch.einsum("...bi,bio->...bo", a, m)
    o1r = F.relu(ein(xr, w1[0]) - ein(xi, w1[1]) + b1[0])
    o1i = F.relu(ein(xi, w1[0]) + ein(xr, w1[1]) + b1[1])
    o2r = ein(o1r, w2[0]) - ein(o1i, w2[1]) + b2[0]
    o2i = ein(o1i, w2[0]) + ein(o1r, w2[1]) + b2[1]
    z = F.softshrink(torch.stack([o2r, o2i], dim=-1), lambd=sparsity_threshold)
    full = torch.zeros(b, h, w // 2 + 1, num_blocks, bs, 2, device=x_cf.device, dtype=torch.float32)
    full = _put(full, rows, kept, z)
    yf = torch.view_as_complex(full).reshape(b, h, w // 2 + 1, c).permute(0, 3, 1, 2)
    return torch.fft.irfft2(yf, s=(h, w), norm="ortho")


def _put(full, rows, kept, z):
    full = full.clone()
    full[:, rows, :kept] = z
    return full


class _AfnoFilterFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_cf, w1, b1, w2, b2, num_blocks, lam, frac):
        ctx.cfg = (num_blocks, lam, frac)
        ctx.save_for_backward(x_cf, w1, b1, w2, b2)
        with torch.no_grad():
            return ops.afno2d_filter_cf(x_cf.detach(), w1.detach(), b1.detach(), w2.detach(), b2.detach(), num_blocks, lam, frac)

    @staticmethod
    def backward(ctx, grad_out):
        """HIP backward (ops.afno2d_filter_backward: the hand-written transforms around dlwp_afno2d_mix_bwd_f32); grids / block
        sizes it does not take and DLWP_TRAIN_TORCH_BACKWARD=1 differentiate afno_filter_torch."""
        saved = ctx.saved_tensors
        needs = ctx.needs_input_grad[:5]
        if not _torch_backward_selected():
            res = ops.afno2d_filter_backward(saved[0], grad_out, saved[1], saved[2], saved[3], saved[4], *ctx.cfg)
            if res is not None:
                return (*[g if need else None for g, need in zip(res, needs)], None, None, None)
        return (*_grad_of_torch_form(lambda *a: afno_filter_torch(*a, *ctx.cfg), saved, needs, grad_out), None, None, None)


def afno_filter(x_cf, w1, b1, w2, b2, num_blocks, lam, frac):
    return _AfnoFilterFn.apply(x_cf, w1, b1, w2, b2, num_blocks, lam, frac)


def _hpx_pad_torch(x, table):
    """HEALPixPadding(p) as a differentiable gather: x [(B*12), C, H, W], table int32 [12, (H+2p)(W+2p), 2]."""
    n, c, h, w = x.shape
    p = (int(round(table.shape[1] ** 0.5)) - h) // 2
    bsz = n // 12
    flat = x.view(bsz, 12, c, h * w).permute(0, 2, 1, 3).reshape(bsz, c, 12 * h * w)
    a = table[:, :, 0].long().reshape(-1)
    b_ = table[:, :, 1].long().reshape(-1)
    va = flat[:, :, a]
    vb = flat[:, :, b_.clamp(min=0)]
    v = torch.where((b_ >= 0).view(1, 1, -1), 0.5 * va + 0.5 * vb, va)
    return v.view(bsz, c, 12, h + 2 * p, w + 2 * p).permute(0, 2, 1, 3, 4).reshape(n, c, h + 2 * p, w + 2 * p)


class _HpxPadFn(torch.autograd.Function):
    """HEALPixPadding(p) (reference utils/healpix.py:165-368) for any p: dlwp_healpix_pad_f32 forward, its adjoint
    dlwp_healpix_pad_bwd_f32 (the gather through healpix.pad_adjoint_table) backward; DLWP_TRAIN_TORCH_BACKWARD=1
    differentiates the torch gather _hpx_pad_torch instead."""

    @staticmethod
    def forward(ctx, x, padding):
        ctx.padding = padding
        ctx.save_for_backward(x)
        with torch.no_grad():
            return ops.healpix_pad(x.detach(), padding)

    @staticmethod
    def backward(ctx, grad_out):
        if not _torch_backward_selected():
            with torch.no_grad():
                return ops.healpix_pad_backward(grad_out, ctx.padding), None
        x, = ctx.saved_tensors
        table = _hpx.device_table(x.shape[2], x.shape[3], ctx.padding, x.device)
        gx, = _grad_of_torch_form(lambda t: _hpx_pad_torch(t, table), (x,), (True,), grad_out)
        return gx, None


def healpix_pad(x, padding: int):
    return _HpxPadFn.apply(x, int(padding))


def conv3x3_torch(x0, x1, weight, bias, resid, pre_act: int, act: int, hpx_table=None):
    """pad(1) + Conv2d(3x3) (+ fusions) with torch operators: CylinderPad (utils/utils.py:11-26) or HEALPixPadding."""
    x = x0 if x1 is None else torch.cat([x0, x1], dim=1)
    x = _ACT_FNS[pre_act](x)
    if hpx_table is not None:
        x = _hpx_pad_torch(x, hpx_table)
    else:
        x = F.pad(F.pad(x, (1, 1, 0, 0), mode="circular"), (0, 0, 1, 1))
    y = F.conv2d(x, weight, bias)
    if resid is not None:
        y = y + resid
    return _ACT_FNS[act](y)


def conv3x3_weight_grad_torch(x0, x1, gz, pre_act: int, hpx_table=None, need_weight: bool = True, need_bias: bool = True):
    """(dW, db) of conv3x3_torch from gz, the gradient of the convolution's output, as the composition of library operators:
    torch.cat, the pre-activation, the padded copy, torch.nn.grad.conv2d_weight (MIOpen on the GPU) and gz.sum.  On any device:
    the DLWP_CONV_WGRAD=torch path of _Conv3x3Fn.backward, the CPU reference of dlwp_conv3x3_wgrad_f32 and the torch form
    tools/bench_conv_wgrad.py times.  hpx_table: the pad-1 table of healpix.device_table (HEALPixPadding), None = CylinderPad."""
    dw = db = None
    if need_weight:
        xcat = x0 if x1 is None else torch.cat([x0, x1], dim=1)
        xa = _ACT_FNS[pre_act](xcat)
        if hpx_table is None:
            xp = F.pad(F.pad(xa, (1, 1, 0, 0), mode="circular"), (0, 0, 1, 1))
        elif xa.is_cuda:
            xp = ops.healpix_pad(xa, 1)
        else:
            xp = _hpx_pad_torch(xa, hpx_table)
        dw = torch.nn.grad.conv2d_weight(xp, (gz.shape[1], xcat.shape[1], 3, 3), gz)
    if need_bias:
        db = gz.sum(dim=(0, 2, 3))
    return dw, db


CONV_WGRAD_MODES = ("auto", "hip", "torch")
# DLWP_CONV_WGRAD=auto: layers of fewer FLOPs than this (2 N H W cin cout 9) keep the torch form.  Value from the per-layer
# table of profiles/conv_wgrad.jsonl (tools/bench_conv_wgrad.py): of the 14 measured layers above it 12
# run 0.97-1.35 x MIOpen's composition on dlwp_conv3x3_wgrad_f32 and two lose (68 -> 272 on 32 x 32 faces 0.72 x, 12 -> 136
# on 64 x 64 faces 0.58 x: narrow sides fill little of a 64 x 64 channel block); of the 53 below it 51 run 0.34-0.93 x, the
# other two 1.26 and 1.12 x.  Whole steps under auto are not slower than torch on any of the seven measured networks
CONV_WGRAD_AUTO_MIN_FLOPS = 40e9


def conv_wgrad_mode() -> str:
    """DLWP_CONV_WGRAD, the one switch of the U-Net family's convolution weight gradients: "hip" every supported one on
    dlwp_conv3x3_wgrad_f32 / dlwp_conv2d_wgrad_f32, "torch" the library compositions conv3x3_weight_grad_torch /
    conv2d_weight_grad_torch, "auto" (default) HIP where it is supported and measured not slower.  Read at every backward."""
    mode = os.environ.get("DLWP_CONV_WGRAD", "auto")
    if mode not in CONV_WGRAD_MODES:
        raise _lib.DlwpError(f"DLWP_CONV_WGRAD={mode!r}: one of {CONV_WGRAD_MODES}")
    return mode


def conv_wgrad_uses_hip(batch: int, c0: int, c1: int, cout: int, h: int, w: int, hpx: bool) -> bool:
    """whether _Conv3x3Fn.backward takes the HIP weight gradient for a layer under the current DLWP_CONV_WGRAD"""
    mode = conv_wgrad_mode()
    if mode == "torch" or (mode == "auto" and 18.0 * batch * h * w * (c0 + c1) * cout < CONV_WGRAD_AUTO_MIN_FLOPS):
        return False                                     # decided without a library call
    return ops.conv3x3_weight_grad_supported(batch, c0, c1, cout, h, w, hpx)


CONV_DGRAD_MODES = ("torch", "hip")


def conv_dgrad_mode() -> str:
    """DLWP_CONV_DGRAD, the one switch of what the U-Net family's training step still sends to a library: the forward and
    input gradient of the non-3x3 convolutions, the AvgPool2d(2) backward and the wide-HEALPix 3x3 input gradient.  "torch"
    (default): the library calls conv2d_torch / conv_transpose2d_torch / conv2d_input_grad_torch, F.avg_pool2d and
    F.conv_transpose2d.  "hip": dlwp_conv2d_mfma_f32 / dlwp_conv_transpose2d_mfma_f32 in the fp32-grade "bf16x6" form,
    dlwp_conv2d_dgrad_mfma_f32 and dlwp_avgpool2x2_bwd_f32 -- bit-reproducible gradients, no algorithm search, no library
    workspace; a geometry the kernels refuse takes the library call.  Read at every call; DLWP_TRAIN_TORCH_BACKWARD=1 wins."""
    mode = os.environ.get("DLWP_CONV_DGRAD", "torch")
    if mode not in CONV_DGRAD_MODES:
        raise _lib.DlwpError(f"DLWP_CONV_DGRAD={mode!r}: one of {CONV_DGRAD_MODES}")
    return mode


def conv_dgrad_uses_hip() -> bool:
    return conv_dgrad_mode() == "hip" and not _torch_backward_selected()


# output channels up to which the HEALPix input gradient runs dlwp_conv3x3_hpx_bwd_data_f32; wider layers take the two-step
# form (MIOpen transposed conv + dlwp_healpix_pad_bwd_f32), which measured faster there
HPX_DX_DIRECT_MAX_COUT = 48


class _Conv3x3Fn(torch.autograd.Function):
    """pad(1) + Conv2d(3x3) with its fusions (CylinderPad, or HEALPixPadding with hpx): dlwp_conv3x3_ex_f32 forward, the
    kernels of _conv3x3_backward backward.  DLWP_TRAIN_TORCH_BACKWARD=1 differentiates conv3x3_torch instead."""

    @staticmethod
    def forward(ctx, x0, x1, weight, bias, resid, pre_act, act, hpx):
        ctx.cfg = (pre_act, act, hpx)
        ctx.save_for_backward(x0, x1, weight, bias, resid)
        with torch.no_grad():
            d = lambda t: t.detach() if t is not None else None
            return ops.conv3x3(d(x0), d(weight), d(bias), act=act, x1=d(x1), pre_act=pre_act, resid=d(resid), hpx=hpx)

    @staticmethod
    def backward(ctx, grad_out):
        if not _torch_backward_selected():
            return (*_conv3x3_backward(ctx, grad_out), None, None, None)
        pre_act, act, hpx = ctx.cfg
        x0 = ctx.saved_tensors[0]
        table = _hpx.device_table(x0.shape[2], x0.shape[3], 1, x0.device) if hpx else None
        return (*_grad_of_torch_form(lambda *a: conv3x3_torch(*a, pre_act, act, table), ctx.saved_tensors,
                                     ctx.needs_input_grad[:5], grad_out), None, None, None)


def conv3x3(x0, weight, bias, act=0, x1=None, pre_act=0, resid=None, hpx=False):
    return _Conv3x3Fn.apply(x0, x1, weight, bias, resid, pre_act, act, hpx)


def conv2d_torch(x, weight, bias, resid, stride: int, padding: int, pre_act: int, act: int):
    """act(Conv2d(pre_act(x)) + resid), zero padding, with torch operators (reference unet.py:450, :583-584, :879)"""
    y = F.conv2d(_ACT_FNS[int(pre_act)](x), weight, bias, stride=stride, padding=padding)
    return _ACT_FNS[int(act)](y if resid is None else y + resid)


def conv_transpose2d_torch(x, weight, bias, stride: int, padding: int, act: int):
    """act(ConvTranspose2d(x)) with torch operators (reference unet.py:523, :719)"""
    return _ACT_FNS[int(act)](F.conv_transpose2d(x, weight, bias, stride=stride, padding=padding))


def conv2d_input_grad_torch(gz, x, weight, stride: int, padding: int, transposed: bool = False):
    """dx of conv2d_torch (transposed: of conv_transpose2d_torch) before the pre-activation's derivative, from gz, the gradient
    of the convolution's output: the library call autograd makes for the plain composition (aten.convolution_backward, input
    alone).  x gives the shape."""
    return torch.ops.aten.convolution_backward(gz, x, weight, None, [stride, stride], [padding, padding], [1, 1],
                                               bool(transposed), [0, 0], 1, [True, False, False])[0]


def _unsupported_is_none(fn):
    """fn(), or None where the library answers DLWP_ERR_UNSUPPORTED (the caller then takes the library call)"""
    try:
        return fn()
    except _lib.DlwpError as e:
        if e.status != _lib.ERR_UNSUPPORTED:
            raise
        return None


def _conv2_forward_hip(x, weight, bias, resid, stride: int, padding: int, pre_act: int, transposed: bool):
    """z = Conv2d(pre_act(x)) + bias + resid (transposed: ConvTranspose2d(x) + bias) on the matrix-pipe kernel in the "bf16x6"
    form, pre-activation, bias and residual inside it, act = 0 so that z itself can be saved; None for a layer it refuses.
    The weight is packed in this call, from the values it holds now (ops._conv_pack): no cached pack can go stale under an
    optimizer that writes through raw pointers, and a captured step re-packs at every replay."""
    if not (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() == 4):
        return None
    lib = _lib.load()
    n, cin, h, w = x.shape
    k = weight.shape[2]
    cout = weight.shape[1] if transposed else weight.shape[0]
    if max(n, cin, cout, h, w, k, stride, padding) >= 1 << 31 or not lib.dlwp_conv2d_mfma_packed_bytes(cout, cin, k) or \
            not lib.dlwp_conv2d_mfma_variant(int(transposed), n, h, w, cout, k, stride, padding):
        return None
    if transposed:
        return _unsupported_is_none(lambda: ops.conv_transpose2d(x, weight, bias, stride, padding, act=0, form="bf16x6",
                                                                 cached=False))
    resid = resid.contiguous() if resid is not None else None
    return _unsupported_is_none(lambda: ops.conv2d(x, weight, bias, stride, padding, pre_act=pre_act, act=0, resid=resid,
                                                   form="bf16x6", cached=False))


def _conv2_input_grad_hip(gz, x_shape, weight, stride: int, padding: int, transposed: bool):
    """the input gradient (before the pre-activation's derivative) on dlwp_conv2d_dgrad_mfma_f32, the transposed layer's on
    dlwp_conv2d_mfma_f32; None for a layer they refuse.  The adjoint pack is made in this call, as the forward's is."""
    if not (gz.is_cuda and gz.dtype == torch.float32 and weight.dtype == torch.float32):
        return None
    n, cin, h, w = x_shape
    k = weight.shape[2]
    if transposed:
        cout = weight.shape[1]
        if not ops.conv_transpose2d_input_grad_supported(n, cin, cout, gz.shape[2], gz.shape[3], k, stride, padding):
            return None
        return _unsupported_is_none(lambda: ops.conv_transpose2d_input_grad(gz, weight, stride, padding, cached=False))
    if not ops.conv2d_input_grad_supported(n, cin, weight.shape[0], h, w, k, stride, padding):
        return None
    return _unsupported_is_none(lambda: ops.conv2d_input_grad(gz, weight, x_shape, stride, padding, cached=False))


def conv2d_weight_grad_torch(x, gz, k: int, stride: int, padding: int, pre_act: int = 0, transposed: bool = False,
                             need_weight: bool = True, need_bias: bool = True):
    """(dW, db) of conv2d_torch (transposed: of conv_transpose2d_torch) from the layer's input x and gz, the gradient of the
    convolution's output, as the composition of library operators: the pre-activated copy of x, the library's convolution
    weight gradient (MIOpen on the GPU) and gz.sum.  On any device: the DLWP_CONV_WGRAD=torch path of _Conv2dFn /
    _ConvTranspose2dFn, the CPU reference of dlwp_conv2d_wgrad_f32 and the torch form tools/bench_conv2_wgrad.py times."""
    dw = db = None
    if need_weight:
        cin, cout = x.shape[1], gz.shape[1]
        shape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
        dw = torch.ops.aten.convolution_backward(gz, _ACT_FNS[int(pre_act)](x), x.new_empty(shape), None, [stride, stride],
                                                 [padding, padding], [1, 1], bool(transposed), [0, 0], 1,
                                                 [False, True, False])[1]
    if need_bias:
        db = gz.sum(dim=(0, 2, 3))
    return dw, db


# DLWP_CONV_WGRAD=auto for the non-3x3 convolutions: layers of fewer FLOPs than this (2 N SH SW cin cout k^2 over the smaller
# map: Conv2d's output, ConvTranspose2d's input) keep the library form.  Infinite: auto takes no layer.  In the per-layer table
# of profiles/conv2_wgrad.jsonl (tools/bench_conv2_wgrad.py) every one of the 12 measured layers of 8
# GFLOP and more runs 0.51-0.99 x MIOpen's composition on dlwp_conv2d_wgrad_f32 (staging-bound: 0.12-0.26 of the fp32 matrix
# peak), and the 10 of the 46 smaller ones that win (1.09-1.57 x) lie between losers of the same size, so no FLOP threshold
# admits winners only; with every layer on the kernel the MUNetHPX steps are 0.6-0.75 % slower than under auto, beyond the
# spread of their repeats.  DLWP_CONV_WGRAD=hip takes every supported layer (bit-reproducible gradients, 4 % less peak memory)
CONV2_WGRAD_AUTO_MIN_FLOPS = float("inf")


def conv2_wgrad_flops(batch: int, cin: int, cout: int, h: int, w: int, k: int, stride: int, padding: int,
                      transposed: bool) -> float:
    """the multiply-adds (times 2) of the weight gradient of a layer on input [batch, cin, h, w]"""
    sh, sw = (h, w) if transposed else ((h + 2 * padding - k) // stride + 1, (w + 2 * padding - k) // stride + 1)
    return 2.0 * batch * sh * sw * cin * cout * k * k


def conv2_wgrad_uses_hip(batch: int, cin: int, cout: int, h: int, w: int, k: int, stride: int, padding: int,
                         transposed: bool) -> bool:
    """whether _Conv2dFn / _ConvTranspose2dFn take dlwp_conv2d_wgrad_f32 for a layer under the current DLWP_CONV_WGRAD"""
    mode = conv_wgrad_mode()
    if mode == "torch" or (mode == "auto" and conv2_wgrad_flops(batch, cin, cout, h, w, k, stride, padding, transposed)
                           < CONV2_WGRAD_AUTO_MIN_FLOPS):
        return False                                     # decided without a library call
    return ops.conv2d_weight_grad_supported(batch, cin, cout, h, w, k, stride, padding, transposed)


def _conv3x3_backward(ctx, grad_out):
    """(dx0, dx1, dw, db, dresid) of _Conv3x3Fn (reference backward: train.py:271 through unet.py:429-555, convlstm.py:82-111).
    The post-activation derivative from z, recomputed by the forward kernel.  The input gradient: under CylinderPad (circular
    in longitude, zeros in latitude) the SAME operator with the weights transposed and flipped, dlwp_conv3x3_ex_f32 again;
    under HEALPixPadding(1) (healpix.py:69-114) dlwp_conv3x3_hpx_bwd_data_f32, the transposed 3x3 folded through the adjoint
    of the padding table, or for wide layers the library's transposed convolution onto the padded face (DLWP_CONV_DGRAD=hip:
    dlwp_conv2d_dgrad_mfma_f32, the input gradient of the unpadded 3x3 on the padded face) folded by
    dlwp_healpix_pad_bwd_f32; then the pre-activation derivative.  The weight and bias gradients in one
    dlwp_conv3x3_wgrad_f32 call on the unpadded segments (DLWP_CONV_WGRAD: or conv3x3_weight_grad_torch, the correlation of a
    padded copy with the output gradient through MIOpen), the residual's gradient gz itself."""
    pre_act, act, hpx = ctx.cfg
    x0, x1, weight, bias, resid = ctx.saved_tensors
    need_x0, need_x1, need_w, need_b, need_r = ctx.needs_input_grad[:5]
    need_x1, need_b, need_r = need_x1 and x1 is not None, need_b and bias is not None, need_r and resid is not None
    n, c0, h, w = x0.shape
    c1 = x1.shape[1] if x1 is not None else 0
    dx0 = dx1 = dw = db = None
    xcat = None             # cat([x0, x1], 1): made at most once, by the first step below that reads it
    with torch.no_grad():
        gz = grad_out.contiguous()
        if act != 0:
            z = ops.conv3x3(x0, weight, bias, act=0, x1=x1, pre_act=pre_act, resid=resid, hpx=hpx)
            gz = _act_backward(z, gz, act).contiguous()
        if need_x0 or need_x1:
            if hpx and weight.shape[0] <= HPX_DX_DIRECT_MAX_COUT:
                dxa = ops.conv3x3_hpx_backward_data(gz, weight, c0 + c1)
            elif hpx:
                padded = None
                if conv_dgrad_uses_hip():
                    padded = _conv2_input_grad_hip(gz, (n, c0 + c1, h + 2, w + 2), weight, 1, 0, False)     # onto the padded face
                dxa = ops.healpix_pad_backward(F.conv_transpose2d(gz, weight) if padded is None else padded, 1)
                del padded              # the padded face is the largest tensor of this backward: not kept through the rest
            else:
                dxa = ops.conv3x3(gz, weight.flip(2, 3).transpose(0, 1).contiguous(), None)
            if pre_act != 0:
                xcat = x0 if x1 is None else torch.cat([x0, x1], dim=1)
                dxa = _act_backward(xcat, dxa, pre_act)
            dx0 = dxa[:, :c0].contiguous() if need_x0 else None
            dx1 = dxa[:, c0:].contiguous() if need_x1 else None
        if need_w or need_b:
            if conv_wgrad_uses_hip(n, c0, c1, weight.shape[0], h, w, hpx):
                dw, db = ops.conv3x3_weight_grad(x0, x1, gz, pre_act=pre_act, hpx=hpx, need_bias=need_b)
            else:
                table = _hpx.device_table(h, w, 1, x0.device) if hpx else None
                segments = (x0, x1) if xcat is None else (xcat, None)       # two segments it joins itself, where it reads them
                dw, db = conv3x3_weight_grad_torch(*segments, gz, pre_act, table, need_weight=need_w, need_bias=need_b)
    return dx0, dx1, (dw if need_w else None), (db if need_b else None), (gz if need_r else None)


def _conv2_backward(ctx, grad_out, transposed: bool):
    """(dx, dw, db, dresid) of _Conv2dFn / _ConvTranspose2dFn: the post-activation derivative from the saved z, the input
    gradient by the library call autograd makes for the plain composition (conv2d_input_grad_torch; DLWP_CONV_DGRAD=hip:
    dlwp_conv2d_dgrad_mfma_f32, the transposed layer's dlwp_conv2d_mfma_f32, where they take the layer) followed by
    the pre-activation derivative, the weight and bias gradients in one dlwp_conv2d_wgrad_f32 call on x as it lies
    (DLWP_CONV_WGRAD: or conv2d_weight_grad_torch), the residual's gradient gz itself."""
    stride, padding, pre_act, act = ctx.cfg
    x, weight, bias, resid, z = ctx.saved_tensors
    need_x, need_w, need_b = ctx.needs_input_grad[:3]
    need_b = need_b and bias is not None
    need_r = not transposed and resid is not None and ctx.needs_input_grad[3]
    k = weight.shape[2]
    dx = dw = db = None
    with torch.no_grad():
        gz = _act_backward(z, grad_out.contiguous(), act).contiguous()
        if need_x:
            dxa = _conv2_input_grad_hip(gz, x.shape, weight, stride, padding, transposed) if conv_dgrad_uses_hip() else None
            if dxa is None:
                dxa = conv2d_input_grad_torch(gz, x, weight, stride, padding, transposed)
            dx = _act_backward(x, dxa, pre_act)
        if need_w or need_b:
            n, cin, h, w = x.shape
            cout = weight.shape[1] if transposed else weight.shape[0]
            if conv2_wgrad_uses_hip(n, cin, cout, h, w, k, stride, padding, transposed):
                dw, db = ops.conv2d_weight_grad(x, gz, k, stride, padding, pre_act=pre_act, transposed=transposed,
                                                need_weight=need_w, need_bias=need_b)
            else:
                dw, db = conv2d_weight_grad_torch(x, gz, k, stride, padding, pre_act, transposed, need_weight=need_w,
                                                  need_bias=need_b)
    return dx, dw, db, (gz if need_r else None)


class _Conv2dFn(torch.autograd.Function):
    """ops.conv2d under autograd: the forward is conv2d_torch's operators (values bit for bit the plain composition's), under
    DLWP_CONV_DGRAD=hip dlwp_conv2d_mfma_f32 ("bf16x6") followed by training.activation's kernel; saved are x, weight, bias,
    resid and -- only with a post-activation -- the convolution's output z.  Backward: _conv2_backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, resid, stride, padding, pre_act, act):
        ctx.cfg = (stride, padding, pre_act, act)
        with torch.no_grad():
            z = _conv2_forward_hip(x, weight, bias, resid, stride, padding, pre_act, False) if conv_dgrad_uses_hip() else None
            y = None
            if z is None:
                z = conv2d_torch(x, weight, bias, resid, stride, padding, pre_act, 0)
                y = _ACT_FNS[act](z)
            ctx.save_for_backward(x, weight, bias, resid, z if act != 0 else None)
            return y if y is not None else (z if act == 0 else activation(z, act))

    @staticmethod
    def backward(ctx, grad_out):
        return (*_conv2_backward(ctx, grad_out, False), None, None, None, None)


class _ConvTranspose2dFn(torch.autograd.Function):
    """ops.conv_transpose2d under autograd, as _Conv2dFn (no pre-activation, no residual)"""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, act):
        ctx.cfg = (stride, padding, 0, act)
        with torch.no_grad():
            z = _conv2_forward_hip(x, weight, bias, None, stride, padding, 0, True) if conv_dgrad_uses_hip() else None
            y = None
            if z is None:
                z = conv_transpose2d_torch(x, weight, bias, stride, padding, 0)
                y = _ACT_FNS[act](z)
            ctx.save_for_backward(x, weight, bias, None, z if act != 0 else None)
            return y if y is not None else (z if act == 0 else activation(z, act))

    @staticmethod
    def backward(ctx, grad_out):
        return (*_conv2_backward(ctx, grad_out, True)[:3], None, None, None)


def _plain_conv2(weight) -> bool:
    """the cases that keep the plain composition under autograd: the cross-check setting and kernels that are not square"""
    return _torch_backward_selected() or weight.dim() != 4 or weight.shape[2] != weight.shape[3]


def conv2d(x, weight, bias, resid, stride: int, padding: int, pre_act: int, act: int):
    if _plain_conv2(weight):
        return conv2d_torch(x, weight, bias, resid, stride, padding, pre_act, act)
    return _Conv2dFn.apply(x, weight, bias, resid, stride, padding, pre_act, act)


def conv_transpose2d(x, weight, bias, stride: int, padding: int, act: int):
    if _plain_conv2(weight):
        return conv_transpose2d_torch(x, weight, bias, stride, padding, act)
    return _ConvTranspose2dFn.apply(x, weight, bias, stride, padding, act)


class _AvgPool2x2Fn(torch.autograd.Function):
    """AvgPool2d(2) with HIP in both directions: dlwp_avgpool2x2_f32 forward, dlwp_avgpool2x2_bwd_f32 backward"""

    @staticmethod
    def forward(ctx, x):
        ctx.hw = tuple(x.shape[2:])
        with torch.no_grad():
            return ops.avgpool2x2(x.detach())

    @staticmethod
    def backward(ctx, grad_out):
        return ops.avgpool2x2_backward(grad_out, *ctx.hw)


def avgpool2x2(x):
    return _AvgPool2x2Fn.apply(x)


def convlstm_gates_torch(gates, c_prev):
    """The ConvLSTM cell update (reference convlstm.py:96-109) with torch operators, on any device and dtype: (h, c) from
    gates [B, 4*hid, H, W] = (netin, i, f, o) before their activations and c_prev [B, hid, H, W]."""
    netin, ig, fg, og = torch.split(gates, gates.shape[1] // 4, dim=1)
    c_new = torch.sigmoid(fg) * c_prev + torch.sigmoid(ig) * torch.tanh(netin)
    return torch.sigmoid(og) * torch.tanh(c_new), c_new


def convlstm_gates_backward_torch(gates, c_prev, dh, dc):
    """The backward of convlstm_gates_torch from its inputs alone, as plain torch operators on any device and dtype: what
    dlwp_convlstm_gates_bwd_f32 computes (csrc/convlstm_cell.hpp), term by term.  dh, dc: the gradients of h and c, either
    None (zero).

        si, sf, so = sigma(i), sigma(f), sigma(o)      tn = tanh(netin)     c = sf c_prev + si tn     tc = tanh(c)
        dct      = dc + dh so (1 - tc^2)
        d_o      = dh tc so (1 - so)          d_f = dct c_prev sf (1 - sf)
        d_i      = dct tn si (1 - si)         d_netin = dct si (1 - tn^2)
        dc_prev  = dct sf

    Returns (dgates in the gate order of `gates`, dc_prev)."""
    if dh is None and dc is None:
        raise _lib.DlwpError("convlstm_gates_backward_torch: neither dh nor dc given")
    netin, ig, fg, og = torch.split(gates, gates.shape[1] // 4, dim=1)
    dh = torch.zeros_like(c_prev) if dh is None else dh
    dc = torch.zeros_like(c_prev) if dc is None else dc
    si, sf, so, tn = torch.sigmoid(ig), torch.sigmoid(fg), torch.sigmoid(og), torch.tanh(netin)
    tc = torch.tanh(sf * c_prev + si * tn)
    dct = dc + dh * so * (1.0 - tc * tc)
    d_o = dh * tc * so * (1.0 - so)
    d_f = dct * c_prev * sf * (1.0 - sf)
    d_i = dct * tn * si * (1.0 - si)
    d_n = dct * si * (1.0 - tn * tn)
    return torch.cat([d_n, d_i, d_f, d_o], dim=1), dct * sf


class _ConvLstmGatesFn(torch.autograd.Function):
    """The ConvLSTM cell update on HIP in both directions: dlwp_convlstm_gates_f32 (the inference kernel: h and c bit for bit
    what eval() computes) and dlwp_convlstm_gates_bwd_f32.  Saved for the backward: gates and c_prev, the forward's inputs --
    no activated plane (the torch chain keeps six per cell and frame).  A gradient autograd does not have (the last frame's
    c) stays None and reaches the kernel as a null pointer; dc_prev is not computed where c_prev takes no gradient (the first
    frame's state is a constant zero)."""

    @staticmethod
    def forward(ctx, gates, c_prev):
        gates, c_prev = gates.contiguous(), c_prev.contiguous()
        ctx.save_for_backward(gates, c_prev)
        ctx.set_materialize_grads(False)
        with torch.no_grad():
            return ops.convlstm_gates(gates.detach(), c_prev.detach())

    @staticmethod
    @once_differentiable
    def backward(ctx, dh, dc):
        gates, c_prev = ctx.saved_tensors
        need_g, need_c = ctx.needs_input_grad
        if (dh is None and dc is None) or not (need_g or need_c):
            return None, None
        dgates, dc_prev = ops.convlstm_gates_backward(gates, c_prev, dh, dc, need_c_prev=need_c)
        return (dgates if need_g else None), dc_prev


def convlstm_gates(gates, c_prev):
    """differentiable ConvLSTM cell update (h, c): HIP forward and HIP backward; under DLWP_TRAIN_TORCH_BACKWARD=1, and for
    tensors that are not fp32 on the GPU, convlstm_gates_torch, left to autograd"""
    if _torch_backward_selected() or not (gates.is_cuda and gates.dtype == torch.float32 and c_prev.dtype == torch.float32):
        return convlstm_gates_torch(gates, c_prev)
    return _ConvLstmGatesFn.apply(gates, c_prev)


def groupnorm_act_backward_torch(x, mean, rstd, gamma, beta, gy, groups: int, act: int):
    """The backward of y = act(GroupNorm(groups)(x)) (reference unet.py:739 + :761, :887-888 under train.py:271) from x and
    the forward's statistics alone, as plain torch operators on any device: what dlwp_groupnorm_act_bwd_f32 computes
    (csrc/groupnorm_bwd.hip), term by term.  x, gy [N, C, *]; mean, rstd [N, groups]; gamma, beta [C] or None.

        xh = (x - mean) rstd      v = xh gamma_c + beta_c      gv = gy act'(v)      E = (C / groups) HW
        s1[n,c] = sum_hw gv       s2[n,c] = sum_hw gv xh       dbeta_c = sum_n s1   dgamma_c = sum_n s2
        a[n,g] = sum_{c in g} gamma_c s1 / E                   b[n,g] = sum_{c in g} gamma_c s2 / E
        dx = rstd (gv gamma_c - a - xh b)

    Returns (dx, dgamma, dbeta); the last two are the sums s2, s1 over n whether or not gamma / beta exist."""
    n, c = x.shape[0], x.shape[1]
    cpg = c // groups
    x4 = x.reshape(n, groups, cpg, -1)
    e = cpg * x4.shape[-1]
    mean, rstd = mean.reshape(n, groups, 1, 1), rstd.reshape(n, groups, 1, 1)
    gm = gamma.reshape(1, groups, cpg, 1) if gamma is not None else torch.ones(1, 1, 1, 1, dtype=x.dtype, device=x.device)
    bt = beta.reshape(1, groups, cpg, 1) if beta is not None else torch.zeros(1, 1, 1, 1, dtype=x.dtype, device=x.device)
    xh = (x4 - mean) * rstd
    gv = gy.reshape(x4.shape) * _act_grad_torch(xh * gm + bt, int(act))
    s1 = gv.sum(dim=3, keepdim=True)
    s2 = (gv * xh).sum(dim=3, keepdim=True)
    a = (gm * s1).sum(dim=2, keepdim=True) / e
    b = (gm * s2).sum(dim=2, keepdim=True) / e
    dx = rstd * (gv * gm - a - xh * b)
    return dx.reshape(x.shape), s2.sum(dim=0).reshape(c), s1.sum(dim=0).reshape(c)


class _GroupNormActFn(torch.autograd.Function):
    """y = act(GroupNorm(groups)(x)) on HIP in both directions: dlwp_groupnorm_act_fwd_stats_f32 (the inference kernel, y bit
    for bit, which also writes mean and rstd per (sample, group)) and dlwp_groupnorm_act_bwd_f32.  Saved for the backward: x,
    the statistics and gamma / beta -- no normalised or activated copy of x."""

    @staticmethod
    def forward(ctx, x, weight, bias, groups, eps, act):
        x = x.contiguous()
        d = lambda t: t.detach() if t is not None else None
        with torch.no_grad():
            y, stats = ops.groupnorm_act_fwd_stats(x.detach(), d(weight), d(bias), groups, eps, act)
        ctx.cfg = (groups, act, weight is not None, bias is not None)
        ctx.save_for_backward(x, stats, *[t for t in (weight, bias) if t is not None])
        return y

    @staticmethod
    def backward(ctx, grad_out):
        groups, act, has_w, has_b = ctx.cfg
        x, stats, *wb = ctx.saved_tensors
        weight = wb.pop(0) if has_w else None
        bias = wb.pop(0) if has_b else None
        need_x, need_w, need_b = ctx.needs_input_grad[0], has_w and ctx.needs_input_grad[1], has_b and ctx.needs_input_grad[2]
        dx = dw = db = None
        if need_x or need_w or need_b:
            with torch.no_grad():
                dx, dw, db = ops.groupnorm_act_backward(x, stats, weight, bias, grad_out.contiguous(), groups, act,
                                                        need_x, need_w, need_b)
        return dx, dw, db, None, None, None


def groupnorm_act(x, weight, bias, groups: int, eps: float = 1e-5, act: int = 0):
    """differentiable act(GroupNorm(groups)(x)) for x [N, C, *]: HIP forward and HIP backward; under
    DLWP_TRAIN_TORCH_BACKWARD=1 the library's group_norm and activation, left to autograd"""
    if _torch_backward_selected():
        return _ACT_FNS[int(act)](F.group_norm(x, int(groups), weight, bias, eps))
    return _GroupNormActFn.apply(x, weight, bias, int(groups), float(eps), int(act))


def layernorm_backward_torch(x, gamma, gy, eps: float):
    """The backward of y = LayerNorm(x) gamma + beta over the last dimension (reference fourcastnet.py:180-193,
    swin_transformer.py:213,262, panguweather.py:281,321 under train.py:271) from x and gamma alone, as plain torch operators on
    any device: what dlwp_layernorm_bwd_f32 computes (csrc/layernorm_bwd.hip), term by term.  x, gy [..., C]; gamma [C].

        mean, rstd: two-pass, biased variance      xh = (x - mean) rstd      g = gy gamma
        a = mean_C(g)      b = mean_C(g xh)        dx = rstd (g - a - xh b)
        dgamma_c = sum_rows gy xh                  dbeta_c = sum_rows gy

    Returns (dx, dgamma, dbeta)."""
    c = x.shape[-1]
    x2, gy2 = x.reshape(-1, c), gy.reshape(-1, c)
    mean = x2.mean(dim=1, keepdim=True)
    rstd = torch.rsqrt(((x2 - mean) ** 2).mean(dim=1, keepdim=True) + eps)
    xh = (x2 - mean) * rstd
    g = gy2 * gamma.reshape(1, c)
    a = g.mean(dim=1, keepdim=True)
    b = (g * xh).mean(dim=1, keepdim=True)
    dx = rstd * (g - a - xh * b)
    return dx.reshape(x.shape), (gy2 * xh).sum(dim=0), gy2.sum(dim=0)


class _LayerNormFn(torch.autograd.Function):
    """y = LayerNorm(x) gamma + beta over the last dimension on HIP in both directions: dlwp_layernorm_prebias_f32 (the
    inference kernel, y bit for bit) and dlwp_layernorm_bwd_f32.  Saved for the backward: x and gamma -- no statistics, no
    normalised copy of x (the kernel recomputes mean and rstd with the forward's arithmetic)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x = x.contiguous()
        with torch.no_grad():
            y = ops.layer_norm(x.detach(), weight.detach(), bias.detach(), eps)
        ctx.eps = eps
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        """HIP backward; DLWP_ERR_UNSUPPORTED (a tensor that is not 16-byte aligned) and DLWP_TRAIN_TORCH_BACKWARD=1
        evaluate layernorm_backward_torch; any other error raises."""
        x, weight = ctx.saved_tensors
        needs = ctx.needs_input_grad[:3]
        if not any(needs):
            return None, None, None, None
        with torch.no_grad():
            gy = grad_out.contiguous()
            grads = None
            if not _torch_backward_selected():
                try:
                    grads = ops.layernorm_backward(x, weight, gy, ctx.eps, *needs)
                except _lib.DlwpError as e:
                    if e.status != _lib.ERR_UNSUPPORTED:
                        raise
            if grads is None:
                grads = layernorm_backward_torch(x, weight, gy, ctx.eps)
        return (*[g if need else None for g, need in zip(grads, needs)], None)


def layer_norm(x, weight, bias, eps: float = 1e-5):
    """differentiable LayerNorm over the last dimension: HIP forward and HIP backward; under DLWP_TRAIN_TORCH_BACKWARD=1 the
    library's layer_norm, left to autograd"""
    if _torch_backward_selected():
        return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)
    return _LayerNormFn.apply(x, weight, bias, float(eps))


def bias_act_backward_torch(gy, z, act: int):
    """The pointwise part of the backward of y = act(z) + resid, z = x W^T + b, as plain torch operators on any device: what
    dlwp_bias_act_bwd_f32 computes (csrc/bias_act.hip), term by term.  gy, z [..., N] (z unused for act 0).
    Returns (gz, db): gz = gy act'(z) in the closed form of _act_grad_torch, db_n = sum_rows gz."""
    gz = gy * _act_grad_torch(z, int(act)) if int(act) != 0 else gy
    return gz, gz.reshape(-1, gz.shape[-1]).sum(dim=0)


class _ActFn(torch.autograd.Function):
    """h = act(z) on dlwp_act_f32 forward and dlwp_bias_act_bwd_f32 backward (saved: z): the activation of a Linear whose
    GEMMs the HIP kernel does not take, so that its GELU is still the one inference evaluates."""

    @staticmethod
    def forward(ctx, z, act):
        z = z.contiguous()
        ctx.act = int(act)
        ctx.save_for_backward(z)
        with torch.no_grad():
            return ops.activation(z.detach(), ctx.act)

    @staticmethod
    def backward(ctx, gy):
        z, = ctx.saved_tensors
        with torch.no_grad():
            gy = gy.contiguous()
            try:
                return ops.bias_act_backward(gy, z, ctx.act, False)[0], None
            except _lib.DlwpError as e:
                if e.status != _lib.ERR_UNSUPPORTED:
                    raise
            return bias_act_backward_torch(gy, z, ctx.act)[0], None


def activation(z, act: int):
    """differentiable act(z) for a fp32 GPU tensor of a multiple of 4 values: HIP forward and HIP backward; anything else,
    and everything under DLWP_TRAIN_TORCH_BACKWARD=1, the library's activation, left to autograd"""
    if _torch_backward_selected() or not z.is_cuda or z.dtype != torch.float32 or z.numel() % 4 or z.numel() == 0:
        return _ACT_FNS[int(act)](z)
    return _ActFn.apply(z, int(act))


class _LinearFn(torch.autograd.Function):
    """y = act(x W^T + b) + resid with the HIP Linear kernel in BOTH directions (reference backward: scripts/train.py:271
    through the nn.Linear layers of swin_transformer.py:21-39, :107-120 and panguweather.py:176-211): the fp32-accurate GEMM of
    csrc/linear.hip (bf16x6) computes the output, the input gradient dX = dZ W (the same kernel on the transposed weight) and
    the weight gradient dW = dZ^T X (the same kernel with dZ^T as the activation and X^T as the "weight"; the reduction runs
    over the tokens).  Without an activation the bias and the residual ride in the GEMM epilogue, one launch, bit-equal to
    inference; with one the GEMM stores z = x W^T + b, which the backward needs, and dlwp_act_f32 applies the epilogue's own
    activation to it (saved: x, W and z).  The backward first takes dZ = dY act'(z) and the bias gradient, the column sum of
    dZ, in one pass (dlwp_bias_act_bwd_f32); the gradient of resid is dY itself.  Shapes the kernel does not take (in / out
    features not multiples of 32 / 4 in the roles they play in the three products) use the torch operator."""

    @staticmethod
    def supported(rows: int, k: int, n: int) -> bool:
        return (ops.linear_supported(k, n) and ops.linear_supported(n, k) and ops.linear_supported(rows, k) and
                not _torch_backward_selected())

    @staticmethod
    def forward(ctx, x, weight, bias, act=0, resid=None):
        d = lambda t: t.detach() if t is not None else None
        ctx.has_bias, ctx.act = bias is not None, int(act)
        with torch.no_grad():
            if ctx.act == 0:
                ctx.save_for_backward(x, weight)
                return ops.linear_raw(d(x), d(weight), d(bias), resid=d(resid).contiguous() if resid is not None else None)
            z = ops.linear_raw(d(x), d(weight), d(bias))
            ctx.save_for_backward(x, weight, z)
            y = ops.activation(z, ctx.act)
            return y if resid is None else y.add_(d(resid))

    @staticmethod
    def backward(ctx, gy):
        x, weight, *z = ctx.saved_tensors
        n, k = weight.shape
        gy2 = gy.reshape(-1, n).contiguous()
        x2 = x.reshape(-1, k)
        gx = gw = gb = None
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        with torch.no_grad():
            gz = gy2
            if ctx.act != 0 or need_b:
                z2 = z[0].reshape(-1, n) if z else None
                try:
                    gz, gb = ops.bias_act_backward(gy2, z2, ctx.act, need_b)
                except _lib.DlwpError as e:
                    if e.status != _lib.ERR_UNSUPPORTED:      # a grad_out that is not 16-byte aligned: the torch form
                        raise
                    gz, gb = bias_act_backward_torch(gy2, z2, ctx.act)
                    gb = gb if need_b else None
            if ctx.needs_input_grad[0]:
                gx = ops.linear_raw(gz, weight.t().contiguous(), None).view(x.shape)          # [M, N] x [K, N]^T
            if ctx.needs_input_grad[1]:
                gw = ops.linear_raw(gz.t().contiguous(), x2.t().contiguous(), None)             # [N, M] x [K, M]^T -> [N, K]
        return gx, gw, gb, None, gy if ctx.needs_input_grad[4] else None


def linear_fn(x, weight, bias, act: int = 0, resid=None):
    return _LinearFn.apply(x, weight, bias, int(act), resid)


def wants_grad(*tensors) -> bool:
    """True when autograd is recording and one of the tensors takes part: the ops then run their differentiable form."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


# ---- MeshGraphNet (models/mgn.py; csrc/mgn.hip forward, csrc/mgn_bwd.hip backward) -------------------------------------
def _mgn_rows(x: torch.Tensor, batch: int, rows: int, channels_first: bool) -> torch.Tensor:
    """[batch, C, rows...] channels-first or [batch * rows, C] -> [batch * rows, C] (the torch composition's row view)"""
    if not channels_first:
        return x.reshape(batch * rows, -1)
    return x.reshape(batch, -1, rows).permute(0, 2, 1).reshape(batch * rows, -1)


def mgn_mlp_backward_torch(seq, x, grad_out, batch: int, rows: int, channels_first_in: bool, channels_first_out: bool,
                           need_input_grad: bool):
    """the backward of one MeshGraphMLP by autograd of the torch composition (DLWP_TRAIN_TORCH_BACKWARD=1): (grad_x or None,
    [gradients in the order of seq.parameters()])"""
    def form(x_):
        y = ops.mgn_mlp_torch(seq, _mgn_rows(x_, batch, rows, channels_first_in))
        return y.view(batch, rows, -1).permute(0, 2, 1) if channels_first_out else y

    gx, *gp = _grad_of_torch_form(form, (x,), (need_input_grad,), grad_out, params=list(seq.parameters()))
    return gx, gp


class _MgnMlpFn(torch.autograd.Function):
    """One MeshGraphMLP: dlwp_mgn_mlp_f32 forward, dlwp_mgn_mlp_bwd_f32 backward (recomputes the forward from x; only x is
    saved).  DLWP_TRAIN_TORCH_BACKWARD=1 differentiates the torch composition instead."""

    @staticmethod
    def forward(ctx, x, seq, packed, batch, rows, channels_first_in, channels_first_out, *params):
        with torch.no_grad():
            y = ops.mgn_mlp(packed, seq, x.detach(), batch, rows, channels_first_in, channels_first_out)
        ctx.save_for_backward(x, *params)         # the parameters too: autograd's version check sees in-place edits
        ctx.cfg = (seq, packed, batch, rows, channels_first_in, channels_first_out)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        x = ctx.saved_tensors[0]
        seq, packed, batch, rows, cf_in, cf_out = ctx.cfg
        need_x = ctx.needs_input_grad[0]
        if _torch_backward_selected():
            gx, gp = mgn_mlp_backward_torch(seq, x, grad_out, batch, rows, cf_in, cf_out, need_x)
        else:
            gx, gp = ops.mgn_mlp_backward(packed, seq, x, grad_out, batch, rows, cf_in, cf_out, need_x)
        if gx is not None:
            gx = gx.view(x.shape)
        return (gx, None, None, None, None, None, None, *gp)


def mgn_mlp(seq, packed, x, batch: int, rows: int, channels_first_in: bool = False, channels_first_out: bool = False):
    """differentiable MeshGraphMLP (ops.mgn_mlp layouts): HIP forward and HIP backward"""
    return _MgnMlpFn.apply(x, seq, packed, batch, rows, channels_first_in, channels_first_out, *seq.parameters())


def mgn_layer_backward_torch(edge_seq, node_seq, aggregation, graph, batch: int, x, e, dx_out, de_out):
    """the backward of one processor layer by autograd of ops.mgn_layer_torch (DLWP_TRAIN_TORCH_BACKWARD=1): (dx, de,
    [edge MLP gradients], [node MLP gradients])"""
    _, src, dst, deg = graph[:4]
    pe, pn = list(edge_seq.parameters()), list(node_seq.parameters())
    form = lambda x_, e_: ops.mgn_layer_torch(edge_seq, node_seq, aggregation, src, dst, deg, batch, x_, e_)
    dx, de, *gp = _grad_of_torch_form(form, (x, e), (True, True), (dx_out, de_out), params=pe + pn, zero_fill=True)
    return dx, de, gp[:len(pe)], gp[len(pe):]


class _MgnLayerFn(torch.autograd.Function):
    """One processor layer: dlwp_mgn_processor_layer_f32 forward into FRESH x' / e' (they are the next layer's saved
    inputs), dlwp_mgn_processor_layer_bwd_f32 backward from the saved inputs x, e.  de' is None for a layer whose e'
    nothing reads (the last of a message-passing step).  DLWP_TRAIN_TORCH_BACKWARD=1 differentiates ops.mgn_layer_torch."""

    @staticmethod
    def forward(ctx, x, e, e_shared, cfg, *params):
        edge_seq, edge_packed, node_seq, node_packed, aggregation, graph, batch = cfg
        row_ptr, src, dst = graph[0], graph[1], graph[2]
        d = x.shape[1]
        with torch.no_grad():
            x_out = torch.empty_like(x)
            e_out = torch.empty(batch * src.numel(), d, device=x.device, dtype=torch.float32)
            ops.mgn_processor_layer(edge_packed, edge_seq, node_packed, node_seq, aggregation, row_ptr, src, dst, batch,
                                    x.detach(), x_out, e.detach(), e_shared, e_out)
        ctx.save_for_backward(x, e, *params)      # the parameters too: autograd's version check sees in-place edits
        ctx.cfg, ctx.e_shared = cfg, e_shared
        ctx.set_materialize_grads(False)
        return x_out, e_out

    @staticmethod
    def backward(ctx, dx_out, de_out):
        x, e = ctx.saved_tensors[:2]
        edge_seq, edge_packed, node_seq, node_packed, aggregation, graph, batch = ctx.cfg
        if _torch_backward_selected():
            dx, de, ge, gn = mgn_layer_backward_torch(edge_seq, node_seq, aggregation, graph, batch, x, e, dx_out, de_out)
        else:
            if dx_out is None:
                dx_out = torch.zeros_like(x)
            row_ptr, src, dst, _, src_row_ptr, src_perm = graph
            dx, de, ge, gn = ops.mgn_processor_layer_backward(edge_packed, edge_seq, node_packed, node_seq, aggregation,
                                                              row_ptr, src, dst, src_row_ptr, src_perm, batch, x, e,
                                                              ctx.e_shared, dx_out, de_out)
        return (dx if ctx.needs_input_grad[0] else None, de if ctx.needs_input_grad[1] else None, None, None, *ge, *gn)


def mgn_layer(edge_seq, edge_packed, node_seq, node_packed, aggregation: str, graph, batch: int, x, e, e_shared: bool):
    """differentiable processor layer on [batch * N, D] nodes and [batch * E, D] (or shared [E, D]) edges: (x', e').
    graph = (row_ptr, src, dst, deg, src_row_ptr, src_perm): the CSC graph, its in-degrees and the CSR by source
    (ops.mgn_source_csr)"""
    cfg = (edge_seq, edge_packed, node_seq, node_packed, aggregation, graph, batch)
    return _MgnLayerFn.apply(x, e, e_shared, cfg, *edge_seq.parameters(), *node_seq.parameters())


# ---- GraphCastNet (models/graphcast.py; csrc/graphcast.hip forward, csrc/graphcast_bwd.hip backward) --------------------
def _gc_tail_backward(seq, batch: int, rows: int, zs, gy, out_cf: bool, ln_gather: Optional[dict] = None,
                      want_total: bool = False):
    """the backward of a MeshGraphMLP above its first Linear from the saved pre-activations zs: (dZ_0 [batch * rows, H],
    the LayerNorm's total output gradient or None, [gradients in the order of seq.parameters(), the first Linear's None])"""
    lins, ln = ops.mgn_parts(seq)
    act = ops.GC_ACT[type(seq[1])]
    n = len(lins)
    grads = [None] * (2 * n + (2 if ln is not None else 0))
    g_total = None
    g, cf = gy, out_cf
    if ln is not None:
        g_total, g, grads[2 * n], grads[2 * n + 1] = ops.gc_layernorm_backward(zs[-1], ln, batch, rows, gy,
                                                                              want_total=want_total, **(ln_gather or {}))
        cf = False
    for i in range(n - 1, 0, -1):
        l = lins[i]
        grads[2 * i], grads[2 * i + 1] = ops.gc_weight_grad(
            dict(a_mode=0, a=zs[i - 1], a_batch_stride=rows * l.in_features, lda=l.in_features, a_act=act),
            l.in_features, l.out_features, batch, rows, g, dz_cf=cf)
        g = ops.gc_data_grad(g, l.weight.detach(), batch, rows, dz_cf=cf, z=zs[i - 1], act=act)
        cf = False
    return g, g_total, grads


def _gc_batch_sum(t: torch.Tensor, batch: int) -> torch.Tensor:
    """the fixed-order sum over the batch of [batch * rows, D] (the gradient of a table the batch shares)"""
    if batch == 1:
        return t
    return ops.gc_segment_sum(t, batch, None, None, t.shape[0] // batch, batch_sum=True)


def gc_mlp_torch(seq, x, batch: int, rows: int, mode: int = 0, x_bs: Optional[int] = None, residual: bool = False,
                 out_cf: bool = False, col_order=None):
    """torch composition of one GraphCast MLP in the layouts of gc_mlp (GraphCastNet's composition,
    DLWP_TRAIN_TORCH_BACKWARD=1, tests)"""
    if mode == 1:
        a = x.reshape(batch, -1, rows)
        if col_order is not None:
            a = a[:, col_order]
        a = a.permute(0, 2, 1).reshape(batch * rows, -1)
    else:
        a = x.repeat(batch, 1) if x_bs == 0 and batch > 1 else x
    y = seq(a)
    if residual:
        y = y + a
    if out_cf:
        y = y.view(batch, rows, -1).permute(0, 2, 1)
    return y


class _GcMlpFn(torch.autograd.Function):
    """One GraphCast MeshGraphMLP (A modes 0 / 1, optional LayerNorm, residual and channels-first output): forward on
    dlwp_gc_linear_f32 saving the input (a reference), each pre-activation z_i and the LayerNorm input; backward on
    csrc/graphcast_bwd.hip.  DLWP_TRAIN_TORCH_BACKWARD=1 differentiates gc_mlp_torch instead."""

    @staticmethod
    def forward(ctx, x, cfg, *params):
        seq, pk, batch, rows, mode, x_bs, residual, out_cf, col_order = cfg
        with torch.no_grad():
            xd = x.detach()
            y, zs = ops.gc_mlp(pk, seq, batch, rows, ops.gc_a_fields(mode, xd, x_bs), res=xd if residual else None,
                               res_bs=x_bs, out_cf=out_cf, save=True)
        ctx.save_for_backward(x, *zs, *params)    # the parameters too: autograd's version check sees in-place edits
        ctx.cfg, ctx.n_z = cfg, len(zs)
        return y

    @staticmethod
    def backward(ctx, gy):
        seq, pk, batch, rows, mode, x_bs, residual, out_cf, col_order = ctx.cfg
        saved = ctx.saved_tensors
        x, zs = saved[0], saved[1:1 + ctx.n_z]
        need_x = ctx.needs_input_grad[0]
        if _torch_backward_selected():
            form = lambda x_: gc_mlp_torch(seq, x_, batch, rows, mode, x_bs, residual, out_cf, col_order)
            gx, *gp = _grad_of_torch_form(form, (x,), (need_x,), gy, params=list(seq.parameters()))
            return (gx, None, *gp)
        gy = gy.contiguous()
        lins, _ = ops.mgn_parts(seq)
        g0, _, grads = _gc_tail_backward(seq, batch, rows, zs, gy, out_cf)
        l0 = lins[0]
        dw, grads[1] = ops.gc_weight_grad(ops.gc_a_fields(mode, x, x_bs), l0.in_features, l0.out_features, batch, rows, g0)
        grads[0] = dw[:, col_order] if col_order is not None else dw
        gx = None
        if need_x:
            w0 = pk.backward_first(seq)[0]
            res = gy if residual else None
            gx = ops.gc_data_grad(g0, w0, batch, rows, res=res, res_bs=rows * l0.in_features, out_cf=mode == 1)
            if mode == 0 and not x_bs:
                gx = _gc_batch_sum(gx, batch)
            gx = gx.view(x.shape)
        return (gx, None, *grads)


def gc_mlp(seq, pk, x, batch: int, rows: int, mode: int = 0, x_bs: Optional[int] = None, residual: bool = False,
           out_cf: bool = False, col_order=None):
    """differentiable GraphCast MLP: x [batch * rows, D] rows (x_bs 0: one [rows, D] table shared by the batch) or, mode 1,
    channels-first [batch, C, rows...] whose weight-gradient columns are put back in torch's order by col_order"""
    if x_bs is None:
        x_bs = rows * x.shape[-1] if mode == 0 else x.numel() // batch
    cfg = (seq, pk, batch, rows, mode, x_bs, residual, out_cf, col_order)
    return _GcMlpFn.apply(x, cfg, *seq.parameters())


def gc_layer_torch(edge_seq, node_seq, aggregation: str, graph: dict, batch: int, e, xs, xd, residual: bool):
    """torch composition of one GraphCast message-passing layer (edge MLP on [e, xs[src], xd[dst]] (+ e), node MLP on
    [agg e', xd] + xd): (x', e') as [batch * n_dst, D], [batch * E, D].  Shared tables are [rows, D]."""
    src, dst = graph["src"].long(), graph["dst"].long()
    n_src, n_dst, ne = graph["n_src"], graph["n_dst"], src.numel()
    ar = torch.arange(batch, device=e.device).repeat_interleave(ne)
    e_b = e if e.shape[0] == batch * ne else e.repeat(batch, 1)
    xs_b = xs if xs.shape[0] == batch * n_src else xs.repeat(batch, 1)
    xd_b = xd if xd.shape[0] == batch * n_dst else xd.repeat(batch, 1)
    e_new = edge_seq(torch.cat((e_b, xs_b[src.repeat(batch) + ar * n_src], xd_b[dst.repeat(batch) + ar * n_dst]), dim=1))
    if residual:
        e_new = e_new + e_b
    t = dst.repeat(batch) + ar * n_dst
    agg = torch.zeros(batch * n_dst, e_new.shape[1], device=e.device, dtype=e.dtype).index_add(0, t, e_new)
    if aggregation == "mean":
        agg = agg / graph["deg"].clamp(min=1).to(e.dtype).repeat(batch).unsqueeze(1)
    return node_seq(torch.cat((agg, xd_b), dim=1)) + xd_b, e_new


class _GcLayerFn(torch.autograd.Function):
    """One GraphCast message-passing layer: the split edge MLP (node products W_s x_src, W_d x_dst computed once per node
    and gathered) writing e' = LN(z) (+ e), then the node MLP on [agg e', x_dst] + x_dst.  Saves the inputs (references),
    each MLP's pre-activations and LayerNorm input, and e'.  The backward runs the node MLP's first, so the edge
    LayerNorm backward gathers its aggregate gradient by destination (dlwp_gc_layernorm_bwd_f32); the source /
    destination products' gradients are per-node segment sums (N rows, not E).  DLWP_TRAIN_TORCH_BACKWARD=1
    differentiates gc_layer_torch instead."""

    @staticmethod
    def forward(ctx, e, xs, xd, cfg, *params):
        edge_seq, epk, node_seq, npk, aggregation, graph, batch, residual = cfg
        # batch strides: 0 for one [rows, D] table the batch shares (at batch 1 every operand counts as per sample)
        bs = tuple(rows * t.shape[-1] if t.shape[0] == batch * rows else 0
                   for t, rows in ((e, graph["src"].numel()), (xs, graph["n_src"]), (xd, graph["n_dst"])))
        with torch.no_grad():
            x_new, e_new, ze, zn = ops.gc_layer(epk, edge_seq, npk, node_seq, aggregation, graph, batch, e.detach(),
                                                xs.detach(), xd.detach(), bs, residual, save=True)
        ctx.save_for_backward(e, xs, xd, e_new, *ze, *zn, *params)   # the parameters: in-place edits raise
        ctx.cfg, ctx.n_ze, ctx.n_zn, ctx.bs = cfg, len(ze), len(zn), bs
        ctx.set_materialize_grads(False)
        return x_new, e_new

    @staticmethod
    def backward(ctx, gx_out, ge_out):
        edge_seq, epk, node_seq, npk, aggregation, graph, batch, residual = ctx.cfg
        sv = ctx.saved_tensors
        e, xs, xd, e_new = sv[:4]
        ze, zn = sv[4:4 + ctx.n_ze], sv[4 + ctx.n_ze:4 + ctx.n_ze + ctx.n_zn]
        e_bs, xs_bs, xd_bs = ctx.bs
        n_src, n_dst, ne = graph["n_src"], graph["n_dst"], graph["src"].numel()
        if _torch_backward_selected():
            form = lambda e_, xs_, xd_: gc_layer_torch(edge_seq, node_seq, aggregation, graph, batch, e_, xs_, xd_, residual)
            grads = _grad_of_torch_form(form, (e, xs, xd), ctx.needs_input_grad[:3], (gx_out, ge_out),
                                        params=[*edge_seq.parameters(), *node_seq.parameters()], zero_fill=True)
            return (*grads[:3], None, *grads[3:])
        if gx_out is None:
            gx_out = torch.zeros(batch * n_dst, xd.shape[-1], device=xd.device, dtype=torch.float32)
        gx_out = gx_out.contiguous()
        ge_out = ge_out.contiguous() if ge_out is not None else None
        d = e_new.shape[-1]
        # node MLP: x' = LN(mlp([agg e', x])) + x
        gu, _, gn = _gc_tail_backward(node_seq, batch, n_dst, zn, gx_out, False)
        nl0 = ops.mgn_parts(node_seq)[0][0]
        gn[0], gn[1] = ops.gc_weight_grad(ops.gc_agg_a_fields(xd, xd_bs, e_new, graph, aggregation), nl0.in_features,
                                          nl0.out_features, batch, n_dst, gu)
        v_agg, v_x = npk.backward_first(node_seq, (d, nl0.in_features - d))
        g_agg = ops.gc_data_grad(gu, v_agg, batch, n_dst)
        gxd = ops.gc_data_grad(gu, v_x, batch, n_dst, res=gx_out, res_bs=n_dst * xd.shape[-1])
        # edge MLP: e' = LN(mlp([e, xs[src], xd[dst]])) (+ e); its output gradient ge' + g_agg[dst] (/ deg) is formed
        # inside the LayerNorm backward
        gather = dict(g_agg=g_agg, g_agg_bs=n_dst * d, idx=graph["dst"],
                      deg=graph["deg"] if aggregation == "mean" else None)
        gz, ge_tot, gedge = _gc_tail_backward(edge_seq, batch, ne, ze, ge_out, False, ln_gather=gather,
                                              want_total=residual and ctx.needs_input_grad[0])
        el0 = ops.mgn_parts(edge_seq)[0][0]
        h, de = el0.out_features, e.shape[-1]
        w_e, w_s, w_d = epk.backward_first(edge_seq)
        dw0 = torch.empty(h, el0.in_features, device=e.device, dtype=torch.float32)
        _, gedge[1] = ops.gc_weight_grad(ops.gc_a_fields(0, e, e_bs), de, h, batch, ne, gz, dw=dw0[:, :de])
        gps = ops.gc_segment_sum(gz, batch, graph["src_row_ptr"], graph["src_perm"], n_src, batch_sum=not xs_bs)
        gpd = ops.gc_segment_sum(gz, batch, graph["row_ptr"], None, n_dst, batch_sum=not xd_bs)
        bs_s, bs_d = (batch if xs_bs else 1), (batch if xd_bs else 1)
        ds = xs.shape[-1]
        ops.gc_weight_grad(ops.gc_a_fields(0, xs, xs_bs), ds, h, bs_s, n_src, gps, dw=dw0[:, de:de + ds], bias=False)
        ops.gc_weight_grad(ops.gc_a_fields(0, xd, xd_bs), xd.shape[-1], h, bs_d, n_dst, gpd, dw=dw0[:, de + ds:], bias=False)
        gedge[0] = dw0
        gxs = ops.gc_data_grad(gps, w_s, bs_s, n_src) if ctx.needs_input_grad[1] else None
        gxd_out = None
        if ctx.needs_input_grad[2]:
            if not xd_bs:
                gxd = _gc_batch_sum(gxd, batch)
            gxd_out = ops.gc_data_grad(gpd, w_d, bs_d, n_dst, res=gxd, res_bs=n_dst * xd.shape[-1])
        ge = None
        if ctx.needs_input_grad[0]:
            ge = ops.gc_data_grad(gz, w_e, batch, ne, res=ge_tot, res_bs=ne * de)
            if not e_bs:
                ge = _gc_batch_sum(ge, batch)
        return (ge, gxs, gxd_out, None, *gedge, *gn)


def gc_layer(edge_seq, edge_packed, node_seq, node_packed, aggregation: str, graph: dict, batch: int, e, xs, xd,
             residual: bool):
    """differentiable GraphCast message-passing layer: (x' [batch * n_dst, D], e' [batch * E, D]).  e, xs, xd are per
    sample ([batch * rows, D]) or one table the batch shares ([rows, D]).  graph: row_ptr, src, dst, deg (CSC by
    destination), src_row_ptr, src_perm (ops.mgn_source_csr), n_src, n_dst."""
    cfg = (edge_seq, edge_packed, node_seq, node_packed, aggregation, graph, batch, residual)
    return _GcLayerFn.apply(e, xs, xd, cfg, *edge_seq.parameters(), *node_seq.parameters())


def mse_loss_torch(x, target, weight=None):
    """mean((target - x)^2 weight): the reference's CustomMSELoss.forward with reduction 'mean' (scripts/losses.py:175-188) as
    plain torch operators on any device; a float64 weight promotes the product, as there."""
    d = (target - x) ** 2
    if weight is not None:
        d = d * torch.as_tensor(weight, device=x.device)
    return torch.mean(d)


class _MseLossFn(torch.autograd.Function):
    """loss = mean((target - x)^2 weight) on dlwp_mse_loss_f32.  When x needs a gradient the forward writes
    d loss / d x = 2 (x - target) weight / N in the same pass (x and target are read once in the whole step); the backward only
    multiplies it by the upstream scalar, on the device, and that kernel touches nothing when the scalar is exactly 1 (the
    `loss.backward()` of train.py:271).  target and weight get no gradient."""

    @staticmethod
    def forward(ctx, x, target, weight):
        need = ctx.needs_input_grad[0]
        with torch.no_grad():
            loss, grad = ops.mse_loss_forward(x.detach(), target.detach(), weight, need_grad=need)
        if need:
            ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        (grad,) = ctx.saved_tensors
        with torch.no_grad():
            if getattr(ctx, "_used", False):        # the saved gradient was scaled in place: it serves one backward
                raise _lib.DlwpError("mse_loss: a second backward through the same loss is not supported")
            ctx._used = True
            g = ops.mse_loss_scale_grad(grad, grad_out)
        return g, None, None


def mse_loss(x, target, weight=None):
    """differentiable (in x) weighted mean squared error: HIP forward with the gradient written in the same pass; under
    DLWP_TRAIN_TORCH_BACKWARD=1 mse_loss_torch, left to autograd.  A target or weight that requires a gradient is outside
    the kernel's scope and raises."""
    if _torch_backward_selected():
        return mse_loss_torch(x, target, weight)
    if target.requires_grad or (weight is not None and weight.requires_grad):
        raise _lib.DlwpError("mse_loss: only the input can require a gradient")
    return _MseLossFn.apply(x, target, weight)


# ---- spherical harmonic transforms and the Driscoll-Healy mix (models/sfno.py; csrc/sht.hip forward and backward) ------------
# Each Function runs its HIP backward: the adjoint of a transform is the other transform's kernel over
# the same table, the mix has an input- and a weight-gradient kernel.  The torch form beside each computes the same thing from
# the SAME fp32 device tables (sphere.device_tables); it is differentiated under DLWP_TRAIN_TORCH_BACKWARD=1 and where a kernel
# answers "unsupported".
def _real_einsum_complex(eq: str, table: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """einsum of a real table with a complex tensor, part by part (einsum wants one dtype)"""
    return torch.complex(torch.einsum(eq, table, z.real), torch.einsum(eq, table, z.imag))


def sht_torch(x: torch.Tensor, tab) -> torch.Tensor:
    """what dlwp_sht_f32 computes, with torch operators: 2 pi rfft(norm="forward")[..., :mmax], then the contraction over
    latitude with tab.wleg [nlat, lmax, mmax]"""
    xf = torch.fft.rfft(x, dim=-1, norm="forward")[..., :tab.mmax] * (2.0 * math.pi)
    return _real_einsum_complex("klm,...km->...lm", tab.wleg, xf)


def isht_torch(c: torch.Tensor, tab) -> torch.Tensor:
    """what dlwp_isht_f32 computes: the contraction over l >= m with tab.leg [lmax, nlat, mmax] (the other triangle of c is
    masked out, not multiplied by the table's zeros), the imaginary parts of m = 0 and m = nlon / 2 dropped,
    irfft(n=nlon, norm="forward")"""
    lmax, mmax, nlon = tab.lmax, tab.mmax, tab.nlon
    keep = torch.ones(lmax, mmax, device=c.device).tril().bool()
    xf = _real_einsum_complex("lkm,...lm->...km", tab.leg, torch.where(keep, c, torch.zeros((), dtype=c.dtype, device=c.device)))
    real_only = torch.zeros(mmax, dtype=torch.bool, device=c.device)
    real_only[0] = True
    if nlon // 2 < mmax:
        real_only[nlon // 2] = True
    xf = torch.complex(xf.real, torch.where(real_only, torch.zeros((), device=c.device), xf.imag))
    if mmax < nlon // 2 + 1:        # the columns m >= mmax are zero
        xf = torch.cat([xf, torch.zeros(*xf.shape[:-1], nlon // 2 + 1 - mmax, dtype=xf.dtype, device=xf.device)], dim=-1)
    return torch.fft.irfft(xf, n=nlon, dim=-1, norm="forward")


def sph_mix_torch(c: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """what dlwp_sph_mix_f32 computes: einsum over the input channels per degree, entries above the diagonal (m > l) neither
    read nor written (zero)"""
    keep = torch.ones(c.shape[-2], c.shape[-1], device=c.device).tril().bool()
    zero = torch.zeros((), dtype=c.dtype, device=c.device)
    return torch.where(keep, torch.einsum("bilm,iol->bolm", torch.where(keep, c, zero), weight), zero)


def _hip_backward_or_none(run):
    """what `run` returns -- a HIP backward -- or None where the torch form is to be differentiated: under
    DLWP_TRAIN_TORCH_BACKWARD=1, and where the kernel answers DLWP_ERR_UNSUPPORTED.  Any other error raises."""
    if _torch_backward_selected():
        return None
    try:
        with torch.no_grad():
            return run()
    except _lib.DlwpError as e:
        if e.status != _lib.ERR_UNSUPPORTED:
            raise
    return None


class _ShtFn(torch.autograd.Function):
    """ops.sht forward, dlwp_sht_bwd_f32 backward.  Nothing is saved: the transform is linear, its backward needs the
    cotangent and the tables only (the torch-form branch differentiates at a zero field of the input's shape)."""

    @staticmethod
    def forward(ctx, x, tab):
        ctx.tab = tab
        ctx.in_shape = tuple(x.shape)
        with torch.no_grad():
            return ops.sht(x.detach(), tab.grid, tab.lmax, tab.mmax)

    @staticmethod
    def backward(ctx, grad_out):
        tab = ctx.tab
        g = _hip_backward_or_none(lambda: ops.sht_backward(grad_out.contiguous(), tab.grid, tab.nlat, tab.nlon))
        if g is None:
            zero = torch.zeros(ctx.in_shape, device=grad_out.device, dtype=torch.float32)
            g, = _grad_of_torch_form(lambda t: sht_torch(t, tab), (zero,), (True,), grad_out)
        return g, None


class _IshtFn(torch.autograd.Function):
    """ops.isht forward, dlwp_isht_bwd_f32 backward; nothing saved, as _ShtFn"""

    @staticmethod
    def forward(ctx, c, tab):
        ctx.tab = tab
        ctx.in_shape = tuple(c.shape)
        with torch.no_grad():
            return ops.isht(c.detach(), tab.grid, tab.nlat, tab.nlon)

    @staticmethod
    def backward(ctx, grad_out):
        tab = ctx.tab
        g = _hip_backward_or_none(lambda: ops.isht_backward(grad_out.contiguous(), tab.grid, tab.lmax, tab.mmax))
        if g is None:
            zero = torch.zeros(ctx.in_shape, device=grad_out.device, dtype=torch.complex64)
            g, = _grad_of_torch_form(lambda t: isht_torch(t, tab), (zero,), (True,), grad_out)
        return g, None


class _SphMixFn(torch.autograd.Function):
    """ops.sph_mix forward; backward the mix kernel over the conjugate-transposed weight (input gradient) and
    dlwp_sph_mix_wgrad_f32 (weight gradient), each only where needs_input_grad asks for it.  Saved: c and weight."""

    @staticmethod
    def forward(ctx, c, weight):
        ctx.save_for_backward(c, weight)
        with torch.no_grad():
            return ops.sph_mix(c.detach(), weight.detach())

    @staticmethod
    def backward(ctx, grad_out):
        c, weight = ctx.saved_tensors
        need_c, need_w = ctx.needs_input_grad
        if not (need_c or need_w):
            return None, None
        grads = _hip_backward_or_none(lambda: ops.sph_mix_backward(c, weight, grad_out.contiguous(), need_c, need_w))
        if grads is None:
            grads = _grad_of_torch_form(sph_mix_torch, (c, weight), (need_c, need_w), grad_out)
        return tuple(grads)


def sht(x, tab):
    """differentiable ops.sht: HIP forward and HIP backward (the torch form under DLWP_TRAIN_TORCH_BACKWARD=1)"""
    return _ShtFn.apply(x, tab)


def isht(c, tab):
    """differentiable ops.isht: HIP forward and HIP backward (the torch form under DLWP_TRAIN_TORCH_BACKWARD=1)"""
    return _IshtFn.apply(c, tab)


def sph_mix(c, weight):
    """differentiable ops.sph_mix: HIP forward and HIP backward (the torch form under DLWP_TRAIN_TORCH_BACKWARD=1)"""
    return _SphMixFn.apply(c, weight)
