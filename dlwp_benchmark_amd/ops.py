"""Thin Python wrappers over the C ABI (include/dlwp_hip.h) for ops used by several backbones.
Every wrapper takes CUDA tensors, validates them, and reaches a stream-taking entry point only through `lib.launch`,
which owns the device guard, the stream, pointer marshalling and the status check (`DlwpError` on a non-zero status).
No wrapper has a CPU path."""
import ctypes
import functools
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import lib as _lib
from .derived import Derived, bump_pack_epoch, derived_for, live_holders, pack_epoch, source_key  # noqa: F401 (re-exported)
# training.py imports this module at its top, so the other direction of the cycle stays lazy: the wrappers below import
# training (as _T) inside the function, where a gradient may be wanted

BIG = 1 << 30


def _contig(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else t.contiguous()


@dataclass
class WindowSpec:
    """Geometry of one (shifted-)window attention call, see struct dlwp_wattn_desc."""
    grid: Sequence[int]
    padded: Sequence[int]
    pad_lead: Sequence[int]
    window: Sequence[int]
    shift_fwd: Sequence[int]
    shift_back: Sequence[int]
    use_mask: bool
    mask_b1: Sequence[int]
    mask_b2: Sequence[int]
    bias_mode: int
    heads: int
    head_dim: int
    scale: float
    form: int = -1          # dlwp_window_attn_f32: -1 by window size, 0 fp32 MFMA, 1 bf16x6 (struct dlwp_wattn_desc.form)

    def to_c(self) -> "_lib.WAttnDesc":
        d = _lib.WAttnDesc()
        for name in ("grid", "padded", "pad_lead", "window", "shift_fwd", "shift_back", "mask_b1", "mask_b2"):
            arr = getattr(d, name)
            for i, v in enumerate(getattr(self, name)):
                arr[i] = int(v)
        d.use_mask = int(self.use_mask)
        d.bias_mode = int(self.bias_mode)
        d.heads, d.head_dim, d.scale = int(self.heads), int(self.head_dim), float(self.scale)
        d.form = int(self.form)
        return d


def window_attention(qkv: torch.Tensor, qkv_bias: Optional[torch.Tensor], table: torch.Tensor,
                     spec: WindowSpec, precision: str = "fp32", count_fallbacks: bool = False):
    """qkv [B, L, 3*C] (qkv Linear output, un-padded token order) -> [B, L, C].
    precision "fp32": fp32-accurate products (parity path; the form of the contractions by window size),
    "fp32_mfma" / "bf16x6": the same with the form forced (each is the other's cross-check);
    "bf16": bf16 MFMA operands, fp32 accumulate.
    count_fallbacks=True (diagnostics, synchronises): returns (out, workgroups of the fast path that left the exponent
    slack of their softmax offset and were recomputed with the exact row maximum)."""
    forms = {"fp32": spec.form, "fp32_mfma": 0, "bf16x6": 1, "bf16": -1}
    if precision not in forms:
        raise _lib.DlwpError(f"unknown attention precision {precision!r}")
    from . import training as _T
    if _T.wants_grad(qkv, qkv_bias, table) and not count_fallbacks:
        return _T.window_attention(qkv, qkv_bias, table, spec, precision)     # HIP forward, differentiable (training.py)
    if qkv.dtype == torch.bfloat16:
        # the hand-over of a block in the all-bf16 form: bf16 qkv in, bf16 attention output (dlwp_window_attn_bf16_io)
        if precision != "bf16" or count_fallbacks:
            raise _lib.DlwpError("window_attention: a bfloat16 qkv tensor goes with precision='bf16'")
        return _window_attention_bf16_io(qkv, qkv_bias, table, spec)
    _lib.require_cuda_tensor(qkv, "qkv")
    _lib.require_cuda_tensor(table, "bias table")
    _lib.require_cuda_tensor(qkv_bias, "qkv bias")
    qkv = qkv.contiguous()
    table = table.contiguous()
    b, l, c3 = qkv.shape
    c = spec.heads * spec.head_dim
    if c3 != 3 * c or l != spec.grid[0] * spec.grid[1] * spec.grid[2]:
        raise _lib.DlwpError(f"qkv shape {tuple(qkv.shape)} does not match grid {tuple(spec.grid)} x 3*{c}")
    out = torch.empty(b, l, c, device=qkv.device, dtype=torch.float32)
    lib = _lib.load()
    d = spec.to_c()
    d.form = forms[precision]
    bf16 = precision == "bf16"
    # the caller (torch's caching allocator) owns the workspace of the fast path; 0 bytes = generic kernel
    nbytes = int(lib.dlwp_window_attn_workspace_bytes(ctypes.byref(d), b, 1 if bf16 else 0))
    ws = _lib.workspace(nbytes, qkv.device)
    _lib.launch("dlwp_window_attn_bf16" if bf16 else "dlwp_window_attn_f32", qkv.device, d, qkv, _contig(qkv_bias), table, out,
                b, ws, nbytes)
    if count_fallbacks:
        n = ctypes.c_int32(0)
        if ws is not None:
            with torch.cuda.device(qkv.device):     # spelled out: the stream is not this entry point's last parameter
                _lib.check(lib.dlwp_window_attn_fallbacks(ctypes.byref(d), b, 1 if bf16 else 0, ws.data_ptr(),
                                                          _lib.stream_ptr(), ctypes.byref(n)), "dlwp_window_attn_fallbacks")
        return out, int(n.value)
    return out


def window_attention_io_supported(spec: WindowSpec, batch: int) -> bool:
    """True when dlwp_window_attn_bf16_io covers the descriptor (one of the two fast kernels takes it)."""
    d = spec.to_c()
    d.form = -1
    return int(_lib.load().dlwp_window_attn_workspace_bytes(ctypes.byref(d), int(batch), 1)) > 0


def _bias_bf16(bias: torch.Tensor) -> torch.Tensor:
    """bfloat16 image of a qkv bias (read by the earth-window kernel for zero-padded tokens), converted once per parameter
    state instead of once per call; it lives as long as the bias (a captured step has its pointer baked in)."""
    return derived_for(bias, "bias_bf16").get(source_key(bias), lambda: bias.detach().to(torch.bfloat16).contiguous())


def _window_attention_bf16_io(qkv: torch.Tensor, qkv_bias: Optional[torch.Tensor], table: torch.Tensor, spec: WindowSpec):
    if not qkv.is_cuda:
        raise _lib.DlwpError("qkv must be a tensor on an MI355X device")
    _lib.require_cuda_tensor(table, "bias table")
    qkv, table = qkv.contiguous(), table.contiguous()
    b, l, c3 = qkv.shape
    c = spec.heads * spec.head_dim
    if c3 != 3 * c or l != spec.grid[0] * spec.grid[1] * spec.grid[2]:
        raise _lib.DlwpError(f"qkv shape {tuple(qkv.shape)} does not match grid {tuple(spec.grid)} x 3*{c}")
    bias16 = _bias_bf16(qkv_bias) if qkv_bias is not None else None
    out = torch.empty(b, l, c, device=qkv.device, dtype=torch.bfloat16)
    d = spec.to_c()
    d.form = -1
    nbytes = int(_lib.load().dlwp_window_attn_workspace_bytes(ctypes.byref(d), b, 1))
    ws = _lib.workspace(max(nbytes, 256), qkv.device)
    rc = _lib.launch("dlwp_window_attn_bf16_io", qkv.device, d, qkv, bias16, table, out, b, ws, nbytes,
                     accept=(_lib.ERR_UNSUPPORTED,))
    if rc == _lib.ERR_UNSUPPORTED:     # a descriptor only the generic kernel takes -- the same arithmetic on fp32 tensors
        return window_attention(qkv.float(), qkv_bias, table, spec, precision="bf16").to(torch.bfloat16)
    return out


def window_attention_backward(qkv: torch.Tensor, qkv_bias: Optional[torch.Tensor], table: torch.Tensor, spec: WindowSpec,
                              grad_out: torch.Tensor):
    """Gradients of window_attention (fp32) with respect to qkv, the qkv bias (through zero-padded tokens; None when the
    descriptor does not pad or no bias was given) and the bias table: dlwp_window_attn_bwd_f32, flash-style -- the scores are
    recomputed per tile, no [B, heads, N, N] tensor exists (reference backward: scripts/train.py:271 through
    swin_transformer.py:122-154 / panguweather.py:176-211)."""
    _lib.require_cuda_tensor(qkv, "qkv")
    _lib.require_cuda_tensor(table, "bias table")
    _lib.require_cuda_tensor(qkv_bias, "qkv bias")
    _lib.require_cuda_tensor(grad_out, "grad_out")
    qkv, table, grad_out = qkv.contiguous(), table.contiguous(), grad_out.contiguous()
    b, l, c3 = qkv.shape
    c = spec.heads * spec.head_dim
    if c3 != 3 * c or l != spec.grid[0] * spec.grid[1] * spec.grid[2] or tuple(grad_out.shape) != (b, l, c):
        raise _lib.DlwpError(f"qkv {tuple(qkv.shape)} / grad_out {tuple(grad_out.shape)} do not match grid {tuple(spec.grid)} x 3*{c}")
    padded = tuple(spec.padded) != tuple(spec.grid)
    gqkv = torch.empty_like(qkv)
    gtab = torch.empty_like(table)
    gbias = torch.empty(3 * c, device=qkv.device, dtype=torch.float32) if (padded and qkv_bias is not None) else None
    d = spec.to_c()
    nbytes = int(_lib.load().dlwp_window_attn_bwd_workspace_bytes(ctypes.byref(d), b))
    ws = _lib.workspace(nbytes, qkv.device)
    _lib.launch("dlwp_window_attn_bwd_f32", qkv.device, d, qkv, _contig(qkv_bias), table, grad_out, gqkv, gbias, gtab, b, ws,
                nbytes)
    return gqkv, gbias, gtab


ACTS = {"none": 0, "gelu": 1, "tanh": 2, "relu": 3, "silu": 4}


def act_code(activation) -> int:
    """Maps the reference's activation spec (module instance or the config string that the
    reference `eval`s, e.g. "th.nn.GELU()", unet.py:292) to the kernel's activation id."""
    n = activation if isinstance(activation, str) else type(activation).__name__
    for key, tag in (("GELU", "gelu"), ("Tanh", "tanh"), ("LeakyReLU", None), ("ReLU", "relu"), ("SiLU", "silu"),
                     ("Identity", "none")):
        if key in n:
            if tag is None:
                break
            return ACTS[tag]
    raise _lib.DlwpError(f"activation {activation!r} has no fused kernel (supported: GELU, Tanh, ReLU, SiLU)")


# forms of the convolutions: "direct" (default) is the scalar-FMA kernel of csrc/conv.hip (pad(1) + Conv2d(3x3)) or the
# one-thread-per-output kernels of csrc/conv2.hip (conv2d / conv_transpose2d / small_module); "bf16x6" / "bf16" are the implicit
# GEMM of csrc/conv_mfma.hip on the bf16 matrix instructions (fp32-grade three-part splits / RNE bf16 operands), one kernel for all
CONV_FORMS = ("direct", "bf16x6", "bf16")


class ConvWeights:
    """A convolution weight ([cout, cin, k, k]; transposed: ConvTranspose2d's [cin, cout, k, k]) in the MFMA operand layout the
    kernel of csrc/conv_mfma.hip reads (three bf16 images; form "bf16" reads the first), re-packed on the device whenever the
    parameter has been written to -- the derivation rule of LinearWeights.  Packing is a launch of its own and allocates: it
    happens in the eager or warm-up pass; inside a graph capture a stale or missing pack is an error.  `op` names the operation
    in messages."""

    def __init__(self, op: str, transposed: bool = False):
        self._derived = Derived(eager_only=op)
        self._op = op
        self._transposed = bool(transposed)

    def pack(self, weight: torch.Tensor) -> torch.Tensor:
        """a fresh pack of `weight` as it lies now, outside the cache (one launch, one allocation)"""
        cout, cin = (weight.shape[1], weight.shape[0]) if self._transposed else weight.shape[:2]
        k = weight.shape[2]
        lib = _lib.load()
        nbytes = int(lib.dlwp_conv2d_mfma_packed_bytes(cout, cin, k))
        if nbytes == 0:
            raise _lib.DlwpError(f"{self._op}: unsupported shape cout={cout} cin={cin} k={k} for the matrix-pipe forms")
        buf = torch.empty(nbytes // 4, dtype=torch.int32, device=weight.device)
        _lib.launch("dlwp_conv2d_mfma_pack_f32", weight.device, weight.detach().contiguous(), cout, cin, k,
                    int(self._transposed), buf)
        return buf

    def get(self, weight: torch.Tensor) -> torch.Tensor:
        return self._derived.get(source_key(weight), lambda: self.pack(weight))


def conv3x3_weights(weight: torch.Tensor) -> ConvWeights:
    """The pack cache of ops.conv3x3* that belongs to `weight` (a Parameter, or any tensor the caller keeps alive)."""
    return derived_for(weight, "conv3x3", lambda: ConvWeights("conv3x3"))


def conv2d_weights(weight: torch.Tensor, transposed: bool = False) -> ConvWeights:
    """The pack cache of ops.conv2d (transposed: of ops.conv_transpose2d) that belongs to `weight`; the layout flag is part
    of the slot, so a ConvTranspose2d weight and a Conv2d weight of the same shape never share a pack."""
    return derived_for(weight, ("conv2d", bool(transposed)), lambda: ConvWeights("conv2d", transposed))


def _conv_form(form: str) -> str:
    if form not in CONV_FORMS:
        raise _lib.DlwpError(f"unknown conv form {form!r} (one of {CONV_FORMS})")
    return form


def conv3x3_cyl(x0: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: int = 0,
                x1: Optional[torch.Tensor] = None, form: str = "direct") -> torch.Tensor:
    """CylinderPad(1) + Conv2d(3x3) + bias + activation on cat([x0, x1], 1) without the cat.  `form`: CONV_FORMS."""
    from . import training as _T
    if _conv_form(form) != "direct" or _T.wants_grad(x0, x1, weight, bias):      # (conv3x3 ignores `form` under autograd)
        return conv3x3(x0, weight, bias, act=act, x1=x1, form=form)
    _lib.require_cuda_tensor(x0, "x0")
    _lib.require_cuda_tensor(x1, "x1")
    _lib.require_cuda_tensor(weight, "weight")
    x0 = x0.contiguous()
    x1 = x1.contiguous() if x1 is not None else None
    weight = weight.contiguous()
    b, c0, h, w = x0.shape
    c1 = x1.shape[1] if x1 is not None else 0
    cout = weight.shape[0]
    if tuple(weight.shape[1:]) != (c0 + c1, 3, 3):
        raise _lib.DlwpError(f"weight {tuple(weight.shape)} does not match {c0}+{c1} input channels, 3x3")
    y = torch.empty(b, cout, h, w, device=x0.device, dtype=torch.float32)
    _lib.launch("dlwp_conv3x3_cyl_f32", x0.device, x0, c0, x1, c1, weight, _contig(bias), y, b, h, w, cout, act)
    return y


def conv3x3_hpx(x0: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: int = 0,
                x1: Optional[torch.Tensor] = None, form: str = "direct") -> torch.Tensor:
    """HEALPixPadding(1) + Conv2d(3x3) + bias + activation on cat([x0, x1], 1); x [(B*12), C, H, W].  `form`: CONV_FORMS."""
    from . import healpix as _hpx
    from . import training as _T
    if _conv_form(form) != "direct" or _T.wants_grad(x0, x1, weight, bias):      # (conv3x3 ignores `form` under autograd)
        return conv3x3(x0, weight, bias, act=act, x1=x1, hpx=True, form=form)

    _lib.require_cuda_tensor(x0, "x0")
    _lib.require_cuda_tensor(x1, "x1")
    _lib.require_cuda_tensor(weight, "weight")
    x0 = x0.contiguous()
    x1 = x1.contiguous() if x1 is not None else None
    weight = weight.contiguous()
    n, c0, h, w = x0.shape
    c1 = x1.shape[1] if x1 is not None else 0
    cout = weight.shape[0]
    if n % 12:
        raise _lib.DlwpError(f"leading dimension {n} is not (batch * 12 faces)")
    if tuple(weight.shape[1:]) != (c0 + c1, 3, 3):
        raise _lib.DlwpError(f"weight {tuple(weight.shape)} does not match {c0}+{c1} input channels, 3x3")
    table = _hpx.device_table(h, w, 1, x0.device)
    y = torch.empty(n, cout, h, w, device=x0.device, dtype=torch.float32)
    _lib.launch("dlwp_conv3x3_hpx_f32", x0.device, x0, c0, x1, c1, weight, _contig(bias), y, n, h, w, cout, act, table)
    return y


def conv3x3(x0: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: int = 0,
            x1: Optional[torch.Tensor] = None, pre_act: int = 0, resid: Optional[torch.Tensor] = None,
            hpx: bool = False, form: str = "direct") -> torch.Tensor:
    """pad(1) + Conv2d(3x3) on cat([x0, x1], 1) with the input activation `pre_act` applied while staging and
    `resid` added before `act`; padding rule: CylinderPad, or HEALPixPadding when hpx (x [(B*12), C, H, W]).
    `form` (CONV_FORMS): "direct" the scalar-FMA kernel; "bf16x6" / "bf16" dlwp_conv3x3_mfma_f32 (inference only: with
    gradients wanted every form runs the differentiable direct path)."""
    _conv_form(form)
    for t, n in ((x0, "x0"), (x1, "x1"), (weight, "weight"), (resid, "resid")):
        _lib.require_cuda_tensor(t, n)
    from . import training as _T
    if _T.wants_grad(x0, x1, weight, bias, resid):
        return _T.conv3x3(x0, weight, bias, act=act, x1=x1, pre_act=pre_act, resid=resid, hpx=hpx)   # HIP forward, differentiable
    owner = weight          # the pack belongs to the caller's tensor, not to a contiguous copy made below
    x0 = x0.contiguous()
    x1 = x1.contiguous() if x1 is not None else None
    weight = weight.contiguous()
    n, c0, h, w = x0.shape
    c1 = x1.shape[1] if x1 is not None else 0
    cout = weight.shape[0]
    if tuple(weight.shape[1:]) != (c0 + c1, 3, 3):
        raise _lib.DlwpError(f"weight {tuple(weight.shape)} does not match {c0}+{c1} input channels, 3x3")
    if resid is not None and (tuple(resid.shape) != (n, cout, h, w) or not resid.is_contiguous()):
        raise _lib.DlwpError("conv3x3: resid must be contiguous and shaped like the output")
    table = None
    if hpx:
        from . import healpix as _hpx

        if n % 12:
            raise _lib.DlwpError(f"leading dimension {n} is not (batch * 12 faces)")
        table = _hpx.device_table(h, w, 1, x0.device)
    y = torch.empty(n, cout, h, w, device=x0.device, dtype=torch.float32)
    if form != "direct":
        packed = conv3x3_weights(owner).get(owner)
        _lib.launch("dlwp_conv3x3_mfma_f32", x0.device, x0, c0, x1, c1, packed, _contig(bias), resid, y, n, h, w, cout,
                    int(pre_act), int(act), table, CONV_FORMS.index(form) - 1)
        return y
    _lib.launch("dlwp_conv3x3_ex_f32", x0.device, x0, c0, x1, c1, weight, _contig(bias), resid, y, n, h, w, cout, int(pre_act),
                int(act), table)
    return y


def groupnorm_act(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], groups: int,
                  eps: float = 1e-5, act: int = 0) -> torch.Tensor:
    """act(GroupNorm(groups)(x)) for x [N, C, ...] (reference unet.py:739 + :761, :887-888), one launch."""
    _lib.require_cuda_tensor(x, "x")
    from . import training as _T
    if _T.wants_grad(x, weight, bias):
        return _T.groupnorm_act(x, weight, bias, groups, eps, act)           # HIP forward and backward (training.py)
    x = x.contiguous()
    n, c = x.shape[0], x.shape[1]
    hw = x.numel() // (n * c)
    y = torch.empty_like(x)
    _lib.launch("dlwp_groupnorm_act_f32", x.device, x, _contig(weight), _contig(bias), y, n, c, hw, int(groups), float(eps),
                int(act))
    return y


def groupnorm_act_fwd_stats(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], groups: int,
                            eps: float = 1e-5, act: int = 0):
    """groupnorm_act that also returns the statistics a backward needs: (y, stats [N, groups, 2] = (mean, rstd)).  y is
    bit-equal to groupnorm_act's (the same kernel).  Not differentiable: training.groupnorm_act is."""
    _lib.require_cuda_tensor(x, "x")
    x = x.contiguous()
    n, c = x.shape[0], x.shape[1]
    hw = x.numel() // (n * c)
    y = torch.empty_like(x)
    stats = torch.empty(n, max(int(groups), 1), 2, device=x.device, dtype=torch.float32)
    _lib.launch("dlwp_groupnorm_act_fwd_stats_f32", x.device, x, _contig(weight), _contig(bias), y, stats, n, c, hw, int(groups),
                float(eps), int(act))
    return y, stats


def groupnorm_act_backward(x: torch.Tensor, stats: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                           grad_out: torch.Tensor, groups: int, act: int = 0, need_x: bool = True, need_weight: bool = True,
                           need_bias: bool = True):
    """The gradients of groupnorm_act on dlwp_groupnorm_act_bwd_f32 from x, the forward's stats [N, groups, 2] and grad_out
    (both contiguous, [N, C, *]): (dx, dgamma, dbeta), None where not wanted.  Runs on the current stream without a host
    synchronisation; reruns are bitwise identical."""
    for t, name in ((x, "x"), (stats, "stats"), (grad_out, "grad_out")):
        _lib.require_cuda_tensor(t, name)
    n, c = x.shape[0], x.shape[1]
    hw = x.numel() // max(n * c, 1)
    if grad_out.shape != x.shape or not x.is_contiguous() or not grad_out.is_contiguous():
        raise _lib.DlwpError(f"groupnorm_act_backward: x {tuple(x.shape)} and grad_out {tuple(grad_out.shape)} must be "
                             "contiguous and of one shape")
    if int(groups) <= 0 or stats.numel() != 2 * n * int(groups) or not stats.is_contiguous():
        raise _lib.DlwpError(f"groupnorm_act_backward: stats of {stats.numel()} values, 2 * {n} * {groups} needed")
    dx = torch.empty_like(x) if need_x else None
    dw = torch.empty(c, device=x.device, dtype=torch.float32) if need_weight else None
    db = torch.empty(c, device=x.device, dtype=torch.float32) if need_bias else None
    ws = _lib.workspace(max(int(_lib.load().dlwp_groupnorm_act_bwd_workspace_bytes(n, c)), 4), x.device)
    _lib.launch("dlwp_groupnorm_act_bwd_f32", x.device, x, stats, _contig(weight), _contig(bias), grad_out, dx, dw, db, ws, n, c,
                hw, int(groups), int(act))
    return dx, dw, db


def _conv_pack(weight: torch.Tensor, transposed: bool, cached: bool) -> torch.Tensor:
    """the matrix-pipe pack of a convolution weight: from the cache that belongs to the tensor, or (cached False) made now.
    The training step packs per call, as linear_raw does: its parameters are also written by launches that move no version
    counter (optim.FusedAdamW, ExponentialMovingAverage) and inside replayed step graphs, where a cached pack would go stale
    without a sign; a pack launch made per call is part of the captured step."""
    if cached:
        return conv2d_weights(weight, transposed).get(weight)
    return ConvWeights("conv2d", transposed).pack(weight)


def conv2d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], stride: int = 1, padding: int = 0,
           pre_act: int = 0, act: int = 0, resid: Optional[torch.Tensor] = None, form: str = "direct",
           cached: bool = True) -> torch.Tensor:
    """zero-padded Conv2d (square kernel / stride / padding): the strided and 1x1 convolutions of unet.py:583-584, :879, :450.
    `form` (CONV_FORMS): "direct" the one-thread-per-output kernel; "bf16x6" / "bf16" dlwp_conv2d_mfma_f32 (k <= 4, stride 1 or 2,
    padding < k; anything else raises.  Inference only: with gradients wanted every form runs training.conv2d -- the library's
    forward and input gradient, under DLWP_CONV_DGRAD=hip the "bf16x6" kernel and dlwp_conv2d_dgrad_mfma_f32; the weight and
    bias gradient on dlwp_conv2d_wgrad_f32 under DLWP_CONV_WGRAD).  `cached` False: the pack is made in this call (_conv_pack)."""
    _conv_form(form)
    for t, n in ((x, "x"), (weight, "weight"), (resid, "resid")):
        _lib.require_cuda_tensor(t, n)
    from . import training as _T
    if _T.wants_grad(x, weight, bias, resid):       # DLWP_CONV_DGRAD: library or HIP forward and input gradient (training.py)
        return _T.conv2d(x, weight, bias, resid, int(stride), int(padding), int(pre_act), int(act))
    owner = weight          # the pack belongs to the caller's tensor, not to a contiguous copy made below
    x, weight = x.contiguous(), weight.contiguous()
    n, cin, h, w = x.shape
    cout, cin_w, k, k2 = weight.shape
    if cin_w != cin or k != k2:
        raise _lib.DlwpError(f"conv2d: weight {tuple(weight.shape)} does not match input {tuple(x.shape)}")
    oh, ow = (h + 2 * padding - k) // stride + 1, (w + 2 * padding - k) // stride + 1
    if resid is not None and (tuple(resid.shape) != (n, cout, oh, ow) or not resid.is_contiguous()):
        raise _lib.DlwpError("conv2d: resid must be contiguous and shaped like the output")
    y = torch.empty(n, cout, oh, ow, device=x.device, dtype=torch.float32)
    if form != "direct":
        packed = _conv_pack(owner, False, cached)
        _lib.launch("dlwp_conv2d_mfma_f32", x.device, x, packed, _contig(bias), resid, y, n, cin, h, w, cout, k, int(stride),
                    int(padding), int(pre_act), int(act), CONV_FORMS.index(form) - 1)
        return y
    _lib.launch("dlwp_conv2d_f32", x.device, x, weight, _contig(bias), resid, y, n, cin, h, w, cout, k, int(stride), int(padding),
                int(pre_act), int(act))
    return y


def conv_transpose2d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], stride: int, padding: int = 0,
                     act: int = 0, form: str = "direct", cached: bool = True) -> torch.Tensor:
    """ConvTranspose2d (weight [cin, cout, k, k]; unet.py:523 2x2 s2, :719 4x4 s2 p1).  `form` (CONV_FORMS): "direct" the
    one-thread-per-output kernel; "bf16x6" / "bf16" dlwp_conv_transpose2d_mfma_f32 (exactly those two geometries; anything else
    raises.  Inference only: with gradients wanted every form runs training.conv_transpose2d, as conv2d does).  `cached` as
    conv2d's."""
    _conv_form(form)
    _lib.require_cuda_tensor(x, "x")
    _lib.require_cuda_tensor(weight, "weight")
    from . import training as _T
    if _T.wants_grad(x, weight, bias):              # DLWP_CONV_DGRAD: library or HIP forward and input gradient (training.py)
        return _T.conv_transpose2d(x, weight, bias, int(stride), int(padding), int(act))
    owner = weight
    x, weight = x.contiguous(), weight.contiguous()
    n, cin, h, w = x.shape
    cin_w, cout, k, k2 = weight.shape
    if cin_w != cin or k != k2:
        raise _lib.DlwpError(f"conv_transpose2d: weight {tuple(weight.shape)} does not match input {tuple(x.shape)}")
    oh, ow = (h - 1) * stride - 2 * padding + k, (w - 1) * stride - 2 * padding + k
    y = torch.empty(n, cout, oh, ow, device=x.device, dtype=torch.float32)
    if form != "direct":
        packed = _conv_pack(owner, True, cached)
        _lib.launch("dlwp_conv_transpose2d_mfma_f32", x.device, x, packed, _contig(bias), y, n, cin, h, w, cout, k, int(stride),
                    int(padding), int(act), CONV_FORMS.index(form) - 1)
        return y
    _lib.launch("dlwp_conv_transpose2d_f32", x.device, x, weight, _contig(bias), y, n, cin, h, w, cout, k, int(stride),
                int(padding), int(act))
    return y


def avgpool2x2(x: torch.Tensor) -> torch.Tensor:
    """AvgPool2d(kernel_size=2, stride=2) (unet.py:450).  With a gradient wanted: F.avg_pool2d, under DLWP_CONV_DGRAD=hip this
    kernel and dlwp_avgpool2x2_bwd_f32 (training._AvgPool2x2Fn)."""
    _lib.require_cuda_tensor(x, "x")
    if torch.is_grad_enabled() and x.requires_grad:
        from . import training as _T
        if _T.conv_dgrad_uses_hip() and x.dtype == torch.float32 and x.dim() == 4 and min(x.shape[2:]) >= 2:
            return _T.avgpool2x2(x)                 # this kernel forward, dlwp_avgpool2x2_bwd_f32 backward
        return torch.nn.functional.avg_pool2d(x, 2)
    x = x.contiguous()
    n, c, h, w = x.shape
    y = torch.empty(n, c, h // 2, w // 2, device=x.device, dtype=torch.float32)
    _lib.launch("dlwp_avgpool2x2_f32", x.device, x, y, n * c, h, w)
    return y


def avgpool2x2_backward(gy: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """The adjoint of avgpool2x2 on an input of h x w: gy [N, C, h // 2, w // 2] -> dx [N, C, h, w], dx[2i + u][2j + v] =
    0.25 gy[i][j], a trailing odd row or column 0 (dlwp_avgpool2x2_bwd_f32; every element is written)."""
    _lib.require_cuda_tensor(gy, "gy")
    gy = gy.contiguous()
    n, c, oh, ow = gy.shape
    h, w = int(h), int(w)
    if (oh, ow) != (h // 2, w // 2) or min(oh, ow) < 1:
        raise _lib.DlwpError(f"avgpool2x2_backward: gy {tuple(gy.shape)} is not the pooled map of {h} x {w}")
    dx = torch.empty(n, c, h, w, device=gy.device, dtype=torch.float32)
    if dx.numel():
        _lib.launch("dlwp_avgpool2x2_bwd_f32", gy.device, gy, dx, n * c, h, w)
    return dx


class ConvAdjointWeights:
    """A Conv2d weight [cout, cin, k, k] packed for its input gradient (dlwp_conv2d_dgrad_mfma_f32): the channels exchanged,
    k_packed >= k taps per axis, the taps reversed or not -- what dlwp_conv2d_dgrad_mfma_variant names for the layer's stride.
    A buffer of its own beside the forward pack of the same tensor, re-derived by ConvWeights' rule."""

    def __init__(self, k_packed: int, flip: bool):
        self._derived = Derived(eager_only="conv2d_input_grad")
        self._k_packed, self._flip = int(k_packed), bool(flip)

    def pack(self, weight: torch.Tensor) -> torch.Tensor:
        """a fresh adjoint pack of `weight` as it lies now, outside the cache"""
        cout, cin, k = weight.shape[:3]
        nbytes = int(_lib.load().dlwp_conv2d_mfma_packed_bytes(cin, cout, self._k_packed))
        if nbytes == 0:
            raise _lib.DlwpError(f"conv2d_input_grad: unsupported shape cout={cout} cin={cin} k={k} for the matrix-pipe forms")
        buf = torch.empty(nbytes // 4, dtype=torch.int32, device=weight.device)
        _lib.launch("dlwp_conv2d_mfma_pack_ex_f32", weight.device, weight.detach().contiguous(), cin, cout, k,
                    self._k_packed, 1, int(self._flip), buf)
        return buf

    def get(self, weight: torch.Tensor) -> torch.Tensor:
        return self._derived.get(source_key(weight), lambda: self.pack(weight))


def conv2d_adjoint_weights(weight: torch.Tensor, k_packed: int, flip: bool) -> ConvAdjointWeights:
    """The adjoint-pack cache of conv2d_input_grad that belongs to `weight`: a slot per (k_packed, flip), none shared with
    conv2d_weights."""
    return derived_for(weight, ("conv2d_adjoint", int(k_packed), bool(flip)), lambda: ConvAdjointWeights(k_packed, flip))


def _conv2d_dgrad_variant(batch, cin, cout, h, w, k, stride, padding) -> int:
    args = [int(v) for v in (batch, cin, cout, h, w, k, stride, padding)]
    if min(args[:7]) < 1 or args[7] < 0 or max(args) >= 1 << 31:
        return 0
    return int(_lib.load().dlwp_conv2d_dgrad_mfma_variant(*args))


def conv2d_input_grad_supported(batch: int, cin: int, cout: int, h: int, w: int, k: int, stride: int, padding: int) -> bool:
    """whether dlwp_conv2d_dgrad_mfma_f32 takes the input gradient of Conv2d(cin -> cout, k, stride, padding) on [batch, cin,
    h, w] (the launcher's own checks; its envelope: include/dlwp_hip.h); needs the library, not a GPU"""
    return _conv2d_dgrad_variant(batch, cin, cout, h, w, k, stride, padding) != 0


def conv2d_input_grad(gz: torch.Tensor, weight: torch.Tensor, x_shape, stride: int, padding: int,
                      out: Optional[torch.Tensor] = None, cached: bool = True) -> torch.Tensor:
    """The input gradient of conv2d: gz [N, cout, SH, SW], the gradient of the convolution's output, and the layer's weight
    [cout, cin, k, k] -> dx of x_shape = [N, cin, H, W] on dlwp_conv2d_dgrad_mfma_f32 (fp32-grade, every element written, reruns
    bit-identical).  `out`: a contiguous fp32 tensor of x_shape to write instead of a new one (any 4-byte alignment).  A geometry
    outside the envelope raises; conv2d_input_grad_supported asks first.  `cached` False: the adjoint pack is made in this call
    from the weight as it lies (what the training step does, see _conv_pack)."""
    _lib.require_cuda_tensor(gz, "gz")
    _lib.require_cuda_tensor(weight, "weight")
    gz = gz.contiguous()
    n, cin, h, w = (int(v) for v in x_shape)
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or weight.shape[1] != cin:
        raise _lib.DlwpError(f"conv2d_input_grad: weight {tuple(weight.shape)} does not match an input of {cin} channels")
    cout, _, k, _ = weight.shape
    stride, padding = int(stride), int(padding)
    variant = _conv2d_dgrad_variant(n, cin, cout, h, w, k, stride, padding)
    if variant == 0:
        raise _lib.DlwpError(f"conv2d_input_grad: no HIP kernel for {cin} <- {cout} channels on {n} x {h} x {w}, k={k} "
                             f"stride={stride} padding={padding}")
    if tuple(gz.shape) != (n, cout, *_conv2d_out_hw(h, w, k, stride, padding, False)):
        raise _lib.DlwpError(f"conv2d_input_grad: gz {tuple(gz.shape)} is not the output map of {tuple(x_shape)} under k={k} "
                             f"stride={stride} padding={padding}")
    k_packed, flip = variant >> 12, not (variant >> 10) & 1
    packed = (conv2d_adjoint_weights(weight, k_packed, flip).get(weight) if cached
              else ConvAdjointWeights(k_packed, flip).pack(weight))
    dx = out if out is not None else torch.empty(n, cin, h, w, device=gz.device, dtype=torch.float32)
    if out is not None and (tuple(out.shape) != (n, cin, h, w) or out.dtype != torch.float32 or not out.is_contiguous() or
                            out.device != gz.device):
        raise _lib.DlwpError(f"conv2d_input_grad: out must be a contiguous fp32 tensor of {(n, cin, h, w)} on {gz.device}")
    _lib.launch("dlwp_conv2d_dgrad_mfma_f32", gz.device, gz, packed, dx, n, cin, h, w, cout, k, stride, padding)
    return dx


def conv_transpose2d_input_grad_supported(batch: int, cin: int, cout: int, sh: int, sw: int, k: int, stride: int,
                                          padding: int) -> bool:
    """whether conv_transpose2d_input_grad takes gz [batch, cout, sh, sw]: the envelope of dlwp_conv2d_mfma_f32 (k <= 4, stride
    1 or 2, padding < k)"""
    args = [int(v) for v in (batch, sh, sw, cin, k, stride, padding)]
    if min(args[:6]) < 1 or args[6] < 0 or int(cout) < 1 or max(*args, int(cout)) >= 1 << 31:
        return False
    lib = _lib.load()
    return lib.dlwp_conv2d_mfma_variant(0, *args) != 0 and lib.dlwp_conv2d_mfma_packed_bytes(int(cin), int(cout), int(k)) > 0


def conv_transpose2d_input_grad(gz: torch.Tensor, weight: torch.Tensor, stride: int, padding: int,
                                cached: bool = True) -> torch.Tensor:
    """The input gradient of conv_transpose2d: gz [N, cout, OH, OW] and the layer's weight [cin, cout, k, k] -> dx [N, cin, H,
    W].  It is the Conv2d forward of gz with the same stride and padding and the weight read as a Conv2d weight of cin output
    and cout input channels -- no flip, no copy: dlwp_conv2d_mfma_f32 in the "bf16x6" form on conv2d_weights(weight), the
    untransposed pack (its own slot beside the layer's forward pack; `cached` False: made in this call)."""
    _lib.require_cuda_tensor(gz, "gz")
    _lib.require_cuda_tensor(weight, "weight")
    if weight.dim() != 4 or weight.shape[1] != gz.shape[1]:
        raise _lib.DlwpError(f"conv_transpose2d_input_grad: weight {tuple(weight.shape)} does not match gz {tuple(gz.shape)}")
    with torch.no_grad():           # `weight` itself, not a detached alias: the pack belongs to the caller's tensor
        return conv2d(gz.detach(), weight, None, int(stride), int(padding), form="bf16x6", cached=cached)


def small_module(m: torch.nn.Module, x: torch.Tensor, act: int = 0, form: str = "direct") -> torch.Tensor:
    """Runs one of the U-Net family's non-3x3 layers through its HIP kernel: AvgPool2d(2), ConvTranspose2d, Conv2d
    (zero padding, square); raises for anything else so that nothing silently falls back to a torch op.  `form` (CONV_FORMS)
    goes to conv2d / conv_transpose2d; AvgPool2d has one kernel and ignores it."""
    _conv_form(form)
    nn = torch.nn
    if isinstance(m, nn.AvgPool2d):
        k = m.kernel_size if isinstance(m.kernel_size, int) else m.kernel_size[0]
        s_ = m.stride if isinstance(m.stride, int) else m.stride[0]
        if k != 2 or s_ != 2 or m.padding not in (0, (0, 0)):
            raise _lib.DlwpError("only AvgPool2d(2, 2) has a kernel")
        return avgpool2x2(x)
    if isinstance(m, nn.ConvTranspose2d):
        if m.kernel_size[0] != m.kernel_size[1] or m.stride[0] != m.stride[1] or m.padding[0] != m.padding[1] or \
                m.output_padding != (0, 0) or m.dilation != (1, 1) or m.groups != 1:
            raise _lib.DlwpError("ConvTranspose2d: only square kernel / stride / padding without output_padding, dilation, groups")
        return conv_transpose2d(x, m.weight, m.bias, m.stride[0], m.padding[0], act, form=form)
    if isinstance(m, nn.Conv2d):
        if m.kernel_size[0] != m.kernel_size[1] or m.stride[0] != m.stride[1] or m.padding[0] != m.padding[1] or \
                m.dilation != (1, 1) or m.groups != 1 or m.padding_mode != "zeros":
            raise _lib.DlwpError("Conv2d: only square kernel / stride / zero padding without dilation or groups")
        return conv2d(x, m.weight, m.bias, m.stride[0], m.padding[0], act=act, form=form)
    raise _lib.DlwpError(f"no HIP kernel for {type(m).__name__}")


def healpix_pad(x: torch.Tensor, padding: int) -> torch.Tensor:
    """HEALPixPadding(padding) (reference utils/healpix.py:165-368): [(B*12), C, H, W] -> [(B*12), C, H+2p, W+2p]."""
    from . import healpix as _hpx

    _lib.require_cuda_tensor(x, "x")
    x = x.contiguous()
    n, c, h, w = x.shape
    if n % 12:
        raise _lib.DlwpError(f"leading dimension {n} is not (batch * 12 faces)")
    if torch.is_grad_enabled() and x.requires_grad:
        from . import training as _T
        return _T.healpix_pad(x, int(padding))          # HIP forward, backward through the adjoint kernel
    table = _hpx.device_table(h, w, int(padding), x.device)
    y = torch.empty(n, c, h + 2 * padding, w + 2 * padding, device=x.device, dtype=torch.float32)
    _lib.launch("dlwp_healpix_pad_f32", x.device, x, y, table, n, c, h, w, int(padding))
    return y


def healpix_pad_backward(dy: torch.Tensor, padding: int) -> torch.Tensor:
    """Adjoint of healpix_pad: [(B*12), C, H+2p, W+2p] -> [(B*12), C, H, W] through the transposed table
    (dlwp_healpix_pad_bwd_f32)."""
    from . import healpix as _hpx

    _lib.require_cuda_tensor(dy, "dy")
    dy = dy.contiguous()
    p = int(padding)
    n, c, ph, pw = dy.shape
    h, w = ph - 2 * p, pw - 2 * p
    if n % 12:
        raise _lib.DlwpError(f"leading dimension {n} is not (batch * 12 faces)")
    if h <= 0 or h != w:
        raise _lib.DlwpError(f"padded face {ph}x{pw} does not hold a square face with padding {p}")
    adj = _hpx.device_adjoint_table(h, w, p, dy.device)
    dx = torch.empty(n, c, h, w, device=dy.device, dtype=torch.float32)
    _lib.launch("dlwp_healpix_pad_bwd_f32", dy.device, dy, dx, adj.indptr, adj.index, adj.weight, n, c, h, w, p)
    return dx


def healpix_to_latlon(x: torch.Tensor, lats_deg, lons_deg, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """HEALPix fields [..., 12, n, n] -> lat-lon fields [..., H, W] at (lats_deg[j], lons_deg[i]) by the HEALPix library's
    bilinear interpolation (dlwp_healpix_to_latlon_f32; the reference: HEALPixRemap.hpx2ll, healpix_mapping.py:372-404, per plane
    on the host).  `healpix.reference_grid(H, W)` gives the grid hpx2ll itself produces.  `out`: a contiguous float32
    [..., H, W] tensor on the same device to write into (the metric classes' reused workspace); it is returned."""
    from . import healpix as _hpx

    _lib.require_cuda_tensor(x, "x")
    if x.dim() < 3 or x.shape[-3] != 12:
        raise _lib.DlwpError(f"expected HEALPix fields [..., 12, n, n], got shape {tuple(x.shape)}")
    n = int(x.shape[-1])
    if x.shape[-2] != n:
        raise _lib.DlwpError(f"HEALPix faces are square, got {x.shape[-2]}x{n}")
    if n < 2 or n & (n - 1):
        raise _lib.DlwpError(f"nside must be a power of two >= 2, got {n}")
    table = _hpx.device_latlon_table(n, lats_deg, lons_deg, x.device)
    lead = tuple(x.shape[:-3])
    planes = math.prod(lead)
    h = len(lats_deg)
    cells = int(table.index.shape[0])
    shape = lead + (h, cells // h)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    elif (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != x.device
          or not out.is_contiguous()):
        raise _lib.DlwpError(f"out must be a contiguous float32 {shape} tensor on {x.device}")
    if planes:
        _lib.launch("dlwp_healpix_to_latlon_f32", x.device, x.contiguous(), table.index, table.weight, out, planes, n, cells)
    return out


# orbital constants of add_insolation.py:34-41 ("year 1995")
_INSOL_EPS = 23.4441 * math.pi / 180.0      # obliquity
_INSOL_ECC = 0.016715                       # eccentricity
_INSOL_OM = 282.7 * math.pi / 180.0         # longitude of the perihelion


def insolation_day_of_year(dates):
    """float64 [T]: days since the start of each date's year (add_insolation.py:44-45).  `dates`: anything numpy.datetime64
    takes (strings, datetime, datetime64 arrays)."""
    import numpy as np

    d = np.asarray(dates, dtype="datetime64[us]").reshape(-1)
    return (d - d.astype("datetime64[Y]").astype("datetime64[us]")) / np.timedelta64(1, "D")


def insolation_date_table(dates, daily: bool = False):
    """float64 numpy [T, 5]: sin dec, cos dec, rho^-2, cos 2 pi frac(day), sin 2 pi frac(day) of every date
    (add_insolation.py:55-64).  daily=True: the day is 0.5 + round(day) (:49-50)."""
    import numpy as np

    days = insolation_day_of_year(dates)
    if daily:
        days = 0.5 + np.round(days)
    beta = math.sqrt(1.0 - _INSOL_ECC ** 2)
    lambda_m = _INSOL_ECC * (1.0 + beta) * math.sin(_INSOL_OM) + 2.0 * np.pi * (days - 80.5) / 365.0
    lambda_ = lambda_m + 2.0 * _INSOL_ECC * np.sin(lambda_m - _INSOL_OM)
    sin_dec = math.sin(_INSOL_EPS) * np.sin(lambda_)
    rho = (1.0 - _INSOL_ECC ** 2) / (1.0 + _INSOL_ECC * np.cos(lambda_ - _INSOL_OM))
    day_angle = 2.0 * np.pi * (days - np.floor(days))
    return np.ascontiguousarray(np.stack([sin_dec, np.cos(np.arcsin(sin_dec)), rho ** -2.0, np.cos(day_angle), np.sin(day_angle)],
                                         axis=1))


def _insolation_grid(lat_deg, lon_deg):
    import numpy as np

    def f64(a):
        return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)

    lat, lon = f64(lat_deg), f64(lon_deg)
    if lat.ndim != lon.ndim:
        raise _lib.DlwpError("insolation: lat and lon must have the same number of dimensions")
    if lat.ndim != 1 and lat.shape != lon.shape:
        raise _lib.DlwpError(f"insolation: shape mismatch between lat {lat.shape} and lon {lon.shape}")
    return lat, lon


def insolation_point_table(lat_deg, lon_deg, daily: bool = False):
    """(float64 numpy [N, 4], grid shape): sin lat, cos lat, cos 2 pi l, sin 2 pi l of every point with
    l = float32(lon) / float32(360) -- the reference divides the longitude in float32 before it promotes
    (add_insolation.py:54, :62), and so does this.  1-D `lat_deg` [H] and `lon_deg` [W] are a mesh (grid [H, W], :30-31);
    otherwise they are equal-shape per-cell arrays.  daily=True: the longitude is 0 everywhere (:51-52)."""
    import numpy as np

    lat, lon = _insolation_grid(lat_deg, lon_deg)
    if lat.ndim == 1:
        lon, lat = np.meshgrid(lon, lat)
    lon32 = np.zeros(lon.shape, dtype=np.float32) if daily else lon.astype(np.float32)
    lat_r = (np.pi / 180.0 * lat).reshape(-1)
    lon_angle = 2.0 * np.pi * (lon32 / np.float32(360.0)).astype(np.float64).reshape(-1)
    table = np.stack([np.sin(lat_r), np.cos(lat_r), np.cos(lon_angle), np.sin(lon_angle)], axis=1)
    return np.ascontiguousarray(table), tuple(lat.shape)


def insolation_tables(dates, lat_deg, lon_deg, daily: bool = False):
    """The host half of `insolation`, float64 numpy: (date table [T, 5], point table [N, 4], grid shape)."""
    table, grid = insolation_point_table(lat_deg, lon_deg, daily)
    return insolation_date_table(dates, daily), table, grid


_INSOL_POINTS = {}        # (lat bytes, lon bytes, daily, device) -> (device point table, grid shape); the last few grids
_INSOL_POINTS_KEPT = 8


def _insolation_points_on(lat_deg, lon_deg, daily: bool, device):
    """The point table on `device`, made and uploaded once per grid: a rollout asks for the same grid chunk after chunk"""
    lat, lon = _insolation_grid(lat_deg, lon_deg)
    key = (lat.shape, lat.tobytes(), lon.shape, lon.tobytes(), bool(daily), str(device))
    hit = _INSOL_POINTS.pop(key, None)
    if hit is None:
        table, grid = insolation_point_table(lat, lon, daily)
        hit = (torch.from_numpy(table).to(device), grid)
        while len(_INSOL_POINTS) >= _INSOL_POINTS_KEPT:
            _INSOL_POINTS.pop(next(iter(_INSOL_POINTS)))
    _INSOL_POINTS[key] = hit                                   # most recently used last
    return hit


def insolation(dates, lat_deg, lon_deg, S: float = 1.0, daily: bool = False, clip_zero: bool = True, mean: Optional[float] = None,
               std: Optional[float] = None, out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """Top-of-atmosphere insolation for `dates` on a grid, float32 [T, *grid] on the device (dlwp_insolation_f32; reference
    data/datasets/add_insolation.py:9-73, the generator of the prescribed variable `tisr`).  1-D `lat_deg` / `lon_deg` are a mesh
    ([T, H, W]); equal-shape arrays are per-cell coordinates (`healpix.cell_centres(n)` gives [T, 12, n, n]).  The host
    tabulates the per-date and per-point factors in float64 (`insolation_tables`; the point table is uploaded once per grid
    and kept, the date table -- 40 bytes a date -- goes up per call), the kernel forms the separable product in fp64 and rounds
    once.  `mean` / `std`: the dataset's normalisation (x - mean) / std
    (datasets.py:371) applied in the same pass.  `out`: a contiguous float32 [T, *grid] device tensor to write into (it is
    returned); otherwise the result is allocated on `device` (default: the current device)."""
    if out is not None:
        _lib.require_cuda_tensor(out, "out")
    dev = out.device if out is not None else (torch.device("cuda", torch.cuda.current_device()) if device is None
                                              else torch.device(device))
    date_tab = insolation_date_table(dates, daily)
    pt, grid = _insolation_points_on(lat_deg, lon_deg, daily, dev)
    t, n = date_tab.shape[0], int(pt.shape[0])
    shape = (t,) + grid
    if (mean is None) != (std is None):
        raise _lib.DlwpError("insolation: give both mean and std, or neither")
    if std is not None and float(std) == 0.0:
        raise _lib.DlwpError("insolation: std must be non-zero")
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.float32)
    elif tuple(out.shape) != shape or not out.is_contiguous():
        raise _lib.DlwpError(f"out must be a contiguous float32 {shape} tensor")
    if t == 0 or n == 0:
        return out
    dt = torch.from_numpy(date_tab).to(dev, non_blocking=True)
    _lib.launch("dlwp_insolation_f32", out.device, dt, pt, out, t, n, float(S), int(bool(clip_zero)), int(std is not None),
                float(mean) if mean is not None else 0.0, float(std) if std is not None else 1.0)
    return out


def conv3x3_hpx_backward_data(dy: torch.Tensor, weight: torch.Tensor, cin: int) -> torch.Tensor:
    """Gradient of HEALPixPadding(1) + Conv2d(3x3, padding 0) with respect to its (activated, concatenated) input:
    dy [(B*12), Cout, H, W], weight [Cout, cin, 3, 3] in the forward layout -> [(B*12), cin, H, W]
    (dlwp_conv3x3_hpx_bwd_data_f32)."""
    from . import healpix as _hpx

    _lib.require_cuda_tensor(dy, "dy")
    _lib.require_cuda_tensor(weight, "weight")
    dy = dy.contiguous()
    weight = weight.contiguous()
    n, cout, h, w = dy.shape
    if n % 12:
        raise _lib.DlwpError(f"leading dimension {n} is not (batch * 12 faces)")
    if tuple(weight.shape) != (cout, int(cin), 3, 3):
        raise _lib.DlwpError(f"weight {tuple(weight.shape)} does not match {cout} output, {cin} input channels, 3x3")
    adj = _hpx.device_adjoint_table(h, w, 1, dy.device)
    dx = torch.empty(n, int(cin), h, w, device=dy.device, dtype=torch.float32)
    nbytes = _lib.load().dlwp_conv3x3_hpx_bwd_data_workspace_bytes(n, h, w, int(cin))
    ring = _lib.workspace(max(nbytes, 4), dy.device)
    _lib.launch("dlwp_conv3x3_hpx_bwd_data_f32", dy.device, dy, weight, dx, n, h, w, int(cin), cout, adj.indptr, adj.index,
                adj.weight, ring, nbytes)
    return dx


def conv3x3_weight_grad_supported(batch: int, c0: int, c1: int, cout: int, h: int, w: int, hpx: bool = False) -> bool:
    """whether dlwp_conv3x3_wgrad_f32 takes the shape (its envelope: include/dlwp_hip.h); needs the library, not a GPU"""
    if min(int(batch), int(c0), int(cout), int(h), int(w)) < 1 or int(c1) < 0 or (hpx and (int(batch) % 12 or h != w)):
        return False
    if max(int(batch), int(c0), int(c1), int(cout), int(h), int(w)) >= 1 << 31:
        return False
    return _lib.load().dlwp_conv3x3_wgrad_workspace_bytes(int(batch), int(h), int(w), int(c0) + int(c1), int(cout)) > 0


def conv3x3_weight_grad(x0: torch.Tensor, x1: Optional[torch.Tensor], dz: torch.Tensor, pre_act: int = 0, hpx: bool = False,
                        need_bias: bool = True):
    """Weight and bias gradient of pad(1) + Conv2d(3x3) on cat([x0, x1], 1) (conv3x3's arguments) from dz [N, cout, H, W], the
    gradient of the convolution's output: (dw [cout, c0+c1, 3, 3], db [cout] or None) on dlwp_conv3x3_wgrad_f32.  The input is
    read the way the forward reads it -- segments, `pre_act` and the padding rule applied at load, no copies.  Runs on the
    current stream without a host synchronisation; reruns are bitwise identical."""
    for t, name in ((x0, "x0"), (x1, "x1"), (dz, "dz")):
        _lib.require_cuda_tensor(t, name)
    x0 = x0.contiguous()
    x1 = x1.contiguous() if x1 is not None else None
    dz = dz.contiguous()
    if x0.dim() != 4 or dz.dim() != 4:
        raise _lib.DlwpError(f"conv3x3_weight_grad: x0 {tuple(x0.shape)} and dz {tuple(dz.shape)} must be [N, C, H, W]")
    n, c0, h, w = x0.shape
    c1 = x1.shape[1] if x1 is not None else 0
    cout = dz.shape[1]
    if x1 is not None and (x1.dim() != 4 or tuple(x1.shape) != (n, c1, h, w)):
        raise _lib.DlwpError(f"conv3x3_weight_grad: x1 {tuple(x1.shape)} does not match x0 {tuple(x0.shape)}")
    if tuple(dz.shape) != (n, cout, h, w):
        raise _lib.DlwpError(f"conv3x3_weight_grad: dz {tuple(dz.shape)} does not match the input {(n, c0 + c1, h, w)}")
    table = None
    if hpx:
        from . import healpix as _hpx

        if n % 12:
            raise _lib.DlwpError(f"leading dimension {n} is not (batch * 12 faces)")
        table = _hpx.device_table(h, w, 1, x0.device)
    lib = _lib.load()
    nbytes = int(lib.dlwp_conv3x3_wgrad_workspace_bytes(n, h, w, c0 + c1, cout)) if max(n, c0, c1, cout, h, w) < 1 << 31 else 0
    if nbytes == 0 or (hpx and h != w):       # the one query gives the envelope (conv3x3_weight_grad_supported) and the size
        raise _lib.DlwpError(f"conv3x3_weight_grad: no HIP kernel for {c0}+{c1} -> {cout} channels on {n} x {h} x {w}")
    dw = torch.empty(cout, c0 + c1, 3, 3, device=x0.device, dtype=torch.float32)
    db = torch.empty(cout, device=x0.device, dtype=torch.float32) if need_bias else None
    ws = _lib.workspace(nbytes, x0.device)
    _lib.launch("dlwp_conv3x3_wgrad_f32", x0.device, x0, c0, x1, c1, dz, dw, db, n, h, w, cout, int(pre_act), table, ws, nbytes)
    return dw, db


def _conv2d_out_hw(h: int, w: int, k: int, stride: int, padding: int, transposed: bool):
    if transposed:
        return (h - 1) * stride - 2 * padding + k, (w - 1) * stride - 2 * padding + k
    return (h + 2 * padding - k) // stride + 1, (w + 2 * padding - k) // stride + 1


def conv2d_weight_grad_supported(batch: int, cin: int, cout: int, h: int, w: int, k: int, stride: int, padding: int,
                                 transposed: bool = False) -> bool:
    """whether dlwp_conv2d_wgrad_f32 takes the layer (its envelope: include/dlwp_hip.h); needs the library, not a GPU"""
    args = [int(v) for v in (batch, cin, h, w, cout, k, stride, padding)]
    if min(args[:7]) < 1 or args[7] < 0 or max(args) >= 1 << 31:
        return False
    return _lib.load().dlwp_conv2d_wgrad_workspace_bytes(*args, int(bool(transposed))) > 0


def conv2d_weight_grad(x: torch.Tensor, grad_z: torch.Tensor, k: int, stride: int, padding: int, pre_act: int = 0,
                       transposed: bool = False, need_weight: bool = True, need_bias: bool = True):
    """Weight and bias gradient of conv2d (transposed: of conv_transpose2d) with a k x k kernel from the layer's input
    x [N, cin, H, W] and grad_z [N, cout, OH, OW], the gradient of the layer's output before its activation:
    (dw [cout, cin, k, k] -- transposed [cin, cout, k, k] --, db [cout]), None where not wanted, on dlwp_conv2d_wgrad_f32.
    Both maps are read where they lie, `pre_act` applied to x at load (the transposed layer has none); no copies.  Runs on
    the current stream without a host synchronisation; reruns are bitwise identical."""
    for t, name in ((x, "x"), (grad_z, "grad_z")):
        _lib.require_cuda_tensor(t, name)
    x, dz = x.contiguous(), grad_z.contiguous()
    k, stride, padding, transposed = int(k), int(stride), int(padding), bool(transposed)
    if x.dim() != 4 or dz.dim() != 4:
        raise _lib.DlwpError(f"conv2d_weight_grad: x {tuple(x.shape)} and grad_z {tuple(dz.shape)} must be [N, C, H, W]")
    if transposed and int(pre_act) != 0:
        raise _lib.DlwpError("conv2d_weight_grad: the transposed layer has no pre-activation")
    n, cin, h, w = x.shape
    cout = dz.shape[1]
    lib = _lib.load()
    nbytes = 0
    if min(n, cin, cout, h, w, k, stride) >= 1 and padding >= 0 and max(n, cin, cout, h, w, k, stride, padding) < 1 << 31:
        nbytes = int(lib.dlwp_conv2d_wgrad_workspace_bytes(n, cin, h, w, cout, k, stride, padding, int(transposed)))
    if nbytes == 0:                 # the one query gives the envelope (conv2d_weight_grad_supported) and the size
        raise _lib.DlwpError(f"conv2d_weight_grad: no HIP kernel for {cin} -> {cout} channels on {n} x {h} x {w}, k={k} "
                             f"stride={stride} padding={padding} transposed={transposed}")
    if tuple(dz.shape) != (n, cout, *_conv2d_out_hw(h, w, k, stride, padding, transposed)):
        raise _lib.DlwpError(f"conv2d_weight_grad: grad_z {tuple(dz.shape)} is not the output map of x {tuple(x.shape)} under "
                             f"k={k} stride={stride} padding={padding} transposed={transposed}")
    dw = db = None
    if need_weight:
        dw = torch.empty((cin, cout, k, k) if transposed else (cout, cin, k, k), device=x.device, dtype=torch.float32)
    if need_bias:
        db = torch.empty(cout, device=x.device, dtype=torch.float32)
    if dw is None and db is None:
        return None, None
    ws = _lib.workspace(nbytes, x.device)
    _lib.launch("dlwp_conv2d_wgrad_f32", x.device, x, dz, dw, db, n, cin, h, w, cout, k, stride, padding, int(pre_act),
                int(transposed), ws, nbytes)
    return dw, db


def convlstm_gates(gates: torch.Tensor, c_prev: torch.Tensor):
    """The ConvLSTM cell update (convlstm.py:96-109): gates [B, 4*hid, H, W] = (netin, i, f, o) before their activations and
    c_prev [B, hid, H, W] -> (h, c), one dlwp_convlstm_gates_f32 launch.  With a gradient wanted: training.convlstm_gates,
    this kernel forward and dlwp_convlstm_gates_bwd_f32 backward."""
    _lib.require_cuda_tensor(gates, "gates")
    _lib.require_cuda_tensor(c_prev, "c_prev")
    if torch.is_grad_enabled() and (gates.requires_grad or c_prev.requires_grad):
        from . import training as _T
        return _T.convlstm_gates(gates, c_prev)
    gates, c_prev = gates.contiguous(), c_prev.contiguous()
    b, c4, h, w = gates.shape
    hid = c4 // 4
    h_out, c_out = torch.empty_like(c_prev), torch.empty_like(c_prev)
    _lib.launch("dlwp_convlstm_gates_f32", gates.device, gates, c_prev, h_out, c_out, b, hid, h, w)
    return h_out, c_out


def convlstm_gates_backward(gates: torch.Tensor, c_prev: torch.Tensor, dh: Optional[torch.Tensor], dc: Optional[torch.Tensor],
                            need_c_prev: bool = True):
    """The backward of convlstm_gates from its inputs alone (dlwp_convlstm_gates_bwd_f32: the activations are recomputed with
    the forward's arithmetic, nothing activated is saved): (dgates [B, 4*hid, H, W], dc_prev [B, hid, H, W] or None when
    need_c_prev is false).  dh, dc [B, hid, H, W] are the gradients of h and c; either may be None (a zero gradient, not
    read), not both.  One launch on the current stream, no host synchronisation; reruns are bitwise identical."""
    for t, name in ((gates, "gates"), (c_prev, "c_prev"), (dh, "dh"), (dc, "dc")):
        _lib.require_cuda_tensor(t, name)
    if dh is None and dc is None:
        raise _lib.DlwpError("convlstm_gates_backward: neither dh nor dc given")
    gates, c_prev = gates.contiguous(), c_prev.contiguous()
    if gates.dim() != 4 or gates.shape[1] % 4 or tuple(c_prev.shape) != (gates.shape[0], gates.shape[1] // 4, *gates.shape[2:]):
        raise _lib.DlwpError(f"convlstm_gates_backward: gates {tuple(gates.shape)} must be [B, 4*hid, H, W] and c_prev "
                             f"{tuple(c_prev.shape)} [B, hid, H, W]")
    for t, name in ((dh, "dh"), (dc, "dc")):
        if t is not None and t.shape != c_prev.shape:
            raise _lib.DlwpError(f"convlstm_gates_backward: {name} {tuple(t.shape)} is not c_prev's {tuple(c_prev.shape)}")
    dh = dh.contiguous() if dh is not None else None
    dc = dc.contiguous() if dc is not None else None
    b, c4, h, w = gates.shape
    dgates = torch.empty_like(gates)
    dc_prev = torch.empty_like(c_prev) if need_c_prev else None
    if dgates.numel():
        _lib.launch("dlwp_convlstm_gates_bwd_f32", gates.device, gates, c_prev, dh, dc, dgates, dc_prev, b, c4 // 4, h, w)
    return dgates, dc_prev


def afno2d_mix(xf_cf: torch.Tensor, w1, b1, w2, b2, num_blocks: int, sparsity_threshold: float,
               hard_thresholding_fraction: float) -> torch.Tensor:
    """xf_cf complex64 CHANNELS-FIRST [B, C, H, Wf] (rfft2 of a [B, C, H, W] tensor) -> mixed spectrum,
    same shape and layout."""
    if not xf_cf.is_cuda or xf_cf.dtype != torch.complex64:
        raise _lib.DlwpError("afno2d_mix needs a complex64 CUDA tensor")
    xc = xf_cf.contiguous()
    b, c, h, wf = xc.shape
    xr = torch.view_as_real(xc)
    yr = torch.empty_like(xr)
    _lib.launch("dlwp_afno2d_mix_f32", xc.device, xr, yr, w1.contiguous(), b1.contiguous(), w2.contiguous(), b2.contiguous(), b,
                h, wf, c, num_blocks, float(sparsity_threshold), float(hard_thresholding_fraction))
    return torch.view_as_complex(yr)


class _Fft2Plans:
    """hipFFT plan pairs (R2C + C2R) per (device, batch, H, W), created on first use and kept for the process."""

    def __init__(self):
        self._plans = {}

    def get(self, device, batch: int, h: int, w: int):
        key = (str(device), batch, h, w)
        if key not in self._plans:
            lib = _lib.load()
            handle = ctypes.c_void_p()
            with torch.cuda.device(device):
                _lib.check(lib.dlwp_fft2_plan_create(ctypes.byref(handle), batch, h, w), "dlwp_fft2_plan_create")
            self._plans[key] = handle
        return self._plans[key]


_fft2_plans = _Fft2Plans()


class _AfnoFftPlans:
    """twiddle tables of the hand-written kept-column FFTs per (device, H, W, kept columns)"""

    def __init__(self):
        self._plans = {}

    def get(self, device, h: int, w: int, kc: int):
        key = (str(device), h, w, kc)
        if key not in self._plans:
            handle = ctypes.c_void_p()
            _lib.launch("dlwp_afno_fft_plan_create", device, ctypes.byref(handle), h, w, kc)
            self._plans[key] = handle
        return self._plans[key]


_afno_fft_plans = _AfnoFftPlans()


def afno_kept_cols(h: int, w: int, hard_thresholding_fraction: float) -> int:
    """columns of the half spectrum the filter keeps: fourcastnet.py:93-94 (`total_modes = H // 2 + 1` -- the
    reference takes it from the FIRST spatial axis -- `kept_modes = int(total_modes * fraction)`, columns [:kept])"""
    return max(0, min(int((h // 2 + 1) * hard_thresholding_fraction), w // 2 + 1))


def afno2d_filter_backward(x_cf: torch.Tensor, grad_y: torch.Tensor, w1, b1, w2, b2, num_blocks: int,
                           sparsity_threshold: float, hard_thresholding_fraction: float):
    """Gradients of afno2d_filter_cf with respect to (x_cf, w1, b1, w2, b2), or None when the grid is not one of the
    hand-written kept-column transforms / the block size is not 4, 8 or 16 (the caller then differentiates the torch form).
    grad_x = C2R(mix_bwd(R2C(x), R2C(grad_y))): the same two hand-written transforms as the forward around
    dlwp_afno2d_mix_bwd_f32 (which recomputes the per-point MLP); the weight gradients are sums over the spectrum points of
    per-point factors the kernel writes -- four complex einsums (reference backward: train.py:271 through fourcastnet.py:85-124)."""
    _lib.require_cuda_tensor(x_cf, "x_cf")
    _lib.require_cuda_tensor(grad_y, "grad_y")
    x_cf, grad_y = x_cf.contiguous(), grad_y.contiguous()
    b, c, h, w = x_cf.shape
    lib = _lib.load()
    kc = afno_kept_cols(h, w, hard_thresholding_fraction)
    bs = c // num_blocks
    if kc < 1 or not lib.dlwp_afno_fft_supported(h, w, kc) or bs not in (4, 8, 16):
        return None
    scale = 1.0 / float(h * w) ** 0.5
    dev = x_cf.device
    plan = _afno_fft_plans.get(dev, h, w, kc)
    mk = lambda: torch.empty(b, c, h, kc, 2, device=dev, dtype=torch.float32)
    xf, gf, gxf, xin, o1, d1, d2 = mk(), mk(), mk(), mk(), mk(), mk(), mk()
    _lib.launch("dlwp_afno_rfft2_kept_f32", dev, plan, x_cf, xf, b * c)
    _lib.launch("dlwp_afno_rfft2_kept_f32", dev, plan, grad_y, gf, b * c)
    _lib.launch("dlwp_afno2d_mix_bwd_f32", dev, xf, gf, gxf, xin, o1, d1, d2, *(t.detach().contiguous() for t in (w1, b1, w2, b2)),
                b, h, kc, c, num_blocks, w, float(sparsity_threshold), float(hard_thresholding_fraction), scale, scale)
    gx = torch.empty_like(x_cf)
    _lib.launch("dlwp_afno_irfft2_kept_f32", dev, plan, gxf, gx, b * c)
    cv = lambda t: torch.view_as_complex(t).view(b, num_blocks, bs, h, kc)
    gw1 = torch.einsum("bnihk,bnohk->nio", cv(xin).conj(), cv(d1))
    gw2 = torch.einsum("bnihk,bnohk->nio", cv(o1).conj(), cv(d2))
    gb1 = cv(d1).sum(dim=(0, 3, 4))
    gb2 = cv(d2).sum(dim=(0, 3, 4))
    ri = lambda t: torch.stack([t.real, t.imag], dim=0).contiguous()       # reference layout [2, nb, bs(, bs)]
    return gx, ri(gw1), ri(gb1), ri(gw2), ri(gb2)


def afno2d_filter_cf(x_cf: torch.Tensor, w1, b1, w2, b2, num_blocks: int, sparsity_threshold: float,
                     hard_thresholding_fraction: float, use_rocfft: bool = False) -> torch.Tensor:
    """irfft2(mix(rfft2(x_cf, norm="ortho")), norm="ortho") for CHANNELS-FIRST x_cf [B, C, H, W]
    (fourcastnet.py:87-123 without the `+ bias` of :127).  Three launches: the hand-written forward transform that
    produces only the kept columns, the mixing kernel in place on that [B, C, H, kept] spectrum (it carries the two
    1/sqrt(HW) factors of norm="ortho"), the hand-written inverse transform.  Grids that are not instantiated (and
    use_rocfft=True, the cross-check) take the hipFFT path on the full half spectrum."""
    _lib.require_cuda_tensor(x_cf, "x_cf")
    from . import training as _T
    if _T.wants_grad(x_cf, w1, b1, w2, b2):
        return _T.afno_filter(x_cf, w1, b1, w2, b2, num_blocks, sparsity_threshold, hard_thresholding_fraction)
    x_cf = x_cf.contiguous()
    b, c, h, w = x_cf.shape
    lib = _lib.load()
    scale = 1.0 / float(h * w) ** 0.5
    kc = afno_kept_cols(h, w, hard_thresholding_fraction)
    y = torch.empty_like(x_cf)
    dev = x_cf.device
    kept = not use_rocfft and kc >= 1 and lib.dlwp_afno_fft_supported(h, w, kc)
    cols = kc if kept else w // 2 + 1           # the kept columns, or hipFFT's full half spectrum
    spec = torch.empty(b, c, h, cols, 2, device=dev, dtype=torch.float32)
    if kept:
        plan = _afno_fft_plans.get(dev, h, w, kc)
        _lib.launch("dlwp_afno_rfft2_kept_f32", dev, plan, x_cf, spec, b * c)
    else:
        plan = _fft2_plans.get(dev, b * c, h, w)
        _lib.launch("dlwp_rfft2_f32", dev, plan, x_cf, spec)
    _lib.launch("dlwp_afno2d_mix_scaled_f32", dev, spec, spec, w1.contiguous(), b1.contiguous(), w2.contiguous(), b2.contiguous(),
                b, h, cols, c, num_blocks, float(sparsity_threshold), float(hard_thresholding_fraction), scale, scale)
    if kept:
        _lib.launch("dlwp_afno_irfft2_kept_f32", dev, plan, spec, y, b * c)
    else:
        _lib.launch("dlwp_irfft2_f32", dev, plan, spec, y)
    return y


def layernorm_nhwc_to_nchw(x: torch.Tensor, weight, bias, eps: float) -> torch.Tensor:
    """x [B, H, W, C] -> LayerNorm over C, returned channels-first [B, C, H, W]."""
    _lib.require_cuda_tensor(x, "x")
    x = x.contiguous()
    b, h, w, c = x.shape
    y = torch.empty(b, c, h, w, device=x.device, dtype=torch.float32)
    _lib.launch("dlwp_layernorm_nhwc_to_nchw_f32", x.device, x, weight.contiguous(), bias.contiguous(), y, b, h * w, c, float(eps))
    return y


def afno_merge(f_nchw: torch.Tensor, l_nchw: torch.Tensor, x_nhwc: torch.Tensor, weight, bias, eps: float,
               sum_bias: Optional[torch.Tensor] = None, want_norm: bool = True):
    """(f + l) transposed to token-major + x -> (sum [+ sum_bias], LayerNorm(sum)), both [B, H, W, C].
    want_norm=False returns (sum, None): for a consumer that normalises on the fly (token_mlp(ln_eps=...))."""
    for t, n in ((f_nchw, "f"), (l_nchw, "l"), (x_nhwc, "x")):
        _lib.require_cuda_tensor(t, n)
    f_nchw, l_nchw, x_nhwc = f_nchw.contiguous(), l_nchw.contiguous(), x_nhwc.contiguous()
    b, h, w, c = x_nhwc.shape
    s = torch.empty_like(x_nhwc)
    n = torch.empty_like(x_nhwc) if want_norm else None
    gamma, beta = (weight.contiguous(), bias.contiguous()) if want_norm else (None, None)
    _lib.launch("dlwp_afno_merge_f32", x_nhwc.device, f_nchw, l_nchw, x_nhwc, gamma, beta, _contig(sum_bias), s, n, b, h * w, c,
                float(eps))
    return s, n


def patch_embed_1x1_supported(in_channels: int, channels: int) -> bool:
    return in_channels <= 32 and 4 <= channels <= 256 and channels % 4 == 0


def patch_embed_1x1(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                    pos: Optional[torch.Tensor]) -> torch.Tensor:
    """x [B, Cin, H, W], weight [C, Cin, 1, 1] (Conv2d with 1x1 patches), pos [H*W, C] or None ->
    tokens [B, H*W, C] = conv(x).flatten(2).transpose(1, 2) + pos   (fourcastnet.py:530-543, :286-288)."""
    _lib.require_cuda_tensor(x, "x")
    x = x.contiguous()
    b, cin, h, w = x.shape
    c = weight.shape[0]
    if pos is not None and (tuple(pos.shape) != (h * w, c) or not pos.is_contiguous()):
        raise _lib.DlwpError(f"patch embed: pos must be contiguous [{h * w}, {c}], got {tuple(pos.shape)}")
    out = torch.empty(b, h * w, c, device=x.device, dtype=torch.float32)
    _lib.launch("dlwp_patch_embed_1x1_f32", x.device, x, weight.contiguous(), _contig(bias), pos, out, b, cin, h * w, c)
    return out


def concat_channels(parts: Sequence[torch.Tensor]) -> torch.Tensor:
    """torch.cat(parts, dim=1) for [B, Ci, H, W] float32 tensors whose (Ci, H, W) block is contiguous (any batch stride: views into the
    inputs and the trajectory buffer) -- `_prepare_inputs` of the rollout loop (swin_transformer.py:679-692) as one 16-byte copy kernel.
    Parts the kernel does not take (other dtypes, inner strides, > 8 parts, plane not a multiple of 4) go through torch.cat: the same
    copy, written by torch."""
    parts = list(parts)
    p0 = parts[0]
    b, h, w = p0.shape[0], p0.shape[2], p0.shape[3]
    plane = h * w
    ok = 2 <= len(parts) <= 8 and plane % 4 == 0 and b <= 65535        # (one part: torch's copy is one call with less host work)
    for t in parts:
        ok = ok and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[0] == b and tuple(t.shape[2:]) == (h, w) \
            and t.stride(3) == 1 and t.stride(2) == w and t.stride(1) == plane and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0
    if not ok:
        return torch.cat(parts, dim=1)
    n = len(parts)
    ctot = sum(int(t.shape[1]) for t in parts)
    out = torch.empty(b, ctot, h, w, device=p0.device, dtype=torch.float32)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in parts])
    chans = (ctypes.c_int32 * n)(*[int(t.shape[1]) for t in parts])
    strides = (ctypes.c_int64 * n)(*[int(t.stride(0)) for t in parts])
    _lib.launch("dlwp_concat_channels_f32", p0.device, ptrs, chans, strides, n, out, b, plane)
    return out


def patch_recover_1x1_supported(channels: int, out_channels: int) -> bool:
    return channels % 4 == 0 and channels <= 256 and 0 < out_channels <= 16


def patch_recover_1x1(tokens: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], h: int, w: int) -> torch.Tensor:
    """tokens [B, H, W, C] (or [B, H*W, C]) token-major, weight [Cout, C] (the head Linear of a 1x1-patch backbone) ->
    [B, Cout, H, W] = head(tokens) rearranged "b h w c -> b c h w"   (fourcastnet.py:144, :296-303)."""
    _lib.require_cuda_tensor(tokens, "tokens")
    tokens = tokens.contiguous()
    b, c = tokens.shape[0], tokens.shape[-1]
    cout = weight.shape[0]
    if tokens.numel() != b * h * w * c:
        raise _lib.DlwpError(f"patch recover: tokens {tuple(tokens.shape)} do not hold {h} x {w} tokens per sample")
    out = torch.empty(b, cout, h, w, device=tokens.device, dtype=torch.float32)
    _lib.launch("dlwp_patch_recover_1x1_f32", tokens.device, tokens, weight.detach().contiguous(), _contig(bias), out, b, h * w, c,
                cout)
    return out


def token_mlp_supported(channels: int, hidden: int) -> bool:
    """True when dlwp_token_mlp_f32 handles this (channels, hidden) pair."""
    return int(_lib.load().dlwp_token_mlp_packed_bytes(int(channels), int(hidden))) > 0


class TokenMlpWeights:
    """fc1 / fc2 weights of a token MLP in the operand layout of dlwp_token_mlp_f32, re-packed on the device
    whenever a parameter has been written to (optimizer step, load_state_dict, .to()).  With `ln_weight` / `ln_bias`
    (and `b1`) the affine part of the LayerNorm in front of fc1 is folded into the operands, for token_mlp(ln_eps=...)."""

    def __init__(self):
        self._derived = Derived()

    def get(self, w1: torch.Tensor, w2: torch.Tensor, ln_weight: Optional[torch.Tensor] = None,
            ln_bias: Optional[torch.Tensor] = None, b1: Optional[torch.Tensor] = None, merged: bool = False,
            f16x3: bool = False) -> torch.Tensor:
        """merged=True: the k-slot order afno_block_tail wants (a different permutation of W1's columns);
        f16x3=True: the two f16 images of the f16x3 product form (afno_block_tail(form="f16x3"))."""
        def build():
            hid, c = w1.shape
            if tuple(w2.shape) != (c, hid):
                raise _lib.DlwpError(f"token MLP: fc2.weight {tuple(w2.shape)} does not match fc1.weight {tuple(w1.shape)}")
            if (ln_weight is None) != (ln_bias is None):
                raise _lib.DlwpError("token MLP: LayerNorm weight and bias must be given together")
            lib = _lib.load()
            nbytes = int(lib.dlwp_token_mlp_packed_bytes(c, hid))
            if nbytes == 0:
                raise _lib.DlwpError(f"token MLP: unsupported shape channels={c} hidden={hid}")
            buf = torch.empty(nbytes // 4, dtype=torch.int32, device=w1.device)
            _lib.launch("dlwp_token_mlp_pack_f16x3" if f16x3 else "dlwp_token_mlp_pack_f32", w1.device,
                        *(_contig(t) for t in (w1, w2, ln_weight, ln_bias, b1)), c, hid, 1 if merged else 0, buf)
            return buf

        return self._derived.get(source_key(w1, w2, ln_weight, ln_bias, b1, extra=(merged, f16x3)), build)


def token_mlp(n: torch.Tensor, resid: Optional[torch.Tensor], packed: torch.Tensor, b1: Optional[torch.Tensor],
              b2: Optional[torch.Tensor], hidden: int, out: Optional[torch.Tensor] = None,
              ln_eps: Optional[float] = None, emit_norm=None):
    """out = resid + b2 + fc2(gelu(fc1(n)))  over the last dimension (fourcastnet.py:41-57, :191-192), one launch.
    With `ln_eps` the kernel first LayerNorms `n` (packed must carry the folded affine part and fc1 bias, see
    TokenMlpWeights.get; b1 is then unused).  `out` may be `resid` / `n` itself (in place).
    emit_norm = (weight, bias, eps) of the NEXT block's first LayerNorm: n must be [B, H, W, C]; returns
    (out, LayerNorm(out) channels-first [B, C, H, W]) -- the next block's `layernorm_nhwc_to_nchw` for free."""
    _lib.require_cuda_tensor(n, "n")
    n = n.contiguous()
    c = n.shape[-1]
    if resid is not None:
        _lib.require_cuda_tensor(resid, "resid")
        if resid.shape != n.shape or not resid.is_contiguous():
            raise _lib.DlwpError("token MLP: resid must be contiguous and shaped like n")
    if ln_eps is None and b1 is None:
        raise _lib.DlwpError("token MLP: fc1 bias missing")
    if out is None:
        out = torch.empty_like(n)
    elif out.shape != n.shape or not out.is_contiguous():
        raise _lib.DlwpError("token MLP: out must be contiguous and shaped like n")
    common = (n, resid, packed, _contig(b1), _contig(b2), out, n.numel() // c, c, int(hidden),
              float(ln_eps) if ln_eps is not None else -1.0)
    if emit_norm is None:
        _lib.launch("dlwp_token_mlp_f32", n.device, *common)
        return out
    if n.dim() != 4:
        raise _lib.DlwpError("token MLP emit_norm: n must be [B, H, W, C]")
    gamma, beta, eps = emit_norm
    b, h, w, _ = n.shape
    nxt = torch.empty(b, c, h, w, device=n.device, dtype=torch.float32)
    _lib.launch("dlwp_token_mlp_emit_norm_f32", n.device, *common, gamma.contiguous(), beta.contiguous(), float(eps), nxt, h * w)
    return out, nxt


def afno_block_tail(f_cf: torch.Tensor, l_cf: torch.Tensor, x_nhwc: torch.Tensor, packed: torch.Tensor,
                    b2: Optional[torch.Tensor], hidden: int, ln_eps: float, emit_norm=None, out: Optional[torch.Tensor] = None,
                    form: str = "bf16x6"):
    """Everything of an AFNO block after the inverse FFT, one launch (fourcastnet.py:127, :187, :191-192):
    sum = f_cf + l_cf + x;  out = sum + fc2(gelu(fc1(LayerNorm(sum)))).  f_cf / l_cf [B, C, H, W], x / out [B, H, W, C];
    packed = TokenMlpWeights.get(..., norm2.weight, norm2.bias, fc1.bias, merged=True).
    emit_norm = (weight, bias, eps) of the next block's norm1 -> returns (out, LayerNorm(out) [B, C, H, W]).
    form "bf16x6" (three-part bf16 splits, six products) or "f16x3" (two-part f16 splits, three products; `packed` must
    come from TokenMlpWeights.get(..., f16x3=True)) -- both fp32-GEMM accurate, the operands here are LayerNorm / GELU outputs."""
    if form not in ("bf16x6", "f16x3"):
        raise _lib.DlwpError(f"afno_block_tail: unknown form {form!r}")
    for t, nm in ((f_cf, "f_cf"), (l_cf, "l_cf"), (x_nhwc, "x")):
        _lib.require_cuda_tensor(t, nm)
    f_cf, l_cf, x_nhwc = f_cf.contiguous(), l_cf.contiguous(), x_nhwc.contiguous()
    b, h, w, c = x_nhwc.shape
    if tuple(f_cf.shape) != (b, c, h, w) or tuple(l_cf.shape) != (b, c, h, w):
        raise _lib.DlwpError("afno_block_tail: f_cf / l_cf must be [B, C, H, W] matching x [B, H, W, C]")
    if out is None:
        out = torch.empty_like(x_nhwc)
    nxt = torch.empty(b, c, h, w, device=x_nhwc.device, dtype=torch.float32) if emit_norm is not None else None
    gamma, beta, eps = emit_norm if emit_norm is not None else (None, None, 0.0)
    _lib.launch("dlwp_afno_block_tail_f16x3" if form == "f16x3" else "dlwp_afno_block_tail_f32", x_nhwc.device, f_cf, l_cf,
                x_nhwc, packed, _contig(b2), out, b, h * w, c, int(hidden), float(ln_eps), _contig(gamma), _contig(beta),
                float(eps), nxt)
    return (out, nxt) if emit_norm is not None else out


def layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5,
               pre_bias: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """LayerNorm over the last dimension (any leading shape); pre_bias [C] is added to x before the statistics.
    out_dtype=torch.bfloat16: the result rounded to bfloat16 (dlwp_layernorm_prebias_bf16out) -- for a bf16-form Linear, which
    would round it the same way itself."""
    _lib.require_cuda_tensor(x, "x")
    from . import training as _T
    if _T.wants_grad(x, weight, bias, pre_bias):
        if pre_bias is None and weight is not None and bias is not None and layernorm_backward_supported(x.shape[-1]):
            return _T.layer_norm(x, weight, bias, eps)           # HIP forward and backward (training._LayerNormFn)
        # the deferred-bias form is inference only; widths outside the kernels' envelope: the torch operator
        return torch.nn.functional.layer_norm(x if pre_bias is None else x + pre_bias, (x.shape[-1],), weight, bias, eps)
    x = x.contiguous()
    c = x.shape[-1]
    rows = x.numel() // c
    ob16 = out_dtype == torch.bfloat16
    y = torch.empty_like(x, dtype=torch.bfloat16) if ob16 else torch.empty_like(x)
    _lib.launch("dlwp_layernorm_prebias_bf16out" if ob16 else "dlwp_layernorm_prebias_f32", x.device, x, _contig(pre_bias),
                weight.contiguous(), bias.contiguous(), y, rows, c, float(eps))
    return y


def layernorm_backward_supported(channels: int) -> bool:
    """True inside the envelope of dlwp_layernorm_bwd_f32 (the forward's: channels % 4 == 0 and <= 2048)."""
    return int(channels) > 0 and int(channels) % 4 == 0 and int(channels) <= 2048


def layernorm_backward(x: torch.Tensor, weight: torch.Tensor, grad_out: torch.Tensor, eps: float = 1e-5, need_x: bool = True,
                       need_weight: bool = True, need_bias: bool = True):
    """The gradients of layer_norm on dlwp_layernorm_bwd_f32 from x, gamma and grad_out alone (both contiguous, [..., C];
    mean and rstd are recomputed): (dx, dgamma, dbeta), None where not wanted.  Runs on the current stream without a host
    synchronisation; reruns are bitwise identical.  A width or an alignment outside the envelope raises a DlwpError whose
    status is ERR_UNSUPPORTED."""
    for t, name in ((x, "x"), (weight, "weight"), (grad_out, "grad_out")):
        _lib.require_cuda_tensor(t, name)
    c = x.shape[-1]
    rows = x.numel() // max(c, 1)
    if grad_out.shape != x.shape or not x.is_contiguous() or not grad_out.is_contiguous() or weight.numel() != c:
        raise _lib.DlwpError(f"layernorm_backward: x {tuple(x.shape)} and grad_out {tuple(grad_out.shape)} must be contiguous "
                             f"and of one shape, weight [{c}]")
    dx = torch.empty_like(x) if need_x else None
    dw = torch.empty(c, device=x.device, dtype=torch.float32) if need_weight else None
    db = torch.empty(c, device=x.device, dtype=torch.float32) if need_bias else None
    nbytes = max(int(_lib.load().dlwp_layernorm_bwd_workspace_bytes(rows, c)), 16) if (need_weight or need_bias) else 0
    ws = _lib.workspace(nbytes, x.device)
    _lib.launch("dlwp_layernorm_bwd_f32", x.device, x, weight.contiguous(), grad_out, dx, dw, db, ws, nbytes, rows, c, float(eps))
    return dx, dw, db


def activation(z: torch.Tensor, act: int) -> torch.Tensor:
    """act(z) elementwise on dlwp_act_f32 (codes of ACTS): for GELU the arithmetic of the dlwp_linear_f32 epilogue, so the
    result is bit for bit what linear(..., act=1) stores.  z contiguous with a multiple of 4 values."""
    _lib.require_cuda_tensor(z, "z")
    if not z.is_contiguous():
        raise _lib.DlwpError("activation: z must be contiguous")
    h = torch.empty_like(z)
    _lib.launch("dlwp_act_f32", z.device, z, h, z.numel(), int(act))
    return h


def bias_act_backward(grad_out: torch.Tensor, z: Optional[torch.Tensor], act: int = 0, need_bias: bool = True):
    """The pointwise part of a Linear's backward on dlwp_bias_act_bwd_f32: (gz, db) with gz = grad_out * act'(z) and
    db = gz summed over the rows ([N]; None unless need_bias).  grad_out and z contiguous [..., N]; act 0 needs no z and
    returns grad_out itself as gz.  Runs on the current stream without a host synchronisation; reruns are bitwise
    identical.  A width or an alignment outside the envelope raises a DlwpError whose status is ERR_UNSUPPORTED."""
    _lib.require_cuda_tensor(grad_out, "grad_out")
    _lib.require_cuda_tensor(z, "z")
    act = int(act)
    n = grad_out.shape[-1]
    rows = grad_out.numel() // max(n, 1)
    if not grad_out.is_contiguous() or (act != 0 and (z is None or z.shape != grad_out.shape or not z.is_contiguous())):
        raise _lib.DlwpError("bias_act_backward: grad_out and z must be contiguous and of one shape")
    gz = torch.empty_like(grad_out) if act != 0 else grad_out
    db = torch.empty(n, device=grad_out.device, dtype=torch.float32) if need_bias else None
    nbytes = max(int(_lib.load().dlwp_bias_act_bwd_workspace_bytes(rows, n)), 16) if need_bias else 0
    ws = _lib.workspace(nbytes, grad_out.device)
    z_in, gz_out = (z, gz) if act != 0 else (None, None)        # act 0: nothing to read or write but the bias sum
    _lib.launch("dlwp_bias_act_bwd_f32", grad_out.device, grad_out, z_in, gz_out, db, ws, nbytes, rows, n, act)
    return gz, db


@functools.lru_cache(maxsize=None)
def linear_supported(in_features: int, out_features: int) -> bool:
    """True when dlwp_linear_f32 handles this Linear shape (in % 32 == 0, out % 4 == 0)."""
    return int(_lib.load().dlwp_linear_packed_bytes(int(out_features), int(in_features))) > 0


class LinearWeights:
    """A Linear weight [out, in] split into the three bf16 images dlwp_linear_f32 reads, re-split on the device whenever
    the parameter has been written to (optimizer step, load_state_dict, .to()).  Derived data: not in any state dict."""

    def __init__(self):
        self._derived = (Derived(), Derived())      # the bf16x6 images, the f16x3 images

    def get(self, weight: torch.Tensor, f16: bool = False) -> torch.Tensor:
        packer = "dlwp_linear_pack_f16x3" if f16 else "dlwp_linear_pack_f32"

        def build():
            n, k = weight.shape
            lib = _lib.load()
            nbytes = int(lib.dlwp_linear_packed_bytes(n, k))
            if nbytes == 0:
                raise _lib.DlwpError(f"linear: unsupported shape out={n} in={k} (need in % 32 == 0 and out % 4 == 0)")
            buf = torch.empty(nbytes // 4, dtype=torch.int32, device=weight.device)
            _lib.launch(packer, weight.device, weight.detach().contiguous(), n, k, buf)
            return buf

        return self._derived[f16].get(source_key(weight), build)


def linear_raw(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
               resid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [..., K] @ weight[N, K]^T + bias + resid through dlwp_linear_f32 (fp32-accurate) for a weight that is a plain tensor --
    the three GEMMs of a Linear's training step (training._LinearFn); the weight is split on the device per call.  resid
    (contiguous, shaped like the output) is added in the GEMM's epilogue, as linear() does at inference."""
    _lib.require_cuda_tensor(x, "x")
    _lib.require_cuda_tensor(weight, "weight")
    _lib.require_cuda_tensor(bias, "bias")
    x, weight = x.contiguous(), weight.contiguous()
    n, k = weight.shape
    if x.shape[-1] != k:
        raise _lib.DlwpError(f"linear: input width {x.shape[-1]} does not match in_features {k}")
    lib = _lib.load()
    nbytes = int(lib.dlwp_linear_packed_bytes(n, k))
    if nbytes == 0:
        raise _lib.DlwpError(f"linear: unsupported shape out={n} in={k} (need in % 32 == 0 and out % 4 == 0)")
    out = torch.empty((*x.shape[:-1], n), device=x.device, dtype=torch.float32)
    if resid is not None:
        _lib.require_cuda_tensor(resid, "resid")
        if resid.shape != out.shape or not resid.is_contiguous():
            raise _lib.DlwpError("linear: resid must be contiguous and shaped like the output")
    packed = torch.empty(nbytes // 4, dtype=torch.int32, device=x.device)
    _lib.launch("dlwp_linear_pack_f32", x.device, weight, n, k, packed)
    _lib.launch("dlwp_linear_f32", x.device, x, packed, _contig(bias), resid, out, x.numel() // k, k, n, 0)
    return out


def linear(x: torch.Tensor, m: torch.nn.Linear, act: int = 0, resid: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None, precision: str = "fp32", out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """act(x @ m.weight.T + m.bias) + resid over the last dimension in one launch; act 0 none / 1 exact GELU.
    precision "bf16" only: x may BE a bfloat16 tensor, or out_dtype=torch.bfloat16 asks for a bfloat16 result (no residual) --
    dlwp_linear_bf16_io, the hand-over of an MLP's hidden activation at half the bytes, bit-identical to the fp32 hand-over.
    precision "fp32": dlwp_linear_f32, fp32-accurate GEMM on the bf16 matrix pipe (six products of exact three-way splits);
    "bf16": dlwp_linear_bf16, bf16 operands and fp32 accumulation (what autocast(bfloat16) makes of nn.Linear);
    "f16x3": dlwp_linear_f16x3, fp32-GEMM accuracy from exact two-part f16 splits (three products; |x| < 65504).
    `out` may be `resid` (in-place residual add).  With gradients wanted the differentiable form runs (training._LinearFn:
    the same kernels forward, HIP backward; `out`, `precision` and `out_dtype` are inference only), or the torch operators for
    a shape the GEMM kernel does not take."""
    if precision not in ("fp32", "bf16", "f16x3"):
        raise _lib.DlwpError(f"linear: unknown precision {precision!r}")
    from . import training as _T
    if _T.wants_grad(x, m.weight, m.bias, resid):
        rows = x.numel() // max(x.shape[-1], 1)
        if act not in (0, 1):
            raise _lib.DlwpError(f"linear: activation {act} not supported")
        resid_ok = resid is None or (resid.is_cuda and resid.dtype == torch.float32 and
                                     tuple(resid.shape) == (*x.shape[:-1], m.out_features))
        if x.is_cuda and x.dtype == torch.float32 and resid_ok and _T._LinearFn.supported(rows, m.in_features, m.out_features):
            # HIP GEMMs forward and backward, bias / GELU / residual and their gradients on HIP too (training._LinearFn)
            return _T.linear_fn(x, m.weight, m.bias, act=act, resid=resid)
        y = torch.nn.functional.linear(x, m.weight, m.bias)
        if act == 1:
            y = _T.activation(y, 1)         # HIP in both directions on a GPU (training._ActFn); the GEMMs stay torch's
        return y if resid is None else y + resid
    x_bf16 = x.dtype == torch.bfloat16
    o_bf16 = out_dtype == torch.bfloat16 or (out is not None and out.dtype == torch.bfloat16)
    if x_bf16 or o_bf16:
        if precision != "bf16" or (o_bf16 and resid is not None):
            raise _lib.DlwpError("linear: bfloat16 tensors are taken by precision='bf16', without a residual on a bfloat16 output")
        if not x.is_cuda:
            raise _lib.DlwpError("linear: x must be a CUDA tensor")
    else:
        _lib.require_cuda_tensor(x, "x")
    if act not in (0, 1):
        raise _lib.DlwpError(f"linear: activation {act} not supported")
    x = x.contiguous()
    k, n = m.in_features, m.out_features
    if x.shape[-1] != k:
        raise _lib.DlwpError(f"linear: input width {x.shape[-1]} does not match in_features {k}")
    cache = m.__dict__.get("_dlwp_packed")
    if cache is None:
        cache = LinearWeights()
        m.__dict__["_dlwp_packed"] = cache       # plain attribute: neither parameter nor buffer, not in the state dict
    packed = cache.get(m.weight, f16=precision == "f16x3")
    shape = (*x.shape[:-1], n)
    if resid is not None:
        _lib.require_cuda_tensor(resid, "resid")
        if tuple(resid.shape) != shape or not resid.is_contiguous():
            raise _lib.DlwpError("linear: resid must be contiguous and shaped like the output")
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.bfloat16 if o_bf16 else torch.float32)
    elif tuple(out.shape) != shape or not out.is_contiguous():
        raise _lib.DlwpError("linear: out must be contiguous and shaped like the output")
    if out.data_ptr() == x.data_ptr():
        raise _lib.DlwpError("linear: out must not alias x")
    if x_bf16 or o_bf16:
        _lib.launch("dlwp_linear_bf16_io", x.device, x, packed, _contig(m.bias), resid, out, x.numel() // k, k, n, int(act),
                    int(x_bf16), int(o_bf16))
        return out
    name = {"fp32": "dlwp_linear_f32", "bf16": "dlwp_linear_bf16", "f16x3": "dlwp_linear_f16x3"}[precision]
    _lib.launch(name, x.device, x, packed, _contig(m.bias), resid, out, x.numel() // k, k, n, int(act))
    return out


def linear_any(x: torch.Tensor, m: torch.nn.Linear, act: int = 0, resid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(m(x)) + resid for any Linear: through linear() (HIP kernel; with gradients wanted its differentiable form) on a
    GPU, the module itself elsewhere (CPU construction / registry tests) or when the kernel does not take the shape."""
    from . import training as _T
    if x.is_cuda and x.dtype == torch.float32 and (_T.wants_grad(x, m.weight, m.bias, resid) or
                                                   linear_supported(m.in_features, m.out_features)):
        return linear(x, m, act=act, resid=resid.contiguous() if resid is not None else None)
    y = m(x)
    y = torch.nn.functional.gelu(y) if act == 1 else y
    return y if resid is None else y + resid


LINEAR_FORMS = ("bf16x6", "f16x3", "bf16", "rocblas")
_FORM_PRECISION = {"bf16x6": "fp32", "f16x3": "f16x3", "bf16": "bf16"}


def form_precision(form: str) -> str:
    """the `precision` argument of linear() a model's linear_form stands for"""
    return _FORM_PRECISION[form]


def linear_as(form: str, x: torch.Tensor, m: torch.nn.Linear) -> torch.Tensor:
    """m(x) through dlwp_linear_f32 (form "bf16x6") / dlwp_linear_bf16 ("bf16") when the shape is covered, else the module
    itself (rocBLAS fp32)."""
    if form in _FORM_PRECISION and x.is_cuda and linear_supported(m.in_features, m.out_features):
        return linear(x, m, precision=_FORM_PRECISION[form])
    return m(x)


class ConvAsLinear:
    """A Conv2d / ConvTranspose2d whose kernel equals its stride (no overlap, no padding) as a Linear over the channels of
    TOKEN-MAJOR data: ConvTranspose2d(Cin, Cout, k, k) = Linear(Cin -> k k Cout) + a pixel shuffle, Conv2d(Cin, Cout, 1) =
    Linear(Cin -> Cout).  The derived weight / bias follow the module's parameters (data_ptr, version); out_features is
    padded to a multiple of 4 with zero rows (dlwp_linear_f32's store width).  Used by the Swin decoder
    (swin_transformer.py:600-612, :672-677), which the reference runs as MIOpen convolutions on channels-first copies."""

    def __init__(self, conv: torch.nn.Module):
        self.conv = conv
        self.transposed = isinstance(conv, torch.nn.ConvTranspose2d)
        k = conv.kernel_size
        if k[0] != k[1] or tuple(conv.stride) != tuple(k) or conv.padding not in (0, (0, 0)) or conv.groups != 1 or \
                conv.dilation not in (1, (1, 1)) or (not self.transposed and k[0] != 1) or \
                (self.transposed and conv.output_padding not in (0, (0, 0))):
            raise _lib.DlwpError(f"ConvAsLinear: {conv} is not a kernel = stride convolution")
        self.k = k[0]
        self.in_features = conv.in_channels
        self.cout = conv.out_channels
        n = self.k * self.k * self.cout if self.transposed else self.cout
        self.out_features = (n + 3) // 4 * 4
        self._n = n
        self._key = None
        self.weight = None
        self.bias = None

    def refresh(self):
        w, b = self.conv.weight, self.conv.bias
        key = source_key(w, b)
        if key == self._key:
            return
        with torch.no_grad():
            if self.transposed:      # [Cin, Cout, k, k] -> [(di k + dj) Cout + co][ci]
                wl = w.permute(2, 3, 1, 0).reshape(self._n, self.in_features)
                bl = None if b is None else b.repeat(self.k * self.k)
            else:                    # [Cout, Cin, 1, 1]
                wl = w.reshape(self._n, self.in_features)
                bl = b
            if self.out_features != self._n:
                wl = torch.cat([wl, wl.new_zeros(self.out_features - self._n, self.in_features)])
                bl = None if bl is None else torch.cat([bl, bl.new_zeros(self.out_features - self._n)])
            self.weight = wl.contiguous()
            self.bias = None if bl is None else bl.contiguous()
        self._key = key

    def __call__(self, x: torch.Tensor, h: int, w: int, act: int = 0, precision: str = "fp32") -> torch.Tensor:
        """x [B, h*w, Cin] token-major -> [B, (h k)*(w k), Cout] token-major."""
        self.refresh()
        b = x.shape[0]
        y = linear(x, self, act=act, precision=precision)
        if self.out_features != self._n:
            y = y[..., :self._n]
        if self.transposed and self.k > 1:
            k = self.k
            y = y.reshape(b, h, w, k, k, self.cout).permute(0, 1, 3, 2, 4, 5).reshape(b, h * k * w * k, self.cout)
        return y.contiguous()


def attention_block_linears_supported(dim: int, hidden: int) -> bool:
    return linear_supported(dim, 3 * dim) and linear_supported(dim, dim) and linear_supported(dim, hidden) \
        and linear_supported(hidden, dim)


def attention_block_tail(x: torch.Tensor, attn_out: torch.Tensor, proj: torch.nn.Linear, norm2: torch.nn.LayerNorm,
                         fc1: torch.nn.Linear, fc2: torch.nn.Linear, precision: str = "fp32") -> torch.Tensor:
    """`x = x + proj(attn_out); x = x + fc2(gelu(fc1(norm2(x))))` of a Swin / Pangu block (swin_transformer.py:254-262,
    panguweather.py:318-322), IN PLACE on x: three dlwp_linear_f32 launches (bias, GELU and both residual adds in the GEMM
    epilogues) and one LayerNorm."""
    linear(attn_out, proj, resid=x, out=x, precision=precision)
    # bf16 form: LayerNorm output and hidden activation cross HBM as bfloat16 (their consumers round to bf16 anyway: bit-identical)
    b16 = torch.bfloat16 if precision == "bf16" else None
    n2 = layer_norm(x, norm2.weight, norm2.bias, norm2.eps, out_dtype=b16)
    hid = linear(n2, fc1, act=1, precision=precision, out_dtype=b16)
    linear(hid, fc2, resid=x, out=x, precision=precision)
    return x


def residual_block_tail(x: torch.Tensor, pend: Optional[torch.Tensor], attn_out: torch.Tensor, proj: torch.nn.Linear,
                        norm2: torch.nn.LayerNorm, fc1: torch.nn.Linear, fc2: torch.nn.Linear):
    """`x = x + proj(attn_out); x = x + fc2(gelu(fc1(norm2(x))))` of a Swin / Pangu block (swin_transformer.py:254-262,
    panguweather.py:318-322) with both residual adds as the beta = 1 accumulation of the GEMMs, IN PLACE on x, and
    the Linear biases deferred: x holds (true x - pend); returns the new pend.  The caller adds pend once per layer."""
    c = x.shape[-1]
    x2 = x.view(-1, c)
    x2.addmm_(attn_out.reshape(-1, c), proj.weight.t())
    if proj.bias is not None:
        pend = proj.bias if pend is None else pend + proj.bias
    n2 = layer_norm(x, norm2.weight, norm2.bias, norm2.eps, pre_bias=pend)
    hid = torch.nn.functional.gelu(torch.nn.functional.linear(n2, fc1.weight, fc1.bias))
    x2.addmm_(hid.view(-1, hid.shape[-1]), fc2.weight.t())
    if fc2.bias is not None:
        pend = fc2.bias if pend is None else pend + fc2.bias
    return pend


class HipLayerNorm(torch.nn.LayerNorm):
    """nn.LayerNorm (same parameters / state-dict names) whose forward runs dlwp_layernorm_f32."""

    def forward(self, x):
        if len(self.normalized_shape) != 1 or self.weight is None or self.bias is None or x.shape[-1] % 4:
            raise _lib.DlwpError("HipLayerNorm needs a 1-D affine normalized_shape with channels % 4 == 0")
        return layer_norm(x, self.weight, self.bias, self.eps)


def global_attention(qkv: torch.Tensor, heads: int, d_k: int, scale: Optional[float] = None, return_stats: bool = False):
    """Global multi-head self-attention over all tokens of a sample (reference modern_unet.py:565-571, the core of the
    diffusion U-Net's AttentionBlock) on dlwp_global_attn_f32: qkv [Bt, N, heads * 3 * d_k] (or [Bt, N, heads, 3, d_k]),
    per head q | k | v contiguous, as the projection Linear writes it; returns [Bt, N, heads * d_k].  The softmax runs
    over the QUERY axis (the reference's dim=1); scale defaults to d_k ** -0.5.  Runs on the current stream with no host
    synchronisation; there is no other path -- a shape the kernel cannot take raises.  return_stats=True returns
    (out, stats): stats [Bt, heads, N] is the kernel's workspace, the per-key log-sum-exp in base 2 that
    global_attention_backward takes."""
    _lib.require_cuda_tensor(qkv, "qkv")
    heads, d_k = int(heads), int(d_k)
    if heads <= 0 or d_k <= 0:
        raise _lib.DlwpError(f"global_attention: heads {heads} and d_k {d_k} must be positive")
    if qkv.dim() == 5:
        if tuple(qkv.shape[2:]) != (heads, 3, d_k):
            raise _lib.DlwpError(f"global_attention: qkv {tuple(qkv.shape)} is not [Bt, N, {heads}, 3, {d_k}]")
        qkv = qkv.reshape(qkv.shape[0], qkv.shape[1], -1)
    if qkv.dim() != 3 or qkv.shape[-1] != heads * 3 * d_k:
        raise _lib.DlwpError(f"global_attention: qkv {tuple(qkv.shape)} is not [Bt, N, {heads * 3 * d_k}]")
    bt, n = int(qkv.shape[0]), int(qkv.shape[1])
    if bt <= 0 or n <= 0 or bt > 2 ** 31 - 1 or n > 2 ** 31 - 1:
        raise _lib.DlwpError(f"global_attention: batch {bt} and tokens {n} must be in [1, 2^31)")
    scale = d_k ** -0.5 if scale is None else float(scale)
    qkv = qkv.contiguous()
    # the workspace IS the statistics tensor a caller may ask for, so it is typed: [Bt, heads, N] fp32
    ws = torch.empty(int(_lib.load().dlwp_global_attn_workspace_bytes(bt, heads, n)) // 4, device=qkv.device, dtype=torch.float32)
    out = torch.empty((bt, n, heads * d_k), device=qkv.device, dtype=torch.float32)
    _lib.launch("dlwp_global_attn_f32", qkv.device, qkv, out, bt, n, heads, d_k, scale, ws, ws.numel() * 4)
    return (out, ws.view(bt, heads, n)) if return_stats else out


def global_attention_backward(qkv: torch.Tensor, stats: torch.Tensor, grad_out: torch.Tensor, heads: int, d_k: int,
                              scale: Optional[float] = None) -> torch.Tensor:
    """Gradient of global_attention with respect to qkv on dlwp_global_attn_bwd_f32: qkv as given to the forward, stats its
    return_stats workspace [Bt, heads, N], grad_out [Bt, N, heads * d_k]; returns dqkv in the shape of qkv (per head
    dq | dk | dv, the layout the projection Linear's backward takes).  Runs on the current stream with no host
    synchronisation; a shape the kernel does not take raises DlwpError (status -2 for DLWP_ERR_UNSUPPORTED)."""
    _lib.require_cuda_tensor(qkv, "qkv")
    _lib.require_cuda_tensor(stats, "stats")
    _lib.require_cuda_tensor(grad_out, "grad_out")
    heads, d_k = int(heads), int(d_k)
    if heads <= 0 or d_k <= 0:
        raise _lib.DlwpError(f"global_attention_backward: heads {heads} and d_k {d_k} must be positive")
    shape = qkv.shape
    if qkv.dim() == 5:
        if tuple(qkv.shape[2:]) != (heads, 3, d_k):
            raise _lib.DlwpError(f"global_attention_backward: qkv {tuple(qkv.shape)} is not [Bt, N, {heads}, 3, {d_k}]")
        qkv = qkv.reshape(qkv.shape[0], qkv.shape[1], -1)
    if qkv.dim() != 3 or qkv.shape[-1] != heads * 3 * d_k:
        raise _lib.DlwpError(f"global_attention_backward: qkv {tuple(qkv.shape)} is not [Bt, N, {heads * 3 * d_k}]")
    bt, n = int(qkv.shape[0]), int(qkv.shape[1])
    if bt <= 0 or n <= 0 or bt > 2 ** 31 - 1 or n > 2 ** 31 - 1:
        raise _lib.DlwpError(f"global_attention_backward: batch {bt} and tokens {n} must be in [1, 2^31)")
    if tuple(grad_out.shape) != (bt, n, heads * d_k):
        raise _lib.DlwpError(f"global_attention_backward: grad_out {tuple(grad_out.shape)} is not [{bt}, {n}, {heads * d_k}]")
    if stats.numel() != bt * heads * n:
        raise _lib.DlwpError(f"global_attention_backward: stats of {stats.numel()} values, {bt * heads * n} needed")
    if qkv.device != grad_out.device or qkv.device != stats.device:
        raise _lib.DlwpError("global_attention_backward: qkv, stats and grad_out must be on one device")
    scale = d_k ** -0.5 if scale is None else float(scale)
    qkv, grad_out, stats = qkv.contiguous(), grad_out.contiguous(), stats.contiguous()
    nbytes = int(_lib.load().dlwp_global_attn_bwd_workspace_bytes(bt, heads, n))
    ws = _lib.workspace(nbytes, qkv.device)
    dqkv = torch.empty_like(qkv)
    _lib.launch("dlwp_global_attn_bwd_f32", qkv.device, qkv, grad_out, stats, dqkv, bt, n, heads, d_k, scale, ws, nbytes)
    return dqkv.view(shape)


def attention_block(x: torch.Tensor, projection: torch.nn.Linear, output: torch.nn.Linear, heads: int, d_k: int,
                    scale: Optional[float] = None) -> torch.Tensor:
    """AttentionBlock.forward of the diffusion U-Net (reference modern_unet.py:551-585) on [B, C, H, W]: tokens
    [B, H W, C] (a copy), the projection Linear (linear_any), global_attention, the output Linear with the skip `+ x`
    in its epilogue (linear(resid=), in place on the token copy; the module itself where dlwp_linear_f32 does not take
    the shape), back to [B, C, H, W] (a copy)."""
    _lib.require_cuda_tensor(x, "x")
    if x.dim() != 4:
        raise _lib.DlwpError(f"attention_block: x must be [B, C, H, W] (got {tuple(x.shape)})")
    b, c, h, w = x.shape
    if projection.in_features != c or projection.out_features != heads * 3 * d_k or \
            output.in_features != heads * d_k or output.out_features != c:
        raise _lib.DlwpError(f"attention_block: Linears {projection} / {output} do not match C {c}, heads {heads}, d_k {d_k}")
    t = x.reshape(b, c, h * w).transpose(1, 2).contiguous()
    res = global_attention(linear_any(t, projection), heads, d_k, scale)
    if linear_supported(output.in_features, output.out_features):
        y = linear(res, output, resid=t, out=t)
    else:
        y = output(res).add_(t)
    return y.transpose(1, 2).reshape(b, c, h, w).contiguous()


# ---- MeshGraphNet (models/mgn.py; csrc/mgn.hip) --------------------------------------------------------------------------
MGN_MAX_WIDTH = 512         # hidden / output widths the HIP kernels take (include/dlwp_hip.h)
MGN_MAX_IN_WIDTH = 2048     # input width of dlwp_mgn_mlp_f32


def mgn_parts(seq: torch.nn.Sequential):
    """(Linears, LayerNorm or None) of a MeshGraphMLP's `model` (mesh_graph_mlp.py: Linear, act, ..., Linear[, norm])"""
    lins = [m for m in seq if isinstance(m, torch.nn.Linear)]
    ln = seq[-1] if isinstance(seq[-1], torch.nn.LayerNorm) else None
    return lins, ln


def mgn_mlp_supported(seq: torch.nn.Sequential, max_in: int = MGN_MAX_IN_WIDTH) -> bool:
    lins, _ = mgn_parts(seq)
    return 2 <= len(lins) <= 5 and lins[0].in_features <= max_in and all(l.out_features <= MGN_MAX_WIDTH for l in lins)


def mgn_layer_supported(edge_seq: torch.nn.Sequential, node_seq: torch.nn.Sequential, aggregation: str) -> bool:
    el, eln = mgn_parts(edge_seq)
    nl, nln = mgn_parts(node_seq)
    d = el[-1].out_features
    return (aggregation in ("sum", "mean") and eln is not None and nln is not None and d <= MGN_MAX_WIDTH
            and mgn_mlp_supported(edge_seq, 3 * d) and mgn_mlp_supported(node_seq, 2 * d)
            and all(l.out_features <= d for l in el + nl))


def _mlp_key(lins, ln):
    return source_key(*(t for l in lins for t in (l.weight, l.bias)), *((ln.weight, ln.bias) if ln is not None else ()))


class MgnMlpWeights:
    """Derived operand of one MeshGraphMLP: its Linear weights transposed to [in][out] and the descriptor pointing at them,
    re-derived when a parameter's (pointer, version) or the pack epoch changes."""

    def __init__(self):
        self._derived = Derived()

    def get(self, seq: torch.nn.Sequential) -> "_lib.MgnMlpDesc":
        lins, ln = mgn_parts(seq)

        def build():
            wts = [l.weight.detach().t().contiguous() for l in lins]
            d = _lib.MgnMlpDesc()
            d.n_linear = len(lins)
            d.dims[0] = lins[0].in_features
            for i, l in enumerate(lins):
                d.dims[i + 1] = l.out_features
                d.wt[i] = wts[i].data_ptr()
                d.bias[i] = l.bias.data_ptr()
            d.ln_gamma = ln.weight.data_ptr() if ln is not None else None
            d.ln_beta = ln.bias.data_ptr() if ln is not None else None
            d.ln_eps = float(ln.eps) if ln is not None else 0.0
            return d, wts               # (the descriptor points into the transposed weights)

        return self._derived.get(_mlp_key(lins, ln), build)[0]


def mgn_mlp(packed: MgnMlpWeights, seq: torch.nn.Sequential, x: torch.Tensor, batch: int, rows: int,
            channels_first_in: bool = False, channels_first_out: bool = False) -> torch.Tensor:
    """dlwp_mgn_mlp_f32 over batch * rows rows; x [batch * rows, C] or channels-first [batch, C, rows] (any trailing shape
    of `rows` elements); returns [batch * rows, C_out] or [batch, C_out, rows]"""
    _lib.require_cuda_tensor(x, "x")
    lins, _ = mgn_parts(seq)
    cin, cout = lins[0].in_features, lins[-1].out_features
    if x.numel() != batch * rows * cin or (channels_first_in and (x.shape[0] != batch or x.shape[1] != cin)) or \
            (not channels_first_in and x.shape[-1] != cin):
        raise _lib.DlwpError(f"mgn mlp: input of shape {tuple(x.shape)} for {batch} x {rows} rows of width {cin}")
    x = x.contiguous()                  # the kernel indexes a dense [B, C, rows] / [rows, C] block
    out = torch.empty((batch, cout, rows) if channels_first_out else (batch * rows, cout), device=x.device, dtype=torch.float32)
    _lib.launch("dlwp_mgn_mlp_f32", x.device, packed.get(seq), x, out, batch, rows, int(channels_first_in),
                int(channels_first_out))
    return out


def mgn_processor_layer(edge_packed: MgnMlpWeights, edge_seq, node_packed: MgnMlpWeights, node_seq, aggregation: str,
                        row_ptr: torch.Tensor, src: torch.Tensor, dst: torch.Tensor, batch: int, x_in: torch.Tensor, x_out: torch.Tensor,
                        e_in: torch.Tensor, e_shared: bool, e_out: torch.Tensor) -> None:
    """dlwp_mgn_processor_layer_f32: x_out <- node block(edge block(x_in, e_in)); e_out <- the edge block's output.
    e_shared: e_in is one [E, D] table for the whole batch (stride 0), else [batch, E, D]."""
    n_nodes, n_edges = row_ptr.numel() - 1, src.numel()
    d = edge_seq[-1].normalized_shape[0]
    _lib.launch("dlwp_mgn_processor_layer_f32", x_in.device, edge_packed.get(edge_seq), node_packed.get(node_seq),
                0 if aggregation == "sum" else 1, row_ptr, src, dst, n_nodes, n_edges, batch, x_in, x_out, e_in,
                0 if e_shared else n_edges * d, e_out)


MGN_BWD_MAX_WIDTH = 64      # hidden / output widths of the backward kernels (csrc/mgn_bwd.hip)
MGN_BWD_MAX_IN_WIDTH = 256  # input width of dlwp_mgn_mlp_bwd_f32


def mgn_mlp_backward_supported(seq: torch.nn.Sequential, max_in: int = MGN_BWD_MAX_IN_WIDTH) -> bool:
    lins, _ = mgn_parts(seq)
    return (2 <= len(lins) <= 5 and lins[0].in_features <= max_in
            and all(l.out_features <= MGN_BWD_MAX_WIDTH for l in lins))


def mgn_layer_backward_supported(edge_seq: torch.nn.Sequential, node_seq: torch.nn.Sequential, aggregation: str) -> bool:
    d = mgn_parts(edge_seq)[0][-1].out_features
    return (mgn_layer_supported(edge_seq, node_seq, aggregation) and d <= MGN_BWD_MAX_WIDTH
            and mgn_mlp_backward_supported(edge_seq, 3 * d) and mgn_mlp_backward_supported(node_seq, 2 * d))


def _mgn_param_grads(seq: torch.nn.Sequential, flat: torch.Tensor):
    """the kernels' flat parameter gradient (include/dlwp_hip.h: per Linear the weight [in][out] then the bias, then gamma,
    beta) as a list in the order of seq.parameters()"""
    lins, ln = mgn_parts(seq)
    out, o = [], 0
    for l in lins:
        k, n = l.in_features, l.out_features
        out.append(flat[o:o + k * n].view(k, n).t().contiguous())
        o += k * n
        out.append(flat[o:o + n])
        o += n
    if ln is not None:
        d = ln.normalized_shape[0]
        out += [flat[o:o + d], flat[o + d:o + 2 * d]]
        o += 2 * d
    assert o == flat.numel()
    return out


def _mgn_param_count(seq: torch.nn.Sequential) -> int:
    lins, ln = mgn_parts(seq)
    return sum(l.in_features * l.out_features + l.out_features for l in lins) + (2 * ln.normalized_shape[0] if ln else 0)


def mgn_mlp_backward(packed: MgnMlpWeights, seq: torch.nn.Sequential, x: torch.Tensor, grad_out: torch.Tensor, batch: int,
                     rows: int, channels_first_in: bool = False, channels_first_out: bool = False, need_input_grad: bool = True):
    """dlwp_mgn_mlp_bwd_f32: the backward of mgn_mlp (same layouts).  Returns (grad_x in x's layout or None, [gradients in
    the order of seq.parameters()])."""
    _lib.require_cuda_tensor(x, "x")
    _lib.require_cuda_tensor(grad_out, "grad_out")
    x, grad_out = x.contiguous(), grad_out.contiguous()
    d = packed.get(seq)
    ws_bytes = _lib.load().dlwp_mgn_mlp_bwd_workspace_bytes(ctypes.byref(d), batch, rows)
    if ws_bytes == 0:
        raise _lib.DlwpError("mgn mlp backward: shape outside the backward envelope (ops.mgn_mlp_backward_supported)")
    ws = _lib.workspace(ws_bytes, x.device)
    gx = torch.empty_like(x) if need_input_grad else None
    flat = torch.empty(_mgn_param_count(seq), device=x.device, dtype=torch.float32)
    _lib.launch("dlwp_mgn_mlp_bwd_f32", x.device, d, x, grad_out, gx, flat, batch, rows, int(channels_first_in),
                int(channels_first_out), ws, ws_bytes)
    return gx, _mgn_param_grads(seq, flat)


def mgn_source_csr(src: torch.Tensor, n_nodes: int):
    """(src_row_ptr [n_nodes + 1], src_perm [E]) int32: the CSC edges sorted by source (stable), for the source-side gather
    of dlwp_mgn_processor_layer_bwd_f32"""
    s = src.long().cpu()
    perm = torch.sort(s, stable=True).indices
    row_ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(s, minlength=n_nodes).cumsum(0)])
    return row_ptr.int().to(src.device), perm.int().to(src.device)


def mgn_processor_layer_backward(edge_packed: MgnMlpWeights, edge_seq, node_packed: MgnMlpWeights, node_seq,
                                 aggregation: str, row_ptr, src, dst, src_row_ptr, src_perm, batch: int, x_in: torch.Tensor,
                                 e_in: torch.Tensor, e_shared: bool, dx_out: torch.Tensor, de_out: Optional[torch.Tensor]):
    """dlwp_mgn_processor_layer_bwd_f32: the backward of mgn_processor_layer from its inputs.  Returns (dx_in [B N, D],
    de_in (e_in's shape), [edge MLP parameter gradients], [node MLP parameter gradients])."""
    n_nodes, n_edges = row_ptr.numel() - 1, src.numel()
    d = edge_seq[-1].normalized_shape[0]
    dx_out = dx_out.contiguous()
    de_out = _contig(de_out)
    ed, nd = edge_packed.get(edge_seq), node_packed.get(node_seq)
    ws_bytes = _lib.load().dlwp_mgn_processor_layer_bwd_workspace_bytes(ctypes.byref(ed), ctypes.byref(nd), n_nodes, n_edges,
                                                                        batch, int(e_shared))
    if ws_bytes == 0:
        raise _lib.DlwpError("mgn processor layer backward: shape outside the backward envelope "
                             "(ops.mgn_layer_backward_supported)")
    ws = _lib.workspace(ws_bytes, x_in.device)
    dx_in = torch.empty_like(x_in)
    de_in = torch.empty(e_in.shape, device=e_in.device, dtype=torch.float32)
    ge = torch.empty(_mgn_param_count(edge_seq), device=x_in.device, dtype=torch.float32)
    gn = torch.empty(_mgn_param_count(node_seq), device=x_in.device, dtype=torch.float32)
    _lib.launch("dlwp_mgn_processor_layer_bwd_f32", x_in.device, ed, nd, 0 if aggregation == "sum" else 1, row_ptr, src, dst,
                src_row_ptr, src_perm, n_nodes, n_edges, batch, x_in, e_in, 0 if e_shared else n_edges * d, dx_out, de_out, dx_in,
                de_in, ge, gn, ws, ws_bytes)
    return dx_in, de_in, _mgn_param_grads(edge_seq, ge), _mgn_param_grads(node_seq, gn)


def mgn_mlp_torch(seq: torch.nn.Sequential, x: torch.Tensor) -> torch.Tensor:
    """torch composition of a MeshGraphMLP (training with gradients, widths outside the HIP envelope)"""
    return seq(x)


def mgn_layer_torch(edge_seq, node_seq, aggregation: str, src: torch.Tensor, dst: torch.Tensor, deg: torch.Tensor,
                    batch: int, x: torch.Tensor, e: torch.Tensor):
    """torch composition of one processor layer on [batch * N, D] nodes and [batch * E, D] (or shared [E, D]) edges,
    one graph shared by the batch: returns (x', e')"""
    n, ne = deg.numel(), src.numel()
    off = (torch.arange(batch, device=x.device) * n).repeat_interleave(ne)
    s, t = src.long().repeat(batch) + off, dst.long().repeat(batch) + off
    if e.shape[0] != batch * ne:
        e = e.repeat(batch, 1)
    e_new = mgn_mlp_torch(edge_seq, torch.cat((e, x[s], x[t]), dim=1)) + e
    agg = torch.zeros_like(x).index_add_(0, t, e_new)
    if aggregation == "mean":
        agg = agg / deg.clamp(min=1).to(x.dtype).repeat(batch).unsqueeze(1)
    elif aggregation != "sum":
        raise _lib.DlwpError(f"aggregation {aggregation!r}: sum or mean")
    return mgn_mlp_torch(node_seq, torch.cat((agg, x), dim=1)) + x, e_new


# ---- GraphCastNet (models/graphcast.py; csrc/graphcast.hip) --------------------------------------------------------------
GC_MAX_WIDTH = 512          # hidden / output widths of dlwp_gc_linear_f32 (include/dlwp_hip.h)
GC_MAX_IN = 4096            # input width of one Linear
GC_ACT = {torch.nn.ReLU: 1, torch.nn.SiLU: 2}


def gc_mlp_supported(seq: torch.nn.Sequential) -> bool:
    """a MeshGraphMLP `model` inside the HIP envelope: 2..5 Linears, ReLU or SiLU between them, LayerNorm or no norm"""
    lins, ln = mgn_parts(seq)
    acts = [m for m in seq if not isinstance(m, (torch.nn.Linear, torch.nn.LayerNorm))]
    return (2 <= len(lins) <= 5 and lins[0].in_features <= GC_MAX_IN and all(l.out_features <= GC_MAX_WIDTH for l in lins)
            and all(type(a) in GC_ACT for a in acts) and len(seq) == 2 * len(lins) - 1 + (ln is not None))


class GcMlpWeights:
    """Derived operands of one MeshGraphMLP for dlwp_gc_linear_f32: Linear weights transposed to [in][out]; the first
    Linear's input rows optionally split into column blocks (the edge MLP's e / x_src / x_dst parts) or permuted (the grid
    embedder reads the rollout's channel order).  Re-derived when a parameter's (pointer, version) or the pack epoch
    changes."""

    def __init__(self, split=None, perm=None):
        self.split, self.perm = split, perm
        self._derived = Derived()
        self.wt = self.first = self.zero = None

    def get(self, seq: torch.nn.Sequential):
        lins, ln = mgn_parts(seq)

        def build():
            self.wt = [l.weight.detach().t().contiguous() for l in lins]
            w0 = self.wt[0]
            if self.perm is not None:
                w0 = w0[self.perm].contiguous()
                self.wt[0] = w0
            if self.split is not None:
                self.first = [p.contiguous() for p in torch.split(w0, list(self.split), dim=0)]
            self.zero = torch.zeros(lins[0].out_features, device=w0.device, dtype=torch.float32)
            self.bwd_first = None
            return self

        return self._derived.get(_mlp_key(lins, ln), build)

    def backward_first(self, seq: torch.nn.Sequential, split=None):
        """the first Linear's weight in torch's [out][in] layout (the data gradient's [k][n] operand), its input columns
        permuted like the forward (`perm`) and split into contiguous column blocks (`split`, else this object's split; the
        node MLP's agg / x halves): cached per weight version with the forward operands"""
        self.get(seq)
        if self.bwd_first is None:
            w = mgn_parts(seq)[0][0].weight.detach()
            if self.perm is not None:
                w = w[:, self.perm]
            split = split if split is not None else self.split
            self.bwd_first = [c.contiguous() for c in torch.split(w, list(split), dim=1)] if split else [w.contiguous()]
        return self.bwd_first


def _gc_args(**kw) -> "_lib.GcLinearArgs":
    a = _lib.GcLinearArgs()
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return a


def gc_linear(args: "_lib.GcLinearArgs", device) -> None:
    _lib.launch("dlwp_gc_linear_f32", device, args)


def gc_layernorm(x: torch.Tensor, batch: int, rows: int, ln: torch.nn.LayerNorm, res: Optional[torch.Tensor] = None,
                 res_bs: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    out = x if out is None else out
    d = ln.normalized_shape[0]
    _lib.launch("dlwp_gc_layernorm_f32", x.device, x, out, batch, rows, d, ln.weight, ln.bias, float(ln.eps), res, res_bs)
    return out


def gc_a_fields(mode: int, x: torch.Tensor, x_bs: int) -> dict:
    """the A fields of a first Linear reading x: mode 0 rows [rows, D] per sample (x_bs 0: one table for the batch),
    mode 1 channels-first [B, C, rows...]"""
    return dict(a_mode=mode, a=x, a_batch_stride=x_bs, lda=x.shape[-1] if mode == 0 else 0)


def gc_agg_a_fields(x: torch.Tensor, x_bs: int, e_new: torch.Tensor, graph: dict, aggregation: str) -> dict:
    """the A fields of a node MLP's first Linear reading [agg e', x] (mode 2): e' [batch * E, D] summed by destination
    in CSC order (/ in-degree for mean), x [rows, D] per sample (x_bs 0: one table for the batch)"""
    d = e_new.shape[-1]
    return dict(a_mode=2, a=x, a_batch_stride=x_bs, lda=x.shape[-1], agg_e=e_new, agg_batch_stride=graph["src"].numel() * d,
                agg_width=d, row_ptr=graph["row_ptr"], agg_mean=int(aggregation == "mean"))


def gc_mlp(pk: GcMlpWeights, seq: torch.nn.Sequential, batch: int, rows: int, first: dict, res: Optional[torch.Tensor] = None,
           res_bs: int = 0, out_cf: bool = False, save: bool = False):
    """One MeshGraphMLP over batch * rows rows on dlwp_gc_linear_f32 / dlwp_gc_layernorm_f32.  `first`: the A operand (and
    gathered products) of the first Linear as dlwp_gc_linear_args fields; its weight is `first["wt"]` if given, else the
    whole transposed first weight.  Then act -> Linears -> [LayerNorm] [+ res].  Returns [batch * rows, D_out], or
    channels-first [batch, D_out, rows] when out_cf (no norm).
    save (training): every Linear writes its pre-activation z_i (the next one applies act on its A load, so act(z_i)
    never exists) and the LayerNorm writes a fresh tensor, so its input survives.  Returns (output, [z_0 .. z_last])."""
    w = pk.get(seq)
    lins, ln = mgn_parts(seq)
    act = GC_ACT[type(seq[1])]
    dev = w.wt[0].device
    cur, zs = None, []
    for i, l in enumerate(lins):
        last = i + 1 == len(lins)
        n = l.out_features
        cf = last and out_cf
        out = torch.empty((batch, n, rows) if cf else (batch * rows, n), device=dev, dtype=torch.float32)
        kw = dict(wt=w.wt[i], bias=l.bias, k=l.in_features, n=n, batch=batch, rows=rows, act=0 if last or save else act,
                  out=out, out_layout=int(cf), ldo=n)
        if i == 0:
            kw.update(first)
            kw["k"] = kw["wt"].shape[0]     # the e-part of a split edge Linear
        else:
            kw.update(a_mode=0, a=cur, a_batch_stride=rows * l.in_features, lda=l.in_features)
            if save:
                kw["a_act"] = act
        if last and ln is None and res is not None:
            kw.update(res=res, res_batch_stride=res_bs)
        gc_linear(_gc_args(**kw), dev)
        cur = out
        if save:
            zs.append(out)
    if ln is not None:
        cur = gc_layernorm(cur, batch, rows, ln, res, res_bs, out=torch.empty_like(cur) if save else None)
    return (cur, zs) if save else cur


def gc_node_products(pk: GcMlpWeights, part: int, x: torch.Tensor, batch: int, rows: int, x_bs: int) -> torch.Tensor:
    """x @ W_part (no bias): one per-node term of an edge MLP's first Linear, [batch * rows, H] (batch 1 when x_bs is 0)"""
    w = pk.first[part]
    k, h = w.shape
    out = torch.empty(batch * rows, h, device=x.device, dtype=torch.float32)
    gc_linear(_gc_args(a_mode=0, a=x, a_batch_stride=x_bs, lda=k, wt=w, bias=pk.zero, k=k, n=h, batch=batch, rows=rows,
                       act=0, out=out, out_layout=0, ldo=h), x.device)
    return out


def gc_layer(edge_pk: GcMlpWeights, edge_seq: torch.nn.Sequential, node_pk: GcMlpWeights, node_seq: torch.nn.Sequential,
             aggregation: str, graph: dict, batch: int, e: torch.Tensor, xs: torch.Tensor, xd: torch.Tensor, bs,
             residual: bool, save: bool = False):
    """One message-passing layer: e' = LN(mlp([e, xs[src], xd[dst]])) (+ e) with the node products W_s xs, W_d xd
    computed once per node and gathered in the first Linear's epilogue, then x' = LN(mlp([agg e', xd])) + xd with the
    aggregate and the concat read in the A-operand load.  bs: the batch strides of e, xs, xd (0: one [rows, D] table the
    batch shares).  graph: as training.gc_layer takes it.  Returns (x', e'), and with save also the pre-activations of
    the edge and the node MLP (gc_mlp)."""
    e_bs, xs_bs, xd_bs = bs
    n_src, n_dst, ne = graph["n_src"], graph["n_dst"], graph["src"].numel()
    pk = edge_pk.get(edge_seq)
    d = edge_seq[0].out_features
    first = dict(a_mode=0, a=e, a_batch_stride=e_bs, lda=e.shape[-1], wt=pk.first[0],
                 src_products=gc_node_products(pk, 1, xs, batch if xs_bs else 1, n_src, xs_bs), src_index=graph["src"],
                 src_products_batch_stride=n_src * d if xs_bs else 0, ld_src_products=d,
                 dst_products=gc_node_products(pk, 2, xd, batch if xd_bs else 1, n_dst, xd_bs), dst_index=graph["dst"],
                 dst_products_batch_stride=n_dst * d if xd_bs else 0, ld_dst_products=d)
    edge = gc_mlp(pk, edge_seq, batch, ne, first, res=e if residual else None, res_bs=e_bs, save=save)
    del first                               # the node products
    e_new = edge[0] if save else edge
    node = gc_mlp(node_pk, node_seq, batch, n_dst, gc_agg_a_fields(xd, xd_bs, e_new, graph, aggregation), res=xd,
                  res_bs=xd_bs, save=save)
    return (node[0], e_new, edge[1], node[1]) if save else (node, e_new)


# ---- GraphCastNet backward (training.gc_mlp / training.gc_layer; csrc/graphcast_bwd.hip) ----------------------------------
def gc_weight_grad(a_fields: dict, k: int, n: int, batch: int, rows: int, dz: torch.Tensor, dz_cf: bool = False,
                   dw: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None, bias: bool = True):
    """dlwp_gc_weight_grad_f32: (dW [n, k] = A^T dZ in torch's layout, db = column sums of dZ or None).  a_fields: the A
    operand as dlwp_gc_linear_args fields (a_mode, a, a_batch_stride, lda, agg_*, row_ptr, a_act).  dw may be a column
    block of a wider weight gradient (a view with unit column stride)."""
    ws_bytes = _lib.load().dlwp_gc_weight_grad_workspace_bytes(k, n, batch, rows)
    if ws_bytes == 0:
        raise _lib.DlwpError(f"gc weight grad: {k} -> {n} is outside the envelope")
    dev = dz.device
    ws = _lib.workspace(ws_bytes, dev)
    if dw is None:
        dw = torch.empty(n, k, device=dev, dtype=torch.float32)
    if dw.stride(1) != 1 or dw.shape != (n, k):
        raise _lib.DlwpError(f"gc weight grad: dW view {tuple(dw.shape)} / {dw.stride()} for {n} x {k}")
    if db is None and bias:
        db = torch.empty(n, device=dev, dtype=torch.float32)
    args = _gc_args(k=k, n=n, batch=batch, rows=rows, **a_fields)
    _lib.launch("dlwp_gc_weight_grad_f32", dev, args, dz, int(dz_cf), 0 if dz_cf else dz.stride(0), dw, dw.stride(0), db, ws,
                ws_bytes)
    return dw, db


def gc_data_grad(dz: torch.Tensor, w: torch.Tensor, batch: int, rows: int, dz_cf: bool = False,
                 z: Optional[torch.Tensor] = None, act: int = 0, res: Optional[torch.Tensor] = None, res_bs: int = 0,
                 out_cf: bool = False) -> torch.Tensor:
    """dA = dZ w on dlwp_gc_linear_f32 (torch's [out][in] weight w as its [k][n] operand) [* act'(z)] [+ res]: [batch * rows,
    in] or channels-first [batch, in, rows]; dZ [batch * rows, out] or channels-first [batch, out, rows]"""
    k, n = w.shape
    zero = torch.zeros(n, device=dz.device, dtype=torch.float32)
    out = torch.empty((batch, n, rows) if out_cf else (batch * rows, n), device=dz.device, dtype=torch.float32)
    kw = dict(a_mode=1 if dz_cf else 0, a=dz, a_batch_stride=k * rows, lda=k, wt=w, bias=zero, k=k, n=n, batch=batch,
              rows=rows, act=0, out=out, out_layout=int(out_cf), ldo=n)
    if z is not None:
        kw.update(act_grad_z=z, act_grad=act, ld_act_grad_z=z.stride(0))
    if res is not None:
        kw.update(res=res, res_batch_stride=res_bs)
    gc_linear(_gc_args(**kw), dz.device)
    return out


def gc_layernorm_backward(z: torch.Tensor, ln: torch.nn.LayerNorm, batch: int, rows: int, gy: Optional[torch.Tensor],
                          g_agg: Optional[torch.Tensor] = None, g_agg_bs: int = 0, idx: Optional[torch.Tensor] = None,
                          deg: Optional[torch.Tensor] = None, want_total: bool = False):
    """dlwp_gc_layernorm_bwd_f32: (g_total or None, dz, dgamma, dbeta) with g = gy + g_agg[idx] (/ deg[idx])"""
    d = ln.normalized_shape[0]
    ws_bytes = _lib.load().dlwp_gc_layernorm_bwd_workspace_bytes(batch, rows, d)
    if ws_bytes == 0:
        raise _lib.DlwpError(f"gc layernorm backward: width {d} is outside the envelope")
    dev = z.device
    ws = _lib.workspace(ws_bytes, dev)
    gx = torch.empty(batch * rows, d, device=dev, dtype=torch.float32)
    gt = torch.empty(batch * rows, d, device=dev, dtype=torch.float32) if want_total else None
    dg = torch.empty(d, device=dev, dtype=torch.float32)
    dbeta = torch.empty(d, device=dev, dtype=torch.float32)
    _lib.launch("dlwp_gc_layernorm_bwd_f32", dev, z, ln.weight, float(ln.eps), gy, g_agg, g_agg_bs, idx, deg, batch, rows, d, gt, gx,
                dg, dbeta, ws, ws_bytes)
    return gt, gx, dg, dbeta


def gc_segment_sum(x: torch.Tensor, batch: int, row_ptr: Optional[torch.Tensor], perm: Optional[torch.Tensor],
                   n_segments: int, batch_sum: bool = False) -> torch.Tensor:
    """dlwp_gc_segment_sum_f32 over x [batch * rows, D]: [batch (1 when batch_sum) * n_segments, D]; row_ptr None: the
    segment of n is row n (a plain fixed-order batch sum)"""
    d = x.shape[-1]
    x = x.contiguous()
    out = torch.empty((1 if batch_sum else batch) * n_segments, d, device=x.device, dtype=torch.float32)
    _lib.launch("dlwp_gc_segment_sum_f32", x.device, x, x.numel() // batch, row_ptr, perm, n_segments, d, batch, int(batch_sum),
                out)
    return out


def _mse_weight(weight: Optional[torch.Tensor], x: torch.Tensor):
    """(the weight on x's device, contiguous, broadcast to the trailing dimensions of x it spans, or None; the element count of
    that span)"""
    if weight is None:
        return None, max(int(x.shape[-1]), 1) if x.dim() else 1
    if weight.dtype not in (torch.float32, torch.float64):
        raise _lib.DlwpError(f"mse_loss: the weight must be float32 or float64 (got {weight.dtype})")
    lead = x.dim() - weight.dim()
    try:
        weight = torch.broadcast_to(weight, x.shape[lead:]) if lead >= 0 else None
    except RuntimeError:
        weight = None
    if weight is None or weight.numel() == 0:
        raise _lib.DlwpError(f"mse_loss: the weight must broadcast to trailing dimensions of the input, {tuple(x.shape)}")
    return weight.to(x.device).contiguous(), weight.numel()


def mse_loss_forward(x: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None, need_grad: bool = False):
    """mean((target - x)^2 weight) on dlwp_mse_loss_f32 (reference scripts/losses.py:175-188): (loss, grad).  weight: None or
    a float32 / float64 tensor whose shape is the trailing dimensions of x; a float64 weight is used as float64 and the loss
    is then a float64 scalar, as the reference's promotion gives.  grad = d loss / d x = 2 (x - target) weight / N, written in
    the same pass when need_grad, else None (nothing is allocated for it).  One pass and a single-workgroup finish, no host
    synchronisation, bitwise identical reruns."""
    _lib.require_cuda_tensor(x, "input")
    _lib.require_cuda_tensor(target, "target")
    if x.shape != target.shape or x.numel() == 0:
        raise _lib.DlwpError(f"mse_loss: input {tuple(x.shape)} and target {tuple(target.shape)} must have one non-empty shape")
    x, target = x.contiguous(), target.contiguous()
    weight, inner = _mse_weight(weight, x)
    n = x.numel()
    grad = torch.empty_like(x) if need_grad else None
    partials = torch.empty(int(_lib.load().dlwp_mse_loss_partials(n)), dtype=torch.float64, device=x.device)
    out = torch.empty(2, dtype=torch.float64, device=x.device)
    w64 = weight is not None and weight.dtype == torch.float64
    _lib.launch("dlwp_mse_loss_f32", x.device, x, target, weight, int(w64), grad, partials, out, n // inner, inner)
    return (out[0] if w64 else out.view(torch.float32)[2]), grad


def mse_loss_scale_grad(grad: torch.Tensor, upstream: torch.Tensor) -> torch.Tensor:
    """grad *= upstream in place on dlwp_mse_loss_scale_grad_f32: upstream is a one-element float32 / float64 device tensor
    that is read on the device; when it is exactly 1 the kernel touches nothing."""
    _lib.require_cuda_tensor(grad, "grad")
    if not upstream.is_cuda or upstream.numel() != 1 or upstream.dtype not in (torch.float32, torch.float64):
        raise _lib.DlwpError("mse_loss: the upstream gradient must be a float32 / float64 device scalar")
    _lib.launch("dlwp_mse_loss_scale_grad_f32", grad.device, grad, upstream.contiguous(), int(upstream.dtype == torch.float64),
                grad.numel())
    return grad


def mse_loss(x: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The reference's CustomMSELoss with reduction 'mean' (scripts/losses.py:175-188), differentiable with respect to x:
    training._MseLossFn (HIP forward that writes the gradient in the same pass)."""
    from . import training as _T
    return _T.mse_loss(x, target, weight)


# ---- the PDE-Refiner noise scheduler on the device (csrc/refiner.hip; schedulers.RefinerScheduler drives these) ----------------
def _i64(v: int) -> int:
    """the low 64 bits of an integer as the signed value the C ABI carries"""
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >> 63 else v


def _noise_offset(offset) -> int:
    offset = int(offset)
    if offset < 0 or offset % 4 or offset >= 1 << 62:
        raise _lib.DlwpError(f"the noise offset must be a non-negative multiple of 4 below 2^62 (got {offset})")
    return offset


def refiner_grid_span() -> int:
    """elements one sweep of the capped grid covers: above it the kernels' strided loop runs"""
    return int(_lib.load().dlwp_refiner_grid_span())


def philox_normal(shape_or_out, seed: int, offset: int = 0, device=None) -> torch.Tensor:
    """Standard normals from the device stream (dlwp_philox_normal_f32; the reference: torch.randn(target_shape),
    modern_unet.py:184): element e of the result is normal(seed, offset + e), a pure function of its arguments -- 10 000
    normals in one call are bitwise the 4096 at offset 0 followed by the rest at offset 4096.  `shape_or_out`: a shape (the
    result is allocated on `device`) or a contiguous float32 device tensor that is filled in place (an unaligned view is
    fine).  A draw of n elements uses up the indices [offset, offset + ceil(n / 4) * 4)."""
    if isinstance(shape_or_out, torch.Tensor):
        out = shape_or_out
        _lib.require_cuda_tensor(out, "out")
        if not out.is_contiguous():
            raise _lib.DlwpError("philox_normal: the output must be contiguous")
    else:
        dev = torch.device(device) if device is not None else None
        if dev is None or dev.type != "cuda":
            raise _lib.DlwpError(f"philox_normal: a device of the HIP path is needed (got {device}); the HIP path has no CPU "
                                 "fallback")
        out = torch.empty(tuple(int(s) for s in shape_or_out), dtype=torch.float32, device=dev)
    if out.numel():
        _lib.launch("dlwp_philox_normal_f32", out.device, out, out.numel(), _i64(seed), _noise_offset(offset))
    return out


def _member_range(members, first_member, what: str):
    members, first_member = int(members), int(first_member)
    if members < 1 or first_member < 0 or first_member + members > 1 << 31:
        raise _lib.DlwpError(f"{what}: members = {members}, first_member = {first_member} must name members within [0, 2^31)")
    return members, first_member


def philox_normal_members(shape_or_out, seed: int, members: int, first_member: int = 0, offset: int = 0,
                          device=None) -> torch.Tensor:
    """philox_normal for ensembles (dlwp_philox_normal_members_f32): the result is member-major along dim 0, which `members`
    must divide, and element e of member m is normal(seed, first_member + m, offset + e) -- the stream of philox_normal with the
    member in the counter, member 0 being that stream itself.  A member's values depend on (seed, member, offset, its own
    element count) only: members 0..5 of one call are bitwise the members of (first 0, 2 members) and (first 2, 4 members).
    Every member uses up the indices [offset, offset + ceil(n_per_member / 4) * 4)."""
    members, first_member = _member_range(members, first_member, "philox_normal_members")
    if isinstance(shape_or_out, torch.Tensor):
        out = shape_or_out
        _lib.require_cuda_tensor(out, "out")
        if not out.is_contiguous():
            raise _lib.DlwpError("philox_normal_members: the output must be contiguous")
    else:
        dev = torch.device(device) if device is not None else None
        if dev is None or dev.type != "cuda":
            raise _lib.DlwpError(f"philox_normal_members: a device of the HIP path is needed (got {device}); the HIP path has no "
                                 "CPU fallback")
        out = torch.empty(tuple(int(s) for s in shape_or_out), dtype=torch.float32, device=dev)
    if out.dim() < 1 or out.shape[0] % members:
        raise _lib.DlwpError(f"philox_normal_members: dim 0 of {tuple(out.shape)} is not divisible by the {members} members")
    if out.numel():
        _lib.launch("dlwp_philox_normal_members_f32", out.device, out, out.numel() // members, members, first_member, _i64(seed),
                    _noise_offset(offset))
    return out


def ddpm_step(sample: torch.Tensor, model_output: torch.Tensor, coefficients, noise: Optional[torch.Tensor] = None,
              seed: int = 0, offset: int = 0, out: Optional[torch.Tensor] = None, members: int = 1,
              first_member: int = 0) -> torch.Tensor:
    """The DDPM ancestral step in one pass (dlwp_ddpm_step_f32; the reference: noise_scheduler.step, modern_unet.py:201):
      prev = c0 (sa sample - sb model_output) + c1 sample + sigma z
    `coefficients` = (sa, sb, c0, c1, sigma) as Python floats (RefinerScheduler.coefficients).  z is `noise` when given, else
    philox_normal(seed, offset) evaluated inside the kernel (bitwise the same values); with sigma == 0 no noise is drawn or
    read.  `out` may be `sample` (in place).  With `members` > 1 or `first_member` > 0 the tensors are member-major along dim 0
    (which `members` must divide) and z is philox_normal_members(seed, members, first_member, offset) instead
    (dlwp_ddpm_step_members_f32)."""
    members, first_member = _member_range(members, first_member, "ddpm_step")
    by_member = members > 1 or first_member > 0
    if by_member and (sample.dim() < 1 or sample.shape[0] % members):
        raise _lib.DlwpError(f"ddpm_step: dim 0 of the sample {tuple(sample.shape)} is not divisible by the {members} members")
    _lib.require_cuda_tensor(sample, "sample")
    _lib.require_cuda_tensor(model_output, "model_output")
    _lib.require_cuda_tensor(noise, "noise")
    _lib.require_cuda_tensor(out, "out")
    n = sample.numel()
    others = [("model_output", model_output)] + ([("noise", noise)] if noise is not None else []) + \
        ([("out", out)] if out is not None else [])
    for name, t in others:
        if t.numel() != n or t.device != sample.device:
            raise _lib.DlwpError(f"ddpm_step: {name} {tuple(t.shape)} must have the sample's {n} elements on its device")
    if n == 0:
        raise _lib.DlwpError("ddpm_step: empty sample")
    if out is not None and not out.is_contiguous():
        raise _lib.DlwpError("ddpm_step: the output must be contiguous")
    sa, sb, c0, c1, sigma = (float(c) for c in coefficients)
    if not all(math.isfinite(c) for c in (sa, sb, c0, c1, sigma)) or sigma < 0:
        raise _lib.DlwpError(f"ddpm_step: coefficients {(sa, sb, c0, c1, sigma)} must be finite with sigma >= 0")
    same = out is sample
    sample, model_output = sample.contiguous(), model_output.contiguous()
    if out is None:
        out = torch.empty_like(sample)
    elif same:
        out = sample
    coef = (ctypes.c_double * 4)(c0 * sa, c0 * sb, c1, sigma)
    noise = noise.contiguous() if noise is not None else None
    if by_member:
        _lib.launch("dlwp_ddpm_step_members_f32", sample.device, sample, model_output, noise, out, n // members, members,
                    first_member, coef, _i64(seed), _noise_offset(offset))
    else:
        _lib.launch("dlwp_ddpm_step_f32", sample.device, sample, model_output, noise, out, n, coef, _i64(seed),
                    _noise_offset(offset))
    return out


def refiner_pair(prognostic: torch.Tensor, target: torch.Tensor, context_size: int, sqrt_abar: float, sqrt_1m_abar: float,
                 noise: Optional[torch.Tensor] = None, seed: int = 0, offset: int = 0):
    """The training pair of PDE-Refiner in one pass (dlwp_refiner_pair_f32; the reference: scripts/train.py:228-255):
      res = target - prognostic[:, context_size - 1 : context_size]
      y_noised = sqrt_abar res + sqrt_1m_abar eps,   v_target = sqrt_abar eps - sqrt_1m_abar res
    prognostic [B, T, C, H, W] with target [B, 1, C, H, W], or the HEALPix [B, T, C, 12, h, w] with [B, 1, C, 12, h, w]; the
    outputs are [B, 1, C, H, W] resp. [(B 12), 1, C, h, w] (train.py:232-233).  The frame of `prognostic` is read in place
    through its batch stride.  eps is `noise` (the outputs' shape) when given, else philox_normal(seed, offset) of the
    outputs' shape evaluated inside the kernel.  Returns (y_noised, v_target)."""
    _lib.require_cuda_tensor(prognostic, "prognostic")
    _lib.require_cuda_tensor(target, "target")
    _lib.require_cuda_tensor(noise, "noise")
    if prognostic.dim() not in (5, 6) or target.dim() != prognostic.dim() or target.shape[1] != 1 \
            or target.shape[0] != prognostic.shape[0] or target.shape[2:] != prognostic.shape[2:] or target.numel() == 0:
        raise _lib.DlwpError(f"refiner_pair: prognostic {tuple(prognostic.shape)} and target {tuple(target.shape)} must be "
                             "[B, T, C, (F,) H, W] and [B, 1, C, (F,) H, W]")
    if not 1 <= int(context_size) <= prognostic.shape[1]:
        raise _lib.DlwpError(f"refiner_pair: context_size {context_size} outside the {prognostic.shape[1]} frames")
    if target.device != prognostic.device:
        raise _lib.DlwpError("refiner_pair: prognostic and target are on different devices")
    frame = prognostic[:, int(context_size) - 1]
    if not frame[0].is_contiguous():                 # the batch stride is free, the frame itself is not
        frame = frame.contiguous()
    if not target[0].is_contiguous():
        target = target.contiguous()
    b, c = int(target.shape[0]), int(target.shape[2])
    faces = int(target.shape[3]) if target.dim() == 6 else 1
    plane = int(target.shape[-2]) * int(target.shape[-1])
    t_bs = int(target.stride(0)) if b > 1 else c * faces * plane
    p_bs = int(frame.stride(0)) if b > 1 else c * faces * plane
    out_shape = (b * faces, 1, c) + tuple(target.shape[-2:])
    if noise is not None:
        if tuple(noise.shape) != out_shape or noise.device != target.device:
            raise _lib.DlwpError(f"refiner_pair: the noise must be {out_shape} on the inputs' device (got {tuple(noise.shape)})")
        noise = noise.contiguous()
    y_noised = torch.empty(out_shape, dtype=torch.float32, device=target.device)
    v_target = torch.empty_like(y_noised)
    _lib.launch("dlwp_refiner_pair_f32", target.device, target, frame, noise, y_noised, v_target, b, faces, c, plane, t_bs, p_bs,
                float(sqrt_abar), float(sqrt_1m_abar), _i64(seed), _noise_offset(offset))
    return y_noised, v_target


# ---- the device-resident dataset (csrc/dataset.hip; data.DeviceWeatherDataset drives these) ------------------------------------
def dataset_grid_blocks() -> int:
    """workgroups of a full grid of the dataset kernels: above it (in tiles of 1024 plane elements) the strided loop runs"""
    return int(_lib.load().dlwp_dataset_grid_blocks())


def _dataset_store(store: torch.Tensor, what: str):
    _lib.require_cuda_tensor(store, "store")
    if store.dim() != 3 or not store.is_contiguous() or store.numel() == 0:
        raise _lib.DlwpError(f"{what}: the store must be a contiguous, non-empty [T, V, plane] tensor (got {tuple(store.shape)})")
    return int(store.shape[0]), int(store.shape[1]), int(store.shape[2])


def _dataset_int32(t: torch.Tensor, shape, device, name: str, what: str):
    if not isinstance(t, torch.Tensor) or t.device != device or t.dtype != torch.int32 or not t.is_contiguous() \
            or tuple(t.shape) != tuple(shape):
        raise _lib.DlwpError(f"{what}: {name} must be a contiguous int32 tensor {tuple(shape)} on the store's device")
    return t


def _dataset_out(out, shape, device, name: str, what: str):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    _lib.require_cuda_tensor(out, name)
    if tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != device:
        raise _lib.DlwpError(f"{what}: {name} must be a contiguous float32 tensor {tuple(shape)} on the store's device "
                             f"(got {tuple(out.shape)})")
    return out


def dataset_gather(store: torch.Tensor, frames: torch.Tensor, prog_table: Optional[torch.Tensor],
                   pres_table: Optional[torch.Tensor], context: int, normalize: bool, noise: float = 0.0,
                   items: Optional[torch.Tensor] = None, seed: int = 0, offset: int = 0, prescribed: Optional[torch.Tensor] = None,
                   prognostic: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None,
                   want_prognostic: bool = True, want_target: bool = True):
    """One batch from the resident store in one launch (dlwp_dataset_gather_f32; the reference: WeatherBenchDataset.__getitem__ +
    default_collate, data/datasets/datasets.py:330-416).  store [T, V, plane] float32; frames int32 [B, S + 1] store time indices
    (-1: no such frame); the channel tables int32 [n, 4] = {source variable, mean bits, std bits, NaN-fill flag} (None: no such
    channels); items int32 [B] (the noise member of each sample; needed with noise != 0).  Returns (prescribed [B, S, P, plane] or
    None, prognostic [B, S, C, plane] or None, target [B, S - context, C, plane] or None); the three may be caller-supplied
    contiguous buffers.  Everything is read from device memory when the launch executes."""
    what = "dataset_gather"
    n_times, n_vars, plane = _dataset_store(store, what)
    dev = store.device
    if not isinstance(frames, torch.Tensor) or frames.dim() != 2 or frames.shape[1] < 2 or frames.shape[0] < 1:
        raise _lib.DlwpError(f"{what}: frames must be [B, S + 1] with S >= 1")
    b, s = int(frames.shape[0]), int(frames.shape[1]) - 1
    _dataset_int32(frames, (b, s + 1), dev, "frames", what)
    context = int(context)
    if not 0 <= context <= s:
        raise _lib.DlwpError(f"{what}: context {context} outside [0, {s}]")
    c = int(prog_table.shape[0]) if prog_table is not None else 0
    p = int(pres_table.shape[0]) if pres_table is not None else 0
    if c:
        _dataset_int32(prog_table, (c, 4), dev, "prog_table", what)
    if p:
        _dataset_int32(pres_table, (p, 4), dev, "pres_table", what)
    noise = float(noise)
    if noise != 0.0 and c and want_prognostic:
        if items is None:
            raise _lib.DlwpError(f"{what}: noise needs the dataset item of every sample")
        _dataset_int32(items, (b,), dev, "items", what)
    pres = _dataset_out(prescribed, (b, s, p, plane), dev, "prescribed", what) if p else None
    prog = _dataset_out(prognostic, (b, s, c, plane), dev, "prognostic", what) if c and want_prognostic else None
    tar = _dataset_out(target, (b, s - context, c, plane), dev, "target", what) if c and want_target and context < s else None
    if pres is None and prog is None and tar is None:
        return None, None, None
    _lib.launch("dlwp_dataset_gather_f32", dev, store, n_times, n_vars, plane, frames, items if noise != 0.0 else None, b, s,
                context, prog_table if c else None, c, pres_table if p else None, p, pres, prog, tar, int(bool(normalize)),
                noise, _i64(seed), _noise_offset(offset))
    return pres, prog, tar


def dataset_stats(store: torch.Tensor, frames: torch.Tensor) -> torch.Tensor:
    """float64 [V, 3] = {count of non-NaN values, their sum, the sum of squared deviations from sum / count} per variable over
    the listed frames (dlwp_dataset_stats_f64; the reference: compute_statistics, datasets.py:419-453).  Repeated calls give the
    same bits."""
    what = "dataset_stats"
    n_times, n_vars, plane = _dataset_store(store, what)
    if not isinstance(frames, torch.Tensor) or frames.dim() != 1 or frames.numel() == 0:
        raise _lib.DlwpError(f"{what}: frames must be a non-empty list of time indices")
    _dataset_int32(frames, (frames.numel(),), store.device, "frames", what)
    out = torch.empty((n_vars, 3), dtype=torch.float64, device=store.device)
    nbytes = int(_lib.load().dlwp_dataset_stats_workspace_bytes(n_vars))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=store.device)
    _lib.launch("dlwp_dataset_stats_f64", store.device, store, n_times, n_vars, plane, frames, frames.numel(), out, ws, nbytes)
    return out


def dataset_group_mean(store: torch.Tensor, frames: torch.Tensor, groups: torch.Tensor, n_groups: int) -> torch.Tensor:
    """[G, V, plane]: the mean of the non-NaN values of every group of frames (dlwp_dataset_group_mean_f32; the reference:
    groupby(time.dt.month).mean(), climatology.py:41), NaN where a group has none.  groups int32 per listed frame; a value
    outside [0, G) skips the frame."""
    what = "dataset_group_mean"
    n_times, n_vars, plane = _dataset_store(store, what)
    if not isinstance(frames, torch.Tensor) or frames.dim() != 1 or frames.numel() == 0 or int(n_groups) < 1:
        raise _lib.DlwpError(f"{what}: frames must be a non-empty list of time indices and n_groups >= 1")
    _dataset_int32(frames, (frames.numel(),), store.device, "frames", what)
    _dataset_int32(groups, (frames.numel(),), store.device, "groups", what)
    out = torch.empty((int(n_groups), n_vars, plane), dtype=torch.float32, device=store.device)
    _lib.launch("dlwp_dataset_group_mean_f32", store.device, store, n_times, n_vars, plane, frames, groups, frames.numel(),
                int(n_groups), out)
    return out


def coarsen_mean(x: torch.Tensor, k: int) -> torch.Tensor:
    """k x k block means over the last two dimensions, NaN skipped (dlwp_coarsen_mean_f32; the reference:
    ds.coarsen(lat=k, lon=k).mean(), datasets.py:303-305).  Both dimensions must be multiples of k."""
    _lib.require_cuda_tensor(x, "x")
    k = int(k)
    if x.dim() < 2 or x.numel() == 0 or k < 1 or x.shape[-2] % k or x.shape[-1] % k:
        raise _lib.DlwpError(f"coarsen_mean: the last two dimensions of {tuple(x.shape)} must be multiples of k = {k}")
    x = x.contiguous()
    h, w = int(x.shape[-2]), int(x.shape[-1])
    out = torch.empty(tuple(x.shape[:-2]) + (h // k, w // k), dtype=torch.float32, device=x.device)
    _lib.launch("dlwp_coarsen_mean_f32", x.device, x, out, x.numel() // (h * w), h, w, k)
    return out


# ---- spherical harmonic transforms and the Driscoll-Healy channel mix (csrc/sht.hip; host tables: sphere.py) -----------------
def _complex_pairs(c: torch.Tensor, name: str) -> torch.Tensor:
    """the contiguous float32 [..., 2] buffer behind a complex64 tensor (what the kernels take)"""
    if not isinstance(c, torch.Tensor) or c.dtype != torch.complex64:
        raise _lib.DlwpError(f"{name} must be a complex64 tensor (got {getattr(c, 'dtype', type(c))})")
    pairs = torch.view_as_real(c.contiguous())
    _lib.require_cuda_tensor(pairs, name)
    return pairs


def sht(x: torch.Tensor, grid: str = "legendre-gauss", lmax: Optional[int] = None, mmax: Optional[int] = None) -> torch.Tensor:
    """Real spherical harmonic transform of fields [..., nlat, nlon] on `grid` ("legendre-gauss" or "equiangular", row 0 the
    northernmost latitude) -> complex64 [..., lmax, mmax], orthonormal with the Condon-Shortley phase (the conventions of
    sphere.py; dlwp_sht_f32).  lmax defaults to nlat, mmax to min(lmax, nlon / 2 + 1).  Entries with l < m are zero.  With a
    gradient wanted the same kernel runs inside training.sht, whose backward is `sht_backward`."""
    from . import sphere as _sph

    _lib.require_cuda_tensor(x, "x")
    if x.dim() < 2:
        raise _lib.DlwpError(f"sht: expected fields [..., nlat, nlon], got shape {tuple(x.shape)}")
    nlat, nlon = int(x.shape[-2]), int(x.shape[-1])
    lmax = nlat if lmax is None else int(lmax)
    mmax = min(lmax, nlon // 2 + 1) if mmax is None else int(mmax)
    tab = _sph.device_tables(grid, nlat, nlon, lmax, mmax, x.device)
    from . import training as _T
    if _T.wants_grad(x):
        return _T.sht(x, tab)
    lead = tuple(x.shape[:-2])
    planes = math.prod(lead)
    out = torch.empty(lead + (lmax, mmax, 2), device=x.device, dtype=torch.float32)
    if planes:
        _lib.launch("dlwp_sht_f32", x.device, x.contiguous(), tab.wleg, tab.tw, out, planes, nlat, nlon, lmax, mmax)
    return torch.view_as_complex(out)


def isht(c: torch.Tensor, grid: str, nlat: int, nlon: int) -> torch.Tensor:
    """The inverse of `sht`: complex64 coefficients [..., lmax, mmax] -> fields [..., nlat, nlon] on `grid` (dlwp_isht_f32).
    Entries with l < m are not read; the imaginary parts of m = 0 and m = nlon / 2 are ignored, as irfft ignores them."""
    from . import sphere as _sph

    pairs = _complex_pairs(c, "c")
    if c.dim() < 2:
        raise _lib.DlwpError(f"isht: expected coefficients [..., lmax, mmax], got shape {tuple(c.shape)}")
    lmax, mmax = int(c.shape[-2]), int(c.shape[-1])
    nlat, nlon = int(nlat), int(nlon)
    tab = _sph.device_tables(grid, nlat, nlon, lmax, mmax, c.device)
    from . import training as _T
    if _T.wants_grad(c):
        return _T.isht(c, tab)
    lead = tuple(c.shape[:-2])
    planes = math.prod(lead)
    out = torch.empty(lead + (nlat, nlon), device=c.device, dtype=torch.float32)
    if planes:
        _lib.launch("dlwp_isht_f32", c.device, pairs, tab.leg, tab.tw, out, planes, nlat, nlon, lmax, mmax)
    return out


class SphMixWeights:
    """A Driscoll-Healy weight ([cin, cout, lmax, 2] pairs) re-laid degree-major, [lmax, cin, cout, 2], the layout
    dlwp_sph_mix_packed_f32 reads in long runs; re-packed on the device whenever the source has been written to -- the derivation
    rule of ConvWeights, with the same rule for graph captures."""

    def __init__(self):
        self._derived = Derived(eager_only="sph_mix")

    @staticmethod
    def pack(pairs: torch.Tensor) -> torch.Tensor:
        ci, co, lmax = (int(s) for s in pairs.shape[:3])
        buf = torch.empty(lmax, ci, co, 2, dtype=torch.float32, device=pairs.device)
        _lib.launch("dlwp_sph_mix_pack_f32", pairs.device, pairs, buf, ci, co, lmax)
        return buf

    def get(self, owner: torch.Tensor, pairs: torch.Tensor) -> torch.Tensor:
        return self._derived.get(source_key(owner), lambda: self.pack(pairs))


def sph_mix(c: torch.Tensor, weight: torch.Tensor, owner: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Driscoll-Healy spectral convolution: out[b, o, l, m] = sum_i c[b, i, l, m] * weight[i, o, l] for m <= l, zero above the
    diagonal whatever c holds there.  c complex64 [B, Ci, lmax, mmax], weight complex64 [Ci, Co, lmax].  `owner`: the tensor the
    caller keeps alive that `weight` is (a view of) -- a module's Parameter; with it the degree-major pack of the weight is cached
    on that tensor (SphMixWeights) and dlwp_sph_mix_packed_f32 runs, the fast form; without it dlwp_sph_mix_f32 reads the weight as
    it lies.  Both give the same bits.  With a gradient wanted: training.sph_mix."""
    cp, wp = _complex_pairs(c, "c"), _complex_pairs(weight, "weight")
    if c.dim() != 4 or weight.dim() != 3 or weight.shape[0] != c.shape[1] or weight.shape[2] != c.shape[2]:
        raise _lib.DlwpError(f"sph_mix: c {tuple(c.shape)} [B, Ci, lmax, mmax] and weight {tuple(weight.shape)} [Ci, Co, lmax] "
                             "do not match")
    from . import training as _T
    if _T.wants_grad(c, weight):
        return _T.sph_mix(c, weight)
    b, ci, lmax, mmax = (int(s) for s in c.shape)
    co = int(weight.shape[1])
    out = torch.empty(b, co, lmax, mmax, 2, device=c.device, dtype=torch.float32)
    if b and owner is not None:
        packed = derived_for(owner, "sph_mix", SphMixWeights).get(owner, wp)
        _lib.launch("dlwp_sph_mix_packed_f32", c.device, cp, packed, out, b, ci, co, lmax, mmax)
    elif b:
        _lib.launch("dlwp_sph_mix_f32", c.device, cp, wp, out, b, ci, co, lmax, mmax)
    return torch.view_as_complex(out)


def sht_backward(g: torch.Tensor, grid: str, nlat: int, nlon: int) -> torch.Tensor:
    """The adjoint of `sht`: the cotangent g complex64 [..., lmax, mmax] of a spectrum -> the gradient [..., nlat, nlon] of the
    field it was transformed from (dlwp_sht_bwd_f32: the inverse transform's kernel over the forward's table wleg, every column
    weighted 2 pi / nlon).  Entries of g with l < m are not read."""
    from . import sphere as _sph

    pairs = _complex_pairs(g, "g")
    if g.dim() < 2:
        raise _lib.DlwpError(f"sht_backward: expected a cotangent [..., lmax, mmax], got shape {tuple(g.shape)}")
    lmax, mmax = int(g.shape[-2]), int(g.shape[-1])
    nlat, nlon = int(nlat), int(nlon)
    tab = _sph.device_tables(grid, nlat, nlon, lmax, mmax, g.device)
    lead = tuple(g.shape[:-2])
    planes = math.prod(lead)
    out = torch.empty(lead + (nlat, nlon), device=g.device, dtype=torch.float32)
    if planes:
        _lib.launch("dlwp_sht_bwd_f32", g.device, pairs, tab.wleg, tab.tw, out, planes, nlat, nlon, lmax, mmax)
    return out


def isht_backward(gy: torch.Tensor, grid: str, lmax: int, mmax: int) -> torch.Tensor:
    """The adjoint of `isht`: the cotangent gy [..., nlat, nlon] of a field -> the gradient complex64 [..., lmax, mmax] of the
    coefficients it was synthesised from, in torch's convention dL/dRe + i dL/dIm (dlwp_isht_bwd_f32: the forward transform's
    kernel over the inverse's table leg, the columns weighted as irfft weights them).  Exactly zero for l < m."""
    from . import sphere as _sph

    _lib.require_cuda_tensor(gy, "gy")
    if gy.dim() < 2:
        raise _lib.DlwpError(f"isht_backward: expected a cotangent [..., nlat, nlon], got shape {tuple(gy.shape)}")
    nlat, nlon = int(gy.shape[-2]), int(gy.shape[-1])
    lmax, mmax = int(lmax), int(mmax)
    tab = _sph.device_tables(grid, nlat, nlon, lmax, mmax, gy.device)
    lead = tuple(gy.shape[:-2])
    planes = math.prod(lead)
    out = torch.empty(lead + (lmax, mmax, 2), device=gy.device, dtype=torch.float32)
    if planes:
        _lib.launch("dlwp_isht_bwd_f32", gy.device, gy.contiguous(), tab.leg, tab.tw, out, planes, nlat, nlon, lmax, mmax)
    return torch.view_as_complex(out)


def sph_power_workspace_bytes(shape, lmax: int, mmax: int) -> int:
    """bytes of the partials dlwp_sph_power_sums_f32 needs for a rollout of `shape` [B, K, C, nlat, nlon] (at least 8)"""
    b, k, c, nlat, nlon = (int(s) for s in shape)
    return max(int(_lib.load().dlwp_sph_power_workspace_bytes(b, k, c, nlat, nlon, int(lmax), int(mmax))), 8)


def sph_power_sums(out: torch.Tensor, target: torch.Tensor, grid: str = "legendre-gauss", lmax: Optional[int] = None,
                   mmax: Optional[int] = None, into: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Spherical power spectrum sums of a rollout and its targets, both [B, K, C, nlat, nlon] float32 on `grid` (row 0 the
    northernmost latitude) -> double [4, K, C, lmax], summed over b:  0 power(out), 1 power(target), 2 power(out - target) with the
    difference formed in the field domain, 3 cross(out, target), where with c = sht(x) (the conventions of `sht`)
      power(x)[l] = sum_{m <= min(l, mmax - 1)} f_m |c[l, m]|^2,   cross(x, y)[l] = sum_m f_m Re(c_x[l, m] conj(c_y[l, m])),
    f_m = 1 for m = 0 and 2 m = nlon (imaginary part dropped), else 2.  One fused transform-and-reduce kernel and one combining
    launch (dlwp_sph_power_sums_f32): no coefficient is written to memory.  lmax defaults to nlat, mmax to min(lmax, nlon / 2 + 1).
    `into`: a [4, K, C, lmax] double tensor of running sums the new ones are ADDED to (dlwp_sph_power_sums_acc_f32: a batch cut
    anywhere gives the bits of the one-shot call); it is returned.  `workspace`: a uint8 tensor of at least
    sph_power_workspace_bytes(...) to use instead of one from torch's allocator (metrics.SphericalSpectrumMetrics keeps one).
    A north-south flip of BOTH inputs on a symmetric grid changes none of the four sums (only the signs of the coefficients
    with odd l - m change), so south-first data such as WeatherBench's may be passed as it is stored."""
    from . import sphere as _sph

    _lib.require_cuda_tensor(out, "out")
    _lib.require_cuda_tensor(target, "target")
    if out.dim() != 5:
        raise _lib.DlwpError(f"sph_power_sums: expected a lat-lon rollout [B, K, C, nlat, nlon], got {out.dim()}-D shape "
                             f"{tuple(out.shape)}")
    if target.shape != out.shape:
        raise _lib.DlwpError(f"target shape {tuple(target.shape)} != output shape {tuple(out.shape)}")
    if target.device != out.device:
        raise _lib.DlwpError(f"target is on {target.device}, output on {out.device}: both must be on one device")
    b, k, c, nlat, nlon = (int(s) for s in out.shape)
    if b < 1 or k < 1 or c < 1:
        raise _lib.DlwpError(f"sph_power_sums: empty rollout {tuple(out.shape)}")
    lmax = nlat if lmax is None else int(lmax)
    mmax = min(lmax, nlon // 2 + 1) if mmax is None else int(mmax)
    dev = out.device
    tab = _sph.device_tables(grid, nlat, nlon, lmax, mmax, dev)
    if into is not None:
        _lib.require_running_sums(into, (4, k, c, lmax), dev)
    need = sph_power_workspace_bytes(out.shape, lmax, mmax)
    if workspace is None:
        workspace = _lib.workspace(need, dev)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or workspace.numel() < need:
        raise _lib.DlwpError(f"workspace must be a uint8 tensor of at least {need} bytes on {dev}")
    sums = into if into is not None else torch.empty(4, k, c, lmax, dtype=torch.float64, device=dev)
    _lib.launch("dlwp_sph_power_sums_acc_f32" if into is not None else "dlwp_sph_power_sums_f32", dev, out.contiguous(),
                target.contiguous(), tab.wleg, tab.tw, sums, b, k, c, nlat, nlon, lmax, mmax, workspace, workspace.numel())
    return sums


# The two candidates of each half of the mix backward (tools/bench_sht.py times both; DESIGN.md section 35.7 has the figures and
# says why these stand):  dgrad "in_place" reads the parameter conjugate-transposed inside the mix kernel, "packed" first makes
# the degree-major image of the conjugate transpose -- per call, from the values the weight holds NOW (it changes every step:
# the rule of _conv2_forward_hip; no Derived cache);  wgrad "direct" stores into the parameter layout, "packed" stores
# degree-major into a scratch buffer and transposes it back.  Each pair gives the same bits.  Measured at the config's width
# (32 x 64, E 256, B 16): dgrad 0.089 ms packed against 0.104 in place; wgrad 0.108 ms direct against 0.111 through the scratch.
SPH_MIX_DGRAD = "packed"
SPH_MIX_WGRAD = "direct"


def sph_mix_backward(c_in: torch.Tensor, weight: torch.Tensor, g: torch.Tensor, need_c: bool = True, need_w: bool = True,
                     dgrad: Optional[str] = None, wgrad: Optional[str] = None):
    """The backward of `sph_mix` for the cotangent g complex64 [B, Co, lmax, mmax] of its output: (gc_in | None, gw | None).
    gc_in[b, i, l, m] = sum_o g[b, o, l, m] conj(weight[i, o, l]) for m <= l, zero above the diagonal (complex64 [B, Ci, lmax, mmax]);
    gw[i, o, l] = sum_b sum_{m <= l} conj(c_in[b, i, l, m]) g[b, o, l, m] (complex64 [Ci, Co, lmax]).  Entries above the diagonal
    of c_in and g are not read.  `dgrad` / `wgrad` choose between the candidates above (default SPH_MIX_DGRAD / SPH_MIX_WGRAD)."""
    cp, wp, gp = _complex_pairs(c_in, "c_in"), _complex_pairs(weight, "weight"), _complex_pairs(g, "g")
    if (c_in.dim() != 4 or weight.dim() != 3 or g.dim() != 4 or weight.shape[0] != c_in.shape[1] or weight.shape[2] != c_in.shape[2]
            or tuple(g.shape) != (c_in.shape[0], weight.shape[1], c_in.shape[2], c_in.shape[3])):
        raise _lib.DlwpError(f"sph_mix_backward: c_in {tuple(c_in.shape)} [B, Ci, lmax, mmax], weight {tuple(weight.shape)} "
                             f"[Ci, Co, lmax] and g {tuple(g.shape)} [B, Co, lmax, mmax] do not match")
    dgrad, wgrad = dgrad or SPH_MIX_DGRAD, wgrad or SPH_MIX_WGRAD
    if dgrad not in ("packed", "in_place") or wgrad not in ("packed", "direct"):
        raise _lib.DlwpError(f"sph_mix_backward: dgrad {dgrad!r} ('packed' or 'in_place'), wgrad {wgrad!r} ('packed' or 'direct')")
    b, ci, lmax, mmax = (int(s) for s in c_in.shape)
    co = int(weight.shape[1])
    dev = c_in.device
    gc = gw = None
    if need_c:
        gc = torch.empty(b, ci, lmax, mmax, 2, device=dev, dtype=torch.float32)
        if b and dgrad == "packed":
            packed = torch.empty(lmax, co, ci, 2, device=dev, dtype=torch.float32)
            _lib.launch("dlwp_sph_mix_pack_adjoint_f32", dev, wp, packed, ci, co, lmax)
            _lib.launch("dlwp_sph_mix_packed_f32", dev, gp, packed, gc, b, co, ci, lmax, mmax)
        elif b:
            _lib.launch("dlwp_sph_mix_dgrad_f32", dev, gp, wp, gc, b, ci, co, lmax, mmax)
        gc = torch.view_as_complex(gc)
    if need_w:
        gw = torch.empty(ci, co, lmax, 2, device=dev, dtype=torch.float32)
        if not b:
            gw.zero_()
        elif wgrad == "packed":
            scratch = torch.empty(lmax, ci, co, 2, device=dev, dtype=torch.float32)
            _lib.launch("dlwp_sph_mix_wgrad_packed_f32", dev, cp, gp, scratch, b, ci, co, lmax, mmax)
            _lib.launch("dlwp_sph_mix_unpack_f32", dev, scratch, gw, ci, co, lmax)
        else:
            _lib.launch("dlwp_sph_mix_wgrad_f32", dev, cp, gp, gw, b, ci, co, lmax, mmax)
        gw = torch.view_as_complex(gw)
    return gc, gw


# ---- 2-D Navier-Stokes trajectories on the unit torus (csrc/navier_stokes.hip) --------------------------
NS2D_SIZES = (32, 64)         # the grids the resident kernel runs (the work planes of 128 x 128 exceed the LDS)
NS2D_MAX_STEPS = 100000       # frames * substeps of one launch (kMaxSteps of csrc/navier_stokes.hip, which refuses more)
_NS2D_TABLES = {}             # (kind, n, ..., device) -> a device table made on the host in float64


def _ns2d_table(key, make):
    if key not in _NS2D_TABLES:
        _NS2D_TABLES[key] = make()
    return _NS2D_TABLES[key]


def ns2d_li2020_forcing(n: int, device) -> torch.Tensor:
    """0.1 (sin 2 pi (a + b) + cos 2 pi (a + b)) on the n x n grid of the unit torus (the forcing of Li et al. 2020), made in
    float64 on the host, kept per (n, device)"""
    def make():
        t = torch.arange(n, dtype=torch.float64) / n
        s = 2.0 * math.pi * (t[:, None] + t[None, :])
        return (0.1 * (torch.sin(s) + torch.cos(s))).to(torch.float32).to(device).contiguous()
    return _ns2d_table(("li2020", int(n), str(device)), make)


def grf_amplitude(n: int, tau: float, alpha: float, device) -> torch.Tensor:
    """float32 [n, n / 2 + 1] on `device`: A(k) = n sqrt(2) tau^(alpha - 1) (4 pi^2 |k|^2 + tau^2)^(-alpha / 2) with A(0) = 0 and
    zeros at |ka| = n / 2 and kb = n / 2 (modes the solver removes), made in float64 on the host, kept per (n, tau, alpha, device)"""
    n, tau, alpha = int(n), float(tau), float(alpha)

    def make():
        ka = torch.fft.fftfreq(n, d=1.0 / n).to(torch.float64)[:, None]
        kb = torch.fft.rfftfreq(n, d=1.0 / n).to(torch.float64)[None, :]
        lap = 4.0 * math.pi ** 2 * (ka * ka + kb * kb)
        amp = n * math.sqrt(2.0) * tau ** (alpha - 1.0) * (lap + tau * tau) ** (-alpha / 2.0)
        amp[0, 0] = 0.0
        amp[(ka.abs() == n // 2) | (kb == n // 2)] = 0.0
        return amp.to(torch.float32).to(device).contiguous()
    return _ns2d_table(("grf", n, tau, alpha, str(device)), make)


def navier_stokes_2d(w0: torch.Tensor, frames: int, substeps: int, dt: float, nu: float, forcing="li2020", filter=None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B, frames, N, N]: the vorticity of B trajectories of the 2-D incompressible Navier-Stokes equations on the unit torus,
    frame t after t * substeps sub-steps of length dt from w0 [B, N, N] (dlwp_ns2d_rollout_f32: pseudo-spectral, advective form,
    Crank-Nicolson on the viscous term, 2/3 rule; one workgroup per trajectory, the spectrum resident in LDS for the whole
    launch).  Frame 0 is w0 times `filter` in spectral space ([N, N / 2 + 1], real) without its modes |ka| = N / 2, kb = N / 2.
    forcing: "li2020", None, or a tensor [N, N].  A trajectory's bits depend on neither the batch nor on how frames * substeps is
    divided.  N in NS2D_SIZES and frames * substeps <= NS2D_MAX_STEPS, else the library refuses."""
    what = "navier_stokes_2d"
    _lib.require_cuda_tensor(w0, "w0")
    if w0.dim() != 3 or w0.shape[-1] != w0.shape[-2] or w0.shape[0] < 1:
        raise _lib.DlwpError(f"{what}: w0 must be [B, N, N] with B >= 1 (got {tuple(w0.shape)})")
    b, n = int(w0.shape[0]), int(w0.shape[-1])
    frames, substeps = int(frames), int(substeps)
    dev = w0.device
    if isinstance(forcing, str):
        if forcing != "li2020":
            raise _lib.DlwpError(f"{what}: forcing {forcing!r}; 'li2020', None or a tensor [N, N]")
        forcing = ns2d_li2020_forcing(n, dev) if n in NS2D_SIZES else None      # any other N: the library names the limit
    for name, t, shape in (("forcing", forcing, (n, n)), ("filter", filter, (n, n // 2 + 1))):
        if t is not None:
            _lib.require_cuda_tensor(t, name)
            if tuple(t.shape) != shape or t.device != dev:
                raise _lib.DlwpError(f"{what}: {name} must be {list(shape)} on {dev} (got {tuple(t.shape)} on {t.device})")
    if frames < 1 or substeps < 1:
        raise _lib.DlwpError(f"{what}: frames = {frames} and substeps = {substeps} must be at least 1")
    if out is None:
        out = torch.empty(b, frames, n, n, dtype=torch.float32, device=dev)
    else:
        _lib.require_cuda_tensor(out, "out")
        if tuple(out.shape) != (b, frames, n, n) or not out.is_contiguous() or out.device != dev:
            raise _lib.DlwpError(f"{what}: out must be a contiguous [{b}, {frames}, {n}, {n}] tensor on {dev}")
    _lib.launch("dlwp_ns2d_rollout_f32", dev, w0.contiguous(), filter.contiguous() if filter is not None else None,
                forcing.contiguous() if forcing is not None else None, out, b, n, frames, substeps, float(dt), float(nu))
    return out


def gaussian_random_field(shape_or_out, seed: int, offset: int = 0, tau: float = 7.0, alpha: float = 2.5, device=None) -> torch.Tensor:
    """Periodic Gaussian random fields [..., N, N] with the covariance of the FNO paper's GaussianRF: irfft2(rfft2(z) A) with
    z = philox_normal(seed, offset) of the same shape and A = grf_amplitude(N, tau, alpha) -- the device stream, then
    dlwp_ns2d_rollout_f32 with one frame and A as its filter, in place.  The field's standard deviation is near 0.29 at N = 64.
    `shape_or_out` as in philox_normal."""
    shape = tuple(int(v) for v in (shape_or_out.shape if isinstance(shape_or_out, torch.Tensor) else shape_or_out))
    if len(shape) < 2 or shape[-1] != shape[-2] or 0 in shape:
        raise _lib.DlwpError(f"gaussian_random_field: fields [..., N, N] are needed (got {shape})")
    z = philox_normal(shape_or_out, seed, offset, device=device)
    n = int(z.shape[-1])
    flat = z.view(-1, n, n)
    amp = grf_amplitude(n, tau, alpha, z.device) if n in NS2D_SIZES else torch.zeros(n, n // 2 + 1, device=z.device)
    navier_stokes_2d(flat, 1, 1, 1.0, 0.0, forcing=None, filter=amp, out=flat.view(-1, 1, n, n))
    return z
