"""FNO2DModule -- drop-in for reference models/fno/fno.py:12-106 on MI355X.

Same class name, constructor kwargs (fno.py:18-32) and forward(constants, prescribed, prognostic)
signature.  The reference builds `neuralop.models.FNO` (fno.py:38-47); that third-party module is
not part of the reference tree, so the sub-module tree below reproduces its published layout
(`lifting.fcs.{0,1}`, `fno_blocks.convs.weight.{l}.tensor` + `convs.bias`, `fno_blocks.fno_skips.{l}`,
`projection.fcs.{0,1}`) for the kwargs the reference passes.  PARITY UNPINNED at this boundary
(see DESIGN.md); the op-level building block is pinned through SpectralConv2d.

The whole rollout (fno.py:79-106: window selection, _prepare_inputs concat, backbone step,
residual add, stack) runs inside ONE C-ABI call, `dlwp_fno2d_rollout_f32`, on the current HIP
stream: no per-step `.cpu()` (fno.py:104), no O(T^2) `stack` (fno.py:92).
"""
import ctypes
from typing import List, Optional

import torch
from torch import nn

from .. import lib as _lib
from ._base import StepBackbone


class _DenseComplexTensor(nn.Module):
    def __init__(self, shape):
        super().__init__()
        self.tensor = nn.Parameter(torch.zeros(*shape, dtype=torch.cfloat))

    def dense(self) -> torch.Tensor:
        return self.tensor


def tucker_rank(shape, rank):
    """Ranks of a Tucker factorisation holding `rank` (float) x the dense parameter count -- the rule the TFNO's
    tensor library applies (tensorly `validate_tucker_rank`, rounding="round", no fixed modes): with x the common
    fraction per mode, core + factors = prod(shape) x^n + sum(s_i^2) x = rank * prod(shape); rank_i = round(s_i x) >= 1.
    An int or a list is taken as is."""
    shape = [int(s) for s in shape]
    if isinstance(rank, (list, tuple)):
        return [int(r) for r in rank]
    if isinstance(rank, int) and not isinstance(rank, bool):
        return [min(int(rank), s) for s in shape]
    rank = float(rank)
    n = len(shape)
    full = 1.0
    for s_ in shape:
        full *= s_
    sq = float(sum(s_ * s_ for s_ in shape))
    f = lambda x: full * x ** n + sq * x - rank * full
    lo, hi = 0.0, max(rank, 1.0)
    for _ in range(200):     # bisection (f is increasing on [0, hi], f(0) < 0 <= f(hi))
        mid = 0.5 * (lo + hi)
        if f(mid) > 0.0:
            hi = mid
        else:
            lo = mid
    x = 0.5 * (lo + hi)
    return [max(int(round(s_ * x)), 1) for s_ in shape]


class _FactorList(nn.Module):
    def __init__(self, factors):
        super().__init__()
        for i, f in enumerate(factors):
            self.register_parameter(f"factor_{i}", f)

    def __iter__(self):
        i = 0
        while hasattr(self, f"factor_{i}"):
            yield getattr(self, f"factor_{i}")
            i += 1


class _TuckerComplexTensor(nn.Module):
    """Complex Tucker-factorised weight in the parameter layout of the TFNO's tensor library (tltorch
    `ComplexTuckerTensor`): `core` [r_0, .., r_{n-1}, 2] and `factors.factor_i` [dim_i, r_i, 2], complex numbers
    stored as trailing (re, im) pairs.  dense() = core x_0 F_0 x_1 F_1 ... (mode products)."""

    def __init__(self, shape, rank):
        super().__init__()
        self.shape = tuple(int(s_) for s_ in shape)
        self.rank = tuple(tucker_rank(self.shape, rank))
        self.core = nn.Parameter(torch.zeros(*self.rank, 2))
        self.factors = _FactorList([nn.Parameter(torch.zeros(d, r, 2)) for d, r in zip(self.shape, self.rank)])

    def dense(self) -> torch.Tensor:
        t = torch.view_as_complex(self.core.contiguous())
        letters = "abcdefgh"[:len(self.shape)]
        outl = "ijklmnop"[:len(self.shape)]
        for n, f in enumerate(self.factors):
            fc = torch.view_as_complex(f.contiguous())
            src = letters[:n].translate(str.maketrans(letters[:n], outl[:n])) + letters[n:]
            dst = src.replace(letters[n], outl[n])
            t = torch.einsum(f"{src},{outl[n]}{letters[n]}->{dst}", t, fc)
        return t


class _ChannelMLP(nn.Module):
    """neuralop MLP(n_layers=2): 1x1 convs with GELU in between."""

    def __init__(self, cin, chid, cout):
        super().__init__()
        self.fcs = nn.ModuleList([nn.Conv2d(cin, chid, 1), nn.Conv2d(chid, cout, 1)])


class _SpectralConvs(nn.Module):
    def __init__(self, channels, n_layers, mh, mw, tucker_rank_=None):
        super().__init__()
        shape = (channels, channels, mh, mw)
        self.weight = nn.ModuleList([_DenseComplexTensor(shape) if tucker_rank_ is None else
                                     _TuckerComplexTensor(shape, tucker_rank_) for _ in range(n_layers)])
        self.bias = nn.Parameter(torch.zeros(n_layers, channels, 1, 1))


class _FNOBlocks(nn.Module):
    def __init__(self, channels, n_layers, mh, mw, tucker_rank_=None):
        super().__init__()
        self.convs = _SpectralConvs(channels, n_layers, mh, mw, tucker_rank_)
        self.fno_skips = nn.ModuleList([nn.Conv2d(channels, channels, 1, bias=False) for _ in range(n_layers)])


class _FNO(nn.Module):
    def __init__(self, n_modes, in_channels, hidden_channels, lifting_channels, projection_channels,
                 out_channels, n_layers, tucker_rank_=None):
        super().__init__()
        self.n_modes = [int(m) for m in n_modes]
        self.lifting = _ChannelMLP(in_channels, lifting_channels, hidden_channels)
        self.fno_blocks = _FNOBlocks(hidden_channels, n_layers, self.n_modes[0], self.n_modes[1] // 2 + 1, tucker_rank_)
        self.projection = _ChannelMLP(hidden_channels, projection_channels, out_channels)


def kept_rows(h: int, n_modes_h: int):
    """Row bookkeeping of neuralop's fftshift-based SpectralConv (see oracle/restate/fno.py)."""
    m = min(h, n_modes_h)
    start = h - m
    pos = list(range(start // 2, h - (start + 1) // 2)) if start else list(range(h))
    sh = h // 2
    return [(p - sh) % h for p in pos], [(p + sh) % h for p in pos]


class FNO2DModule(StepBackbone):
    # the rollout is ONE persistent launch that needs every compute unit resident at once: nothing else (an RCCL
    # kernel of an overlapped collective) may occupy the chip beside it -- sharding.ShardedRollout honours this
    exclusive_launch = True

    def __init__(self, n_modes: list = [12, 12], constant_channels: int = 4, prescribed_channels: int = 1,
                 prognostic_channels: int = 8, hidden_channels: int = 32, lifting_channels: int = 256,
                 projection_channels: int = 256, n_layers: int = 4, max_n_modes: int = None, bias: bool = True,
                 context_size: int = 10, _tucker_rank=None, **kwargs):
        super().__init__()
        n_modes = [int(m) for m in n_modes]
        if len(n_modes) != 2:
            raise ValueError(f"n_modes must have two entries (2-D operator), got {n_modes}")
        if max_n_modes is not None and [int(m) for m in (max_n_modes if hasattr(max_n_modes, "__len__") else
                                                         [max_n_modes] * 2)] != n_modes:
            # the library would allocate max_n_modes-sized weights and use the n_modes corner: not reproduced
            raise NotImplementedError(f"max_n_modes={max_n_modes} != n_modes={n_modes} is not supported by the HIP path")
        # `bias` is accepted and NOT forwarded, exactly like the reference constructor (fno.py:29, :38-47): the
        # library's spectral-convolution bias stays at its default (present)
        self.context_size = int(context_size)
        self.constant_channels = int(constant_channels)
        self.prescribed_channels = int(prescribed_channels)
        self.prognostic_channels = int(prognostic_channels)
        in_channels = constant_channels + (prescribed_channels + prognostic_channels) * context_size
        self.in_channels = int(in_channels)
        self.fno = _FNO(n_modes=list(n_modes), in_channels=in_channels, hidden_channels=hidden_channels,
                        lifting_channels=lifting_channels, projection_channels=projection_channels,
                        out_channels=prognostic_channels, n_layers=n_layers, tucker_rank_=_tucker_rank)
        self._plan = None
        self._plan_key = None
        # execution form of the plan (struct dlwp_fno2d_desc): per-module state, fixed per plan, no process-wide switch
        # "f16x3" (default): the fused step kernel forms its big fp32 products from two-part f16 splits (fp32-GEMM accuracy
        # for |activation| < 65504; a range with a non-finite output is repeated on the bf16x6 kernels by itself);
        # "bf16x6": three-part bf16 splits everywhere (fp32 exponent range); "fp32_mfma": plain fp32-MFMA kernels +
        # unfused spectral path (independent cross-check)
        self.precision_form = "f16x3"
        self.launch_form = 0             # 0 fewest launches, 1 one per step, 2 three per step, 3 unfused kernels
        self.on_timeout = "rerun"        # or "raise": DLWP_ERR_TIMEOUT instead of the automatic re-run on the unfused kernels
        self.check = "per_call"          # or "deferred": asynchronous calls, the caller verifies with .check() (see there)
        self.lift_table = True           # one input channel: the fused step kernel reads the lifting MLP from a plan-time table
        self._debug_spin_limit = 0       # test hook: tiny hand-off spin bound to force the timeout path

    def set_execution_form(self, precision_form: Optional[str] = None, launch_form: Optional[int] = None,
                           on_timeout: Optional[str] = None, check: Optional[str] = None,
                           lift_table: Optional[bool] = None):
        if precision_form is not None:
            if precision_form not in ("f16x3", "bf16x6", "fp32_mfma"):
                raise _lib.DlwpError(f"unknown precision_form {precision_form!r}")
            self.precision_form = precision_form
        if launch_form is not None:
            if launch_form not in (0, 1, 2, 3):
                raise _lib.DlwpError(f"unknown launch_form {launch_form!r}")
            self.launch_form = int(launch_form)
        if on_timeout is not None:
            if on_timeout not in ("rerun", "raise"):
                raise _lib.DlwpError(f"unknown on_timeout {on_timeout!r}")
            self.on_timeout = on_timeout
        if check is not None:
            if check not in ("per_call", "deferred"):
                raise _lib.DlwpError(f"unknown check mode {check!r}")
            self.check = check
        if lift_table is not None:
            self.lift_table = bool(lift_table)
        return self

    def verify(self):
        """Deferred verification (`check="deferred"`): synchronises the current stream and raises DlwpError if a fused
        launch of the current plan timed out (status -5, DLWP_ERR_TIMEOUT) or an f16x3 range produced a non-finite output
        (status -6, DLWP_ERR_RANGE) since the last call of this method -- the pattern for throughput evaluation: many
        asynchronous rollouts, one verification.  In deferred mode NOTHING is repaired: the trajectories of a failed range
        are poisoned with NaN and this call is MANDATORY before they are used (`_get_plan` calls it by itself before a
        plan rebuild would drop the counters).  The same holds for launches recorded into a HIP graph: the per-call check
        cannot synchronise a capturing stream, so replays of a captured rollout are verified here, whatever `check` says.
        With the default `check="per_call"` outside graphs every call verifies (and repairs) itself and this passes."""
        if self._plan is not None:
            _lib.launch("dlwp_fno2d_status", next(self.parameters()).device, self._plan)
        return self

    def fused_timeouts(self) -> int:
        """fused launches of the current plan whose hand-off spin ran out (re-run on the unfused kernels or raised)"""
        return int(_lib.load().dlwp_fno2d_timeouts(self._plan)) if self._plan is not None else 0

    def lift_table_state(self) -> int:
        """the current plan's lifting table: 0 not applicable (or no plan yet), 1 in use, 2 rejected by the guard for these
        weights, 3 switched off (dlwp_fno2d_lift_table_state)"""
        return int(_lib.load().dlwp_fno2d_lift_table_state(self._plan)) if self._plan is not None else 0

    def range_reruns(self) -> int:
        """f16x3 step ranges of the current plan that were repeated on the bf16x6 kernels (non-finite output)"""
        return int(_lib.load().dlwp_fno2d_range_reruns(self._plan)) if self._plan is not None else 0

    # ------------------------------------------------------------------ plan management
    def _destroy_plan(self):
        if self._plan is not None:
            try:
                _lib.load().dlwp_fno2d_plan_destroy(self._plan)
            except Exception:
                pass
            self._plan = None

    def __del__(self):
        try:  # at interpreter shutdown torch internals may already be torn down
            self._destroy_plan()
        except Exception:
            pass

    def _get_plan(self, h: int, w: int, device):
        key = (h, w, str(device), self._param_key(), self.precision_form, self.launch_form, self.on_timeout,
               self._debug_spin_limit, self.check, self.lift_table)
        if self._plan is not None and key == self._plan_key:
            return self._plan
        if self._plan is not None and getattr(self, "_plan_check", None) == "deferred":
            # the sticky failure counters live in the plan: launches of the OLD plan that have not been verified yet are
            # verified now (raises DLWP_ERR_TIMEOUT / DLWP_ERR_RANGE here), before a rebuild would drop them
            self.verify()
        self._destroy_plan()
        f = self.fno
        host = lambda t: t.detach().to("cpu", torch.float32).contiguous()
        keep = []  # keep host tensors alive across the call

        def ptr(t):
            keep.append(t)
            return ctypes.c_void_p(t.data_ptr())

        L = len(f.fno_blocks.fno_skips)
        rows_in, rows_out = kept_rows(h, f.n_modes[0])
        n_rows = len(rows_in)
        n_cols = min(w // 2 + 1, f.n_modes[1] // 2 + 1)
        ri = (ctypes.c_int32 * n_rows)(*rows_in)
        ro = (ctypes.c_int32 * n_rows)(*rows_out)
        spec = (ctypes.c_void_p * L)()
        skip = (ctypes.c_void_p * L)()
        for l in range(L):
            wl = torch.view_as_real(f.fno_blocks.convs.weight[l].dense().detach().cpu().contiguous())
            wl = wl[:, :, :n_rows, :n_cols].contiguous().to(torch.float32)
            spec[l] = ptr(wl)
            skip[l] = ptr(host(f.fno_blocks.fno_skips[l].weight).reshape(
                f.fno_blocks.fno_skips[l].out_channels, -1).contiguous())
        d = _lib.FNO2dDesc()
        d.in_channels = self.in_channels
        d.hidden_channels = f.lifting.fcs[1].out_channels
        d.lifting_channels = f.lifting.fcs[0].out_channels
        d.projection_channels = f.projection.fcs[0].out_channels
        d.out_channels = self.prognostic_channels
        d.n_layers = L
        d.height, d.width = h, w
        d.n_rows, d.n_cols = n_rows, n_cols
        d.rows_in, d.rows_out = ri, ro
        d.fwd_scale = 1.0 / float(h * w)   # rfftn(norm="forward")
        d.inv_scale = 1.0                  # irfftn(norm="forward")
        d.lift_w1 = ptr(host(f.lifting.fcs[0].weight).reshape(d.lifting_channels, -1).contiguous())
        d.lift_b1 = ptr(host(f.lifting.fcs[0].bias))
        d.lift_w2 = ptr(host(f.lifting.fcs[1].weight).reshape(d.hidden_channels, -1).contiguous())
        d.lift_b2 = ptr(host(f.lifting.fcs[1].bias))
        d.spec_w = spec
        d.spec_b = ptr(host(f.fno_blocks.convs.bias).reshape(L, -1).contiguous())
        d.skip_w = skip
        d.proj_w1 = ptr(host(f.projection.fcs[0].weight).reshape(d.projection_channels, -1).contiguous())
        d.proj_b1 = ptr(host(f.projection.fcs[0].bias))
        d.proj_w2 = ptr(host(f.projection.fcs[1].weight).reshape(d.out_channels, -1).contiguous())
        d.proj_b2 = ptr(host(f.projection.fcs[1].bias))
        d.precision_form = {"bf16x6": 0, "fp32_mfma": 1, "f16x3": 2}[self.precision_form]
        d.launch_form = int(self.launch_form)
        d.on_timeout = 1 if self.on_timeout == "raise" else 0
        d.unchecked = 1 if self.check == "deferred" else 0
        d.debug_spin_limit = int(self._debug_spin_limit)
        d.lift_table = 0 if self.lift_table else 1
        plan = ctypes.c_void_p()
        _lib.launch("dlwp_fno2d_plan_create", device, ctypes.byref(plan), d)
        self._plan, self._plan_key, self._plan_check = plan, key, self.check
        return plan

    # ------------------------------------------------------------------ compute
    @torch.no_grad()
    def one_step(self, x_t: torch.Tensor) -> torch.Tensor:
        """`self.fno(x_t)` of fno.py:103 (no residual): [B, in, H, W] -> [B, out, H, W]."""
        _lib.require_cuda_tensor(x_t, "x_t")
        x_t = x_t.contiguous()
        b, c, h, w = x_t.shape
        if c != self.in_channels:
            raise _lib.DlwpError(f"x_t has {c} channels, model expects {self.in_channels}")
        plan = self._get_plan(h, w, x_t.device)
        y = torch.empty(b, self.prognostic_channels, h, w, device=x_t.device, dtype=torch.float32)
        nbytes = _lib.load().dlwp_fno2d_workspace_bytes(plan, b)
        ws = self._workspace(nbytes, x_t.device)
        _lib.launch("dlwp_fno2d_forward_f32", x_t.device, plan, x_t, y, b, ws, nbytes)
        return y

    def rollout_into(self, out: torch.Tensor, constants, prescribed, prognostic, step_begin: int = 0,
                     step_end: int = -1) -> torch.Tensor:
        """Runs rollout steps [step_begin, step_end) into `out` [B, T-ctx, Cg, H, W] (earlier steps
        must already be there).  Inputs are validated, contiguous CUDA tensors."""
        b, t, cg, h, w = prognostic.shape
        ctx = self.context_size
        cc = constants.shape[2] if constants is not None else 0
        cp = prescribed.shape[2] if prescribed is not None else 0
        lib = _lib.load()
        plan = self._get_plan(h, w, prognostic.device)
        nbytes = lib.dlwp_fno2d_workspace_bytes(plan, b)
        ws = self._workspace(nbytes, prognostic.device)
        with torch.cuda.device(prognostic.device):      # spelled out: the stream is not this entry point's last parameter
            _lib.check(lib.dlwp_fno2d_rollout_range_f32(
                plan, constants.data_ptr() if constants is not None else None, cc,
                prescribed.data_ptr() if prescribed is not None else None, cp,
                prognostic.data_ptr(), cg, b, t, ctx, out.data_ptr(), ws.data_ptr(), nbytes,
                _lib.stream_ptr(), step_begin, step_end), "dlwp_fno2d_rollout_range_f32")
        return out

    # ------------------------------------------------------------------ training (first slice)
    def _train_step(self, x_t: torch.Tensor) -> torch.Tensor:
        """One differentiable backbone step: spectral convolutions through the HIP kernels (forward, backward-data
        and weight gradient, dlwp_benchmark_amd/training.py), the pointwise parts through torch ops."""
        import torch.nn.functional as F

        from .. import training as T

        f = self.fno
        _, _, h, w = x_t.shape
        key = (h, w, str(x_t.device))
        if getattr(self, "_train_op_key", None) != key:
            rows_in, rows_out = kept_rows(h, f.n_modes[0])
            n_cols = min(w // 2 + 1, f.n_modes[1] // 2 + 1)
            self._train_op = T.SpectralOperator(f.lifting.fcs[1].out_channels, h, w, rows_in, rows_out, n_cols,
                                                1.0 / float(h * w), 1.0, x_t.device)
            self._train_op_key = key
        op = self._train_op
        hid = f.lifting.fcs[1](F.gelu(f.lifting.fcs[0](x_t)))
        n_layers = len(f.fno_blocks.fno_skips)
        for l in range(n_layers):
            wl = torch.view_as_real(f.fno_blocks.convs.weight[l].dense())[:, :, :len(op.rows_in), :op.n_cols]
            hid = T.spectral_conv(hid, wl, op) + f.fno_blocks.convs.bias[l] + f.fno_blocks.fno_skips[l](hid)
            if l < n_layers - 1:
                hid = F.gelu(hid)
        return f.projection.fcs[1](F.gelu(f.projection.fcs[0](hid)))

    def _forward_train(self, constants, prescribed, prognostic):
        """fno.py:79-106 with autograd alive (the loop the reference trains through, train.py:263-271)."""
        ctx = self.context_size
        outs = []
        for t in range(ctx, prognostic.shape[1]):
            t0 = max(0, t - ctx)
            if t == ctx:
                prog_t = prognostic[:, t0:t]
                presc_t = prescribed[:, t0:t] if prescribed is not None else None
            else:
                prog_t = torch.cat([prognostic[:, t0:ctx], torch.stack(outs, dim=1)[:, -ctx:]], dim=1)
                presc_t = prescribed[:, t - ctx:t] if prescribed is not None else None
            parts = []
            if constants is not None:
                parts.append(constants[:, 0])
            if presc_t is not None:
                parts.append(presc_t.flatten(1, 2))
            parts.append(prog_t.flatten(1, 2))
            outs.append(prog_t[:, -1] + self._train_step(torch.cat(parts, dim=1).contiguous()))
        return torch.stack(outs, dim=1)


class TFNO2DModule(FNO2DModule):
    """Drop-in for reference models/fno/fno.py:109-146 -- the class `configs/model/fno.yaml:1` names.  The reference
    builds `neuralop.models.TFNO(rank=rank)`: the FNO above with every spectral weight stored as a complex Tucker
    factorisation (`fno_blocks.convs.weight.{l}.core` / `.factors.factor_{i}`, tensorly-torch layout).  Here the dense
    weight is rebuilt from the factors when the plan is created (and whenever a factor changes: the plan is keyed on
    parameter versions), then the whole FNO path runs unchanged; in training mode the reconstruction is part of the
    autograd graph.  PARITY UNPINNED like FNO2DModule: both third-party libraries are absent from the reference tree
    and from this image."""

    def __init__(self, n_modes: list = [12, 12], constant_channels: int = 4, prescribed_channels: int = 1,
                 prognostic_channels: int = 8, hidden_channels: int = 32, lifting_channels: int = 256,
                 projection_channels: int = 256, n_layers: int = 4, max_n_modes: int = None, rank: float = 1.0,
                 bias: bool = True, context_size: int = 10, **kwargs):
        kwargs.pop("_tucker_rank", None)
        super().__init__(n_modes=n_modes, constant_channels=constant_channels, prescribed_channels=prescribed_channels,
                         prognostic_channels=prognostic_channels, hidden_channels=hidden_channels,
                         lifting_channels=lifting_channels, projection_channels=projection_channels, n_layers=n_layers,
                         max_n_modes=max_n_modes, bias=bias, context_size=context_size, _tucker_rank=rank, **kwargs)
        self.rank = rank
