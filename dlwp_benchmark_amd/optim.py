"""The training step's tail on the kernels of csrc/optim.hip: what the reference's scripts/train.py does
once the gradients exist -- `clip_grad_norm_` (train.py:299-305), `th.optim.AdamW.step()` (train.py:59,309), `zero_grad()`
(train.py:186) and `ema.update()` (train.py:312) -- each as ONE launch over all parameter tensors through a device table.

    optimizer = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-5)
    ...
    clip_grad_norm_(optimizer, max_norm)         # or clip_grad_norm_(model.parameters(), max_norm)
    optimizer.step()                             # or optimizer.step(clip_max_norm=max_norm): norm, clip and update in one call

Nothing here synchronises with the device or reads a device value on the host: the step counts, the clip coefficient and
the learning rates live in device memory, so clip + step can be recorded in a HIP graph and replayed.  The host only compares
data pointers and hyper-parameters with what the table holds and refreshes the table (one asynchronous copy from a fresh
pinned buffer) when they changed.  There is no CPU fallback.
"""
import weakref
from typing import List, Sequence

import torch

from . import lib as _lib

_HYPER = 5       # doubles per group in the device block: lr, beta1, beta2, eps, weight_decay  (csrc/optim.hip)
_DERIVED = 8     # floats per tensor the AdamW header kernel fills
_ALIGN = 4       # elements: state offsets are multiples of 16 bytes


def chunk_elems() -> int:
    """elements of one chunk of the multi-tensor kernels (dlwp_mt_chunk_elems)"""
    return int(_lib.load().dlwp_mt_chunk_elems())


def build_table(numels: Sequence[int], chunk: int, align: int = _ALIGN) -> dict:
    """The host form of the multi-tensor table, in pure Python: for tensors of `numels` elements, chunks of at most `chunk`
    elements of one tensor that cover every element exactly once (`chunk_tensor`, `chunk_first`), and for every tensor the
    offset of its state in a flat arena (`state_off`, multiples of `align` elements, no overlap; `state_elems` in all).  A
    tensor of 0 elements has no chunk."""
    chunk_tensor: List[int] = []
    chunk_first: List[int] = []
    state_off: List[int] = []
    off = 0
    for t, n in enumerate(numels):
        n = int(n)
        if n < 0:
            raise _lib.DlwpError(f"tensor {t} has {n} elements")
        state_off.append(off)
        off += (n + align - 1) // align * align
        for first in range(0, n, chunk):
            chunk_tensor.append(t)
            chunk_first.append(first)
    return {"numel": [int(n) for n in numels], "chunk_tensor": chunk_tensor, "chunk_first": chunk_first,
            "state_off": state_off, "state_elems": off}


def _upload(values, dtype, device) -> torch.Tensor:
    """a new device tensor from host values, through pinned memory (no host wait)"""
    host = torch.tensor(values, dtype=dtype).pin_memory()
    return host.to(device, non_blocking=True)


def _refresh(dst: torch.Tensor, values) -> None:
    """dst (device) = values: one asynchronous copy from a FRESH pinned buffer, which torch's host allocator keeps alive
    until the copy has run, so the next refresh cannot overwrite what this one still has to send"""
    if torch.cuda.is_current_stream_capturing():
        raise _lib.DlwpError("the multi-tensor table changed (gradient pointers or hyper-parameters) while a graph is being "
                             "captured: run one eager step, or call sync(), before the capture")
    dst.copy_(torch.tensor(values, dtype=dst.dtype).pin_memory(), non_blocking=True)


def _check_param(p, what: str = "parameter") -> None:
    if not isinstance(p, torch.Tensor):
        raise _lib.DlwpError(f"{what} is a {type(p).__name__}, not a tensor")
    if not p.is_cuda:
        raise _lib.DlwpError(f"{what} of shape {tuple(p.shape)} is on {p.device}: the fused optimizer path has no CPU fallback")
    if p.dtype not in (torch.float32, torch.complex64):
        raise _lib.DlwpError(f"{what} of shape {tuple(p.shape)} is {p.dtype}: float32 is needed (or complex64, taken as its "
                             "float32 pairs)")
    if not p.is_contiguous():
        raise _lib.DlwpError(f"{what} of shape {tuple(p.shape)} is not contiguous")


def _nfloats(p: torch.Tensor) -> int:
    """float32 values of a tensor: a complex64 tensor (the FNO's spectral weights) counts as its (real, imaginary) pairs, which
    is how torch.optim.AdamW (view_as_real), the 2-norm and the EMA treat it"""
    return p.numel() * (2 if p.is_complex() else 1)


class MultiTensorTable:
    """The device table of a fixed list of parameters (csrc/optim.hip): pointers, sizes, state offsets and chunks, built once;
    `sync()` brings the parameter and gradient pointers up to date."""

    def __init__(self, params: Sequence[torch.Tensor], track_grads: bool = True):
        self.params = list(params)
        self.track_grads = track_grads           # False: a table whose kernels never read the gradients (EMA)
        if not self.params:
            raise _lib.DlwpError("an empty parameter list")
        for p in self.params:
            _check_param(p)
        self.device = self.params[0].device
        if any(p.device != self.device for p in self.params):
            raise _lib.DlwpError("all parameters must be on one device")
        host = build_table([_nfloats(p) for p in self.params], chunk_elems())
        self.host = host
        self.n_tensors = len(self.params)
        self.n_chunks = len(host["chunk_tensor"])
        self.state_elems = host["state_elems"]
        dev = self.device
        self.numel = _upload(host["numel"], torch.int64, dev)
        self.state_off = _upload(host["state_off"], torch.int64, dev)
        self.chunk_tensor = _upload(host["chunk_tensor"] or [0], torch.int32, dev)
        self.chunk_first = _upload(host["chunk_first"] or [0], torch.int64, dev)
        self.p_ptrs = torch.zeros(self.n_tensors, dtype=torch.int64, device=dev)
        self.g_ptrs = torch.zeros(self.n_tensors, dtype=torch.int64, device=dev)
        self.partials = torch.zeros(max(self.n_chunks, 1), dtype=torch.float32, device=dev)
        self.scal = None                     # the [total_norm, clip_coef] block of the last grad_norm()
        self._p_seen: List[int] = []
        self._g_seen: List[int] = []
        self.sync()

    def state_view(self, arena: torch.Tensor, i: int) -> torch.Tensor:
        p = self.params[i]
        off = self.host["state_off"][i]
        flat = arena[off:off + _nfloats(p)]
        return torch.view_as_complex(flat.view(*p.shape, 2)) if p.is_complex() else flat.view(p.shape)

    def sync(self) -> None:
        """compares the (parameter, gradient) data pointers with the table's; one asynchronous copy each where they changed"""
        p_now = [p.data_ptr() for p in self.params]
        if p_now != self._p_seen:
            for p in self.params:
                _check_param(p)
            _refresh(self.p_ptrs, p_now)
            self._p_seen = p_now
        if not self.track_grads:
            return
        g_now = [0 if p.grad is None else p.grad.data_ptr() for p in self.params]
        if g_now != self._g_seen:
            for p in self.params:
                if p.grad is not None:
                    _check_param(p.grad, "gradient")
                    if p.grad.shape != p.shape or p.grad.dtype != p.dtype:
                        raise _lib.DlwpError("a gradient's shape or dtype differs from its parameter's")
            _refresh(self.g_ptrs, g_now)
            self._g_seen = g_now

    # the launches -----------------------------------------------------------------------------------------------------
    def grad_norm(self, max_norm: float) -> torch.Tensor:
        """launches the norm; returns the new [total_norm, clip_coef] device block (also kept as self.scal)"""
        self.scal = torch.empty(2, dtype=torch.float32, device=self.device)
        _lib.launch("dlwp_mt_grad_norm_f32", self.device, self.g_ptrs, self.numel, self.chunk_tensor, self.chunk_first,
                    self.n_chunks, self.partials, float(max_norm), self.scal)
        return self.scal

    def scale(self, scal: torch.Tensor) -> None:
        _lib.launch("dlwp_mt_scale_f32", self.device, self.g_ptrs, self.numel, self.chunk_tensor, self.chunk_first,
                    self.n_chunks, scal)

    def zero(self) -> None:
        _lib.launch("dlwp_mt_zero_f32", self.device, self.g_ptrs, self.numel, self.chunk_tensor, self.chunk_first,
                    self.n_chunks)


_clip_tables = {}        # tuple of id(parameter) -> (MultiTensorTable, weak references that prove the ids are still theirs)


def _table_for(params: Sequence[torch.Tensor]) -> MultiTensorTable:
    key = tuple(id(p) for p in params)
    hit = _clip_tables.get(key)
    if hit is not None and all(r() is p for r, p in zip(hit[1], params)):
        return hit[0]
    for k in [k for k, (_, refs) in _clip_tables.items() if any(r() is None for r in refs)]:
        del _clip_tables[k]                                  # lists whose parameters are gone
    table = MultiTensorTable(params)
    _clip_tables[key] = (table, [weakref.ref(p) for p in params])
    return table


def clip_grad_norm_(parameters, max_norm: float, norm_type: float = 2.0) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ (reference train.py:299-305) on two launches: the 2-norm of all gradients, then
    g *= min(1, max_norm / (norm + 1e-6)) in place.  `parameters`: a FusedAdamW (its table is used), a tensor, or an iterable
    of tensors (a table is built for the list and cached).  Returns the total norm as a 0-dim device tensor; nothing waits for
    the device.  Only norm type 2."""
    if float(norm_type) != 2.0:
        raise _lib.DlwpError(f"clip_grad_norm_: norm type {norm_type} is not supported, only 2")
    if isinstance(parameters, FusedAdamW):
        table = parameters.table()
    else:
        if isinstance(parameters, torch.Tensor):
            parameters = [parameters]
        table = _table_for(list(parameters))
    table.sync()
    scal = table.grad_norm(max_norm)
    table.scale(scal)
    return scal[0]


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (decoupled weight decay, torch's formula and defaults) on dlwp_mt_adamw_f32: one pass over all
    parameters, gradients and state.  Parameter groups with their own hyper-parameters are supported; `amsgrad`, `maximize`,
    non-fp32, non-contiguous and CPU parameters raise DlwpError (a complex64 parameter, the FNO's spectral weights, is taken as
    its float32 pairs, as torch's AdamW takes it through view_as_real).

    exp_avg, exp_avg_sq and the step counts live in flat device arenas the optimizer owns; `state[p]['exp_avg']` and
    `state[p]['exp_avg_sq']` are views into them (`state[p]['step']` is brought up to date by state_dict()).  state_dict() /
    load_state_dict() speak torch.optim.AdamW's layout, so checkpoints interchange in both directions.

    step() does not synchronise: a group's hyper-parameters are written to the device only when `param_groups` changed, the
    gradient pointers only when they changed.  zero_grad() keeps the gradient storage by default (zeroed in one launch), so
    the pointers stay fixed and a recorded step can be replayed; between replays, call sync() after changing `lr`."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, maximize: bool = False):
        if amsgrad:
            raise _lib.DlwpError("FusedAdamW: amsgrad is not supported")
        if maximize:
            raise _lib.DlwpError("FusedAdamW: maximize is not supported")
        if isinstance(lr, torch.Tensor):
            raise _lib.DlwpError("FusedAdamW: lr must be a number")
        if lr < 0 or eps < 0 or weight_decay < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
            raise ValueError("FusedAdamW: invalid hyper-parameter")
        # torch.optim.AdamW's own defaults, so param_groups (and a state_dict) carry exactly its keys
        defaults = dict(torch.optim.AdamW([torch.zeros(1)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay).defaults)
        super().__init__(params, defaults)
        for group in self.param_groups:
            for p in group["params"]:
                _check_param(p)
        self._table = None
        self.last_total_norm = None

    # the table and the arenas, built at first use ------------------------------------------------------------------------
    def _flat_params(self):
        return [p for group in self.param_groups for p in group["params"]]

    def table(self) -> MultiTensorTable:
        if self._table is None:
            params = self._flat_params()
            t = MultiTensorTable(params)
            dev = t.device
            self._group_of = _upload([gi for gi, g in enumerate(self.param_groups) for _ in g["params"]], torch.int32, dev)
            self._steps = torch.zeros(t.n_tensors, dtype=torch.int32, device=dev)
            self._derived = torch.zeros(t.n_tensors * _DERIVED, dtype=torch.float32, device=dev)
            self._hyper = torch.zeros(len(self.param_groups) * _HYPER, dtype=torch.float64, device=dev)
            self._hyper_seen = None
            self.exp_avg = torch.zeros(max(t.state_elems, _ALIGN), dtype=torch.float32, device=dev)
            self.exp_avg_sq = torch.zeros(max(t.state_elems, _ALIGN), dtype=torch.float32, device=dev)
            for i, p in enumerate(params):
                self.state[p] = {"step": torch.tensor(0.0, dtype=torch.float32),
                                 "exp_avg": t.state_view(self.exp_avg, i), "exp_avg_sq": t.state_view(self.exp_avg_sq, i)}
            self._table = t
        elif len(self._table.params) != sum(len(g["params"]) for g in self.param_groups):
            raise _lib.DlwpError("FusedAdamW: a parameter group was added after the first use; build a new optimizer")
        return self._table

    def _hyper_now(self):
        out = []
        for g in self.param_groups:
            if g.get("amsgrad") or g.get("maximize"):
                raise _lib.DlwpError("FusedAdamW: amsgrad and maximize are not supported")
            out += [float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"])]
        return out

    def sync(self) -> MultiTensorTable:
        """Brings the device table up to date with the host: gradient / parameter pointers and every group's hyper-parameters,
        each written only if it changed.  step(), zero_grad() and clip_grad_norm_ call it; call it yourself between replays of a
        recorded step after a scheduler changed `lr`."""
        t = self.table()
        t.sync()
        hyper = self._hyper_now()
        if hyper != self._hyper_seen:
            _refresh(self._hyper, hyper)
            self._hyper_seen = hyper
        return t

    @torch.no_grad()
    def step(self, closure=None, clip_max_norm=None):
        """One AdamW update of every parameter that has a gradient (one launch plus its one-thread-per-tensor header).
        clip_max_norm: the gradient norm, the clip and the update as one call -- the update consumes g * clip_coef without
        writing it back, so `.grad` then holds the UNCLIPPED values; the parameters are bit for bit those of
        clip_grad_norm_(optimizer, clip_max_norm) followed by step().  The norm is left in `last_total_norm` (device)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        t = self.sync()
        scal = None
        if clip_max_norm is not None:
            scal = t.grad_norm(clip_max_norm)
            self.last_total_norm = scal[0]
        _lib.launch("dlwp_mt_adamw_f32", t.device, t.p_ptrs, t.g_ptrs, t.numel, t.state_off, self._group_of, self._steps,
                    self._derived, self._hyper, t.n_tensors, t.chunk_tensor, t.chunk_first, t.n_chunks, self.exp_avg,
                    self.exp_avg_sq, scal)
        return loss

    def zero_grad(self, set_to_none: bool = False):
        """set_to_none=False (the default HERE): the gradient storage stays and is zeroed by one launch of dlwp_mt_zero_f32, so
        the table's pointers stay valid.  True: torch's behaviour (the gradients are dropped)."""
        if set_to_none:
            return super().zero_grad(set_to_none=True)
        t = self.table()
        t.sync()
        t.zero()

    # checkpoints in torch.optim.AdamW's layout --------------------------------------------------------------------------
    def steps(self) -> List[int]:
        """the step count of every parameter, in param_groups order (reads the device: waits for it)"""
        self.table()
        return [int(s) for s in self._steps.cpu().tolist()]

    def state_dict(self):
        """torch.optim.AdamW's state_dict: per stepped parameter `step` (a float32 scalar), `exp_avg`, `exp_avg_sq`; and the
        param_groups.  Reads the step counts from the device (the one place that waits for it)."""
        steps = self.steps()
        for p, s in zip(self._table.params, steps):
            self.state[p]["step"] = torch.tensor(float(s), dtype=torch.float32)
        sd = super().state_dict()
        sd["state"] = {k: {"step": v["step"], "exp_avg": v["exp_avg"].clone(), "exp_avg_sq": v["exp_avg_sq"].clone()}
                       for k, v in sd["state"].items() if float(v["step"]) > 0}       # torch has no state before a first step
        return sd

    def load_state_dict(self, state_dict):
        """accepts a torch.optim.AdamW (or FusedAdamW) state_dict: the moments are copied into the arenas, the steps into the
        table"""
        t = self.table()
        params = list(t.params)
        for p in params:
            del self.state[p]
        super().load_state_dict(state_dict)
        steps = []
        for i, p in enumerate(params):
            loaded = self.state.get(p) or {}
            m, v = t.state_view(self.exp_avg, i), t.state_view(self.exp_avg_sq, i)
            if "exp_avg" in loaded:
                m.copy_(loaded["exp_avg"])
                v.copy_(loaded["exp_avg_sq"])
                steps.append(int(round(float(loaded["step"]))))
            else:
                m.zero_()
                v.zero_()
                steps.append(0)
            self.state[p] = {"step": torch.tensor(float(steps[-1]), dtype=torch.float32), "exp_avg": m, "exp_avg_sq": v}
        self._steps.copy_(torch.tensor(steps, dtype=torch.int32))
        self._hyper_seen = None


class ExponentialMovingAverage:
    """The exponential moving average of a model's trainable parameters, with the calls reference train.py:71-72,312,332,462
    makes: register(), update(), apply_shadow(), restore().  update() is one launch of dlwp_mt_ema_f32:
    shadow = decay shadow + (1 - decay) p.  PARITY UNPINNED: the reference's helper_scripts/ema.py is not part of the reference
    tree; this is the usual PDE-Refiner form of the class."""

    def __init__(self, model: torch.nn.Module, decay: float):
        self.model = model
        self.decay = float(decay)
        self.shadow = {}
        self.backup = {}
        self._table = None

    def _named(self):
        return [(n, p) for n, p in self.model.named_parameters() if p.requires_grad]

    @torch.no_grad()
    def register(self):
        named = self._named()
        self._table = MultiTensorTable([p for _, p in named], track_grads=False)
        self._arena = torch.zeros(max(self._table.state_elems, _ALIGN), dtype=torch.float32, device=self._table.device)
        self.shadow = {}
        for i, (name, p) in enumerate(named):
            self.shadow[name] = self._table.state_view(self._arena, i)
            self.shadow[name].copy_(p)

    @torch.no_grad()
    def update(self):
        if self._table is None:
            raise _lib.DlwpError("ExponentialMovingAverage.update() before register()")
        t = self._table
        t.sync()
        _lib.launch("dlwp_mt_ema_f32", t.device, t.p_ptrs, t.numel, t.state_off, t.chunk_tensor, t.chunk_first, t.n_chunks,
                    self._arena, self.decay, 1.0 - self.decay)

    @torch.no_grad()
    def apply_shadow(self):
        for name, p in self._named():
            self.backup[name] = p.detach().clone()
            p.copy_(self.shadow[name])

    @torch.no_grad()
    def restore(self):
        for name, p in self._named():
            p.copy_(self.backup[name])
        self.backup = {}
