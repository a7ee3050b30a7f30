"""Device-resident autoregressive driver shared by the backbones whose step is a Python-level
composition of kernels (Swin, Pangu, FourCastNet, U-Net).

Restates the loop every reference backbone carries (canonical copy
models/swintransformer/swin_transformer.py:694-737; `_prepare_inputs` :679-692) with the two host-side
costs removed: the trajectory is written in place into a preallocated [B, T-ctx, Cg, H, W] buffer
(the reference rebuilds `torch.stack(outs)` every step, O(T^2) copies, and the fno/afno/convlstm
variants move every step to the CPU: fno.py:104, fourcastnet.py:359, convlstm.py:249), and nothing in the
loop synchronises with the host.
"""
from typing import Callable, Optional

import torch


def assemble_input(constants: Optional[torch.Tensor], prescribed: Optional[torch.Tensor],
                   frames) -> torch.Tensor:
    """`_prepare_inputs`: cat([constants[:,0], prescribed window (t c), prognostic window (t c)], 1).
    `frames` is the list of the context_size prognostic frames [B, Cg, H, W] (views, no copies)."""
    parts = []
    if constants is not None:
        parts.append(constants[:, 0])
    if prescribed is not None:
        b, t, c, h, w = prescribed.shape
        parts.append(prescribed.reshape(b, t * c, h, w))
    parts.extend(frames)
    if not torch.is_grad_enabled() and parts[0].is_cuda:
        from . import ops

        return ops.concat_channels(parts)          # one 16-byte copy kernel (dlwp_concat_channels_f32)
    return torch.cat(parts, dim=1)


def rollout_into(one_step: Callable[[torch.Tensor], torch.Tensor], context_size: int, out: torch.Tensor,
                 constants: Optional[torch.Tensor], prescribed: Optional[torch.Tensor], prognostic: torch.Tensor,
                 step_begin: int = 0, step_end: int = -1) -> torch.Tensor:
    """Runs rollout steps [step_begin, step_end) writing out[:, s] in place; earlier steps must be
    present in `out`.  Frame f of the window of step s (f in [s, s+ctx)) is the input frame f when
    f < ctx, else out[:, f - ctx]."""
    ctx = context_size
    n_steps = prognostic.shape[1] - ctx
    if step_end < 0:
        step_end = n_steps
    for s in range(step_begin, step_end):
        t = s + ctx
        frames = [prognostic[:, f] if f < ctx else out[:, f - ctx] for f in range(s, t)]
        x_t = assemble_input(constants, prescribed[:, t - ctx:t] if prescribed is not None else None, frames)
        inc = one_step(x_t)
        torch.add(frames[-1], inc, out=out[:, s])
    return out


def rollout_chunks(model, constants: Optional[torch.Tensor], prescribed, prognostic: torch.Tensor, n_steps: int,
                   chunk_steps: int, noise_scheduler=None, carry_state: bool = False):
    """A rollout of any length in fixed device memory: a generator of (step_begin, out_chunk), out_chunk [B, k, Cg, ...] holding
    rollout steps [step_begin, step_begin + k), k = chunk_steps (less in the last chunk).  `out_chunk` is a view of a reused
    buffer: valid until the next iteration.

    `prognostic` holds only the context_size initial frames [B, ctx, Cg, ...].  `prescribed` is None, a device tensor
    [B, ctx + n_steps, Cp, ...] or a callable (frame_begin, frame_end) -> device tensor [B, frame_end - frame_begin, Cp, ...]
    (`insolation_forcing` builds one): frame f is what the one-shot forward would find at prescribed[:, f].

    Every chunk is the model's own `rollout_into` (lat-lon tensors) or `forward` (HEALPix tensors, which the model folds
    itself) over a window whose ctx leading frames are the last ctx frames produced so far -- so the FNO persistent kernel, step
    graphs and precision forms run exactly as in a one-shot forward.  That is sound because every backbone that runs the
    shared loop above reads prognostic[:, :ctx] and the LENGTH of the window only (rollout_into: frame f < ctx comes from the
    input, every later one from `out`; the FNO kernels: csrc/fno2d.hip, fno_rollout_once, the same rule).  The driver holds
    three buffers of ctx + chunk_steps frames at most, whatever n_steps is, and does not synchronise with the host.

    ConvLSTM / ConvLSTMHPX carry a recurrent (h, c) state that starts at frame 0 and cannot be resumed from frames: without
    `carry_state` they are refused.  With carry_state=True the chunks are the model's own `forward_chunk`: the first one is its
    forward over the ctx initial frames and k steps, every later one continues from the state the one before returned (every
    cell's h and c and the last frame, 2 len(hidden_sizes) + 1 tensors), so the chunked run is bitwise the one-shot forward
    and the driver holds one chunk of output beside that state, whatever n_steps is.  The frames of `prescribed` asked for
    are then exactly those read: (0, ctx + k) for the first chunk, (ctx + s0, ctx + s0 + k) afterwards.  `out_chunk` is the
    model's tensor, valid until the next iteration like the reused buffer of the other models.  A model without
    `forward_chunk` is refused under carry_state=True.
    The diffusion backbones (DiffModernUNet, DiffMUNetHPX) need `noise_scheduler` and are refused without it; with it every
    chunk is their own forward(..., noise_scheduler=...), which draws per rollout step on per-step shapes, so a chunked run is
    bitwise the one-shot forward with a scheduler in the same state.  Other models take no scheduler."""
    from . import lib as _lib
    from .models.diffusion import DiffModernUNet
    from .models.unet import ConvLSTM

    carry_state = bool(carry_state)
    if isinstance(model, ConvLSTM) and not carry_state:
        raise _lib.DlwpError(f"rollout_chunks: {type(model).__name__} carries a recurrent (h, c) state that starts at frame 0 of a "
                             "forward and cannot be resumed from the last frames of a chunk: pass carry_state=True to hand the "
                             "state from chunk to chunk (forward_chunk)")
    if carry_state and not callable(getattr(model, "forward_chunk", None)):
        raise _lib.DlwpError(f"rollout_chunks: carry_state=True needs a model with forward_chunk (ConvLSTM, ConvLSTMHPX); "
                             f"{type(model).__name__} has no state to carry")
    diffusion = isinstance(model, DiffModernUNet)
    if diffusion and noise_scheduler is None:
        raise _lib.DlwpError(f"rollout_chunks: {type(model).__name__}.forward needs a noise scheduler: pass noise_scheduler=...")
    if not diffusion and noise_scheduler is not None:
        raise _lib.DlwpError(f"rollout_chunks: {type(model).__name__} is no diffusion backbone and takes no noise scheduler")
    ctx = int(model.context_size)
    n_steps, chunk_steps = int(n_steps), int(chunk_steps)
    if n_steps < 1 or chunk_steps < 1:
        raise _lib.DlwpError(f"rollout_chunks: n_steps = {n_steps} and chunk_steps = {chunk_steps} must be positive")
    _lib.require_cuda_tensor(prognostic, "prognostic")
    _lib.require_cuda_tensor(constants, "constants")
    if prognostic is None or prognostic.dim() < 5 or prognostic.shape[1] != ctx:
        raise _lib.DlwpError(f"rollout_chunks: prognostic must hold the {ctx} initial frames [B, {ctx}, C, ...], got "
                             f"{None if prognostic is None else tuple(prognostic.shape)}")
    fixed = isinstance(prescribed, torch.Tensor)
    if fixed:
        _lib.require_cuda_tensor(prescribed, "prescribed")
        if prescribed.shape[0] != prognostic.shape[0] or prescribed.shape[1] < ctx + n_steps:
            raise _lib.DlwpError(f"rollout_chunks: prescribed {tuple(prescribed.shape)} must hold {ctx + n_steps} frames of "
                                 f"{prognostic.shape[0]} samples")
    elif prescribed is not None and not callable(prescribed):
        raise _lib.DlwpError("rollout_chunks: prescribed must be None, a tensor or a callable (frame_begin, frame_end) -> tensor")
    b, frame = prognostic.shape[0], tuple(prognostic.shape[2:])
    fsz = 1
    for d in frame:
        fsz *= d
    kmax = min(chunk_steps, n_steps)
    dev = prognostic.device
    into = prognostic.dim() == 5 and hasattr(model, "rollout_into")      # the diffusion backbones have none
    constants = constants.contiguous() if constants is not None else None
    presc_buf = None

    def frames_of_prescribed(f0, f1):
        """frames [f0, f1) of `prescribed`, contiguous (None without prescribed channels)"""
        nonlocal presc_buf
        if prescribed is None:
            return None
        if fixed:
            presc = prescribed[:, f0:f1]
            if not presc.is_contiguous():
                if presc_buf is None:
                    presc_buf = torch.empty(b * (ctx + kmax) * (prescribed[0, 0].numel()), device=dev, dtype=torch.float32)
                view = presc_buf[:presc.numel()].view(presc.shape)
                view.copy_(presc)
                presc = view
            return presc
        presc = prescribed(f0, f1)
        _lib.require_cuda_tensor(presc, "prescribed(frame_begin, frame_end)")
        if presc is None or presc.shape[0] != b or presc.shape[1] != f1 - f0:
            raise _lib.DlwpError(f"rollout_chunks: prescribed({f0}, {f1}) must give [{b}, {f1 - f0}, Cp, ...], got "
                                 f"{None if presc is None else tuple(presc.shape)}")
        return presc.contiguous()

    def state_chunks():
        state = None
        for s0 in range(0, n_steps, kmax):
            k = min(kmax, n_steps - s0)
            presc = frames_of_prescribed(0, ctx + k) if s0 == 0 else frames_of_prescribed(ctx + s0, ctx + s0 + k)
            # (forward_chunk runs under no_grad itself; nothing is held across the yield)
            out, state = model.forward_chunk(constants=constants, prescribed=presc, prognostic=prognostic if s0 == 0 else None,
                                             state=state, steps=k)
            yield s0, out

    if carry_state:
        return state_chunks()
    context = prognostic.contiguous().clone()                                  # the last ctx frames produced so far
    win_buf = torch.zeros(b * (ctx + kmax) * fsz, device=dev, dtype=torch.float32)   # frames past ctx are never read
    out_buf = torch.empty(b * kmax * fsz, device=dev, dtype=torch.float32) if into else None

    def chunks():
        for s0 in range(0, n_steps, kmax):
            k = min(kmax, n_steps - s0)
            win = win_buf[:b * (ctx + k) * fsz].view(b, ctx + k, *frame)
            win[:, :ctx].copy_(context)
            presc = frames_of_prescribed(s0, s0 + ctx + k)
            with torch.no_grad():           # not held across the yield: the consumer keeps its own grad mode
                if into:
                    out = out_buf[:b * k * fsz].view(b, k, *frame)
                    model.rollout_into(out, constants, presc, win)
                elif diffusion:
                    out = model(constants=constants, prescribed=presc, prognostic=win, noise_scheduler=noise_scheduler)
                else:
                    out = model(constants=constants, prescribed=presc, prognostic=win)
                if k >= ctx:
                    context.copy_(out[:, k - ctx:])
                else:
                    context[:, :ctx - k].copy_(context[:, k:].clone())
                    context[:, ctx - k:].copy_(out)
            yield s0, out

    return chunks()


def _require_ensemble(model, noise_scheduler, members, first_member, what: str):
    from . import lib as _lib
    from .models.diffusion import DiffModernUNet

    if not isinstance(model, DiffModernUNet):
        raise _lib.DlwpError(f"{what}: {type(model).__name__} is no diffusion backbone (DiffModernUNet, DiffMUNetHPX): a "
                             "deterministic model has one forecast per initial condition")
    if not callable(getattr(noise_scheduler, "set_members", None)):
        raise _lib.DlwpError(f"{what}: the noise scheduler ({type(noise_scheduler).__name__}) has no set_members: member streams "
                             "need schedulers.RefinerScheduler")
    members, first_member = int(members), int(first_member)
    if members < 1 or first_member < 0:
        raise _lib.DlwpError(f"{what}: members = {members} must be at least 1 and first_member = {first_member} non-negative")
    return members, first_member


def _repeat_members(t: Optional[torch.Tensor], members: int) -> Optional[torch.Tensor]:
    """[B, ...] -> member-major [members * B, ...] (member m holds rows m B .. (m + 1) B - 1)"""
    if t is None or members == 1:
        return t
    return t.unsqueeze(0).expand(members, *t.shape).reshape(members * t.shape[0], *t.shape[1:])


def ensemble_chunks(model, noise_scheduler, constants: Optional[torch.Tensor], prescribed, prognostic: torch.Tensor, n_steps: int,
                    chunk_steps: int, members: int, first_member: int = 0):
    """An ensemble forecast of a diffusion backbone in fixed device memory: a generator of (step_begin, ens_chunk), ens_chunk
    [members, B, k, C, ...] holding rollout steps [step_begin, step_begin + k) of members first_member .. first_member +
    members - 1 -- a view of a reused buffer, valid until the next iteration.  The inputs (as rollout_chunks takes them;
    a callable `prescribed` is wrapped) are repeated member-major on the batch axis, the scheduler is put in member mode
    (schedulers.RefinerScheduler.set_members) for the run and restored afterwards, also on an exception, and everything else is
    rollout_chunks.  Member m's noise does not depend on the members beside it: an ensemble too large for the device runs in
    groups (first_member = 0, g, 2 g, ...), each after noise_scheduler.reseed(), and stays one ensemble."""
    from . import lib as _lib

    members, first_member = _require_ensemble(model, noise_scheduler, members, first_member, "ensemble_chunks")
    _lib.require_cuda_tensor(prognostic, "prognostic")
    if prognostic is None or prognostic.dim() < 5:
        raise _lib.DlwpError("ensemble_chunks: prognostic must hold the initial frames [B, ctx, C, ...]")
    b = prognostic.shape[0]
    if callable(prescribed) and not isinstance(prescribed, torch.Tensor):
        forcing = prescribed

        def prescribed(frame_begin, frame_end):
            return _repeat_members(forcing(frame_begin, frame_end), members)
    else:
        prescribed = _repeat_members(prescribed, members)

    def chunks():
        before = (noise_scheduler.members, noise_scheduler.first_member)
        noise_scheduler.set_members(members, first_member)
        try:
            for s0, out in rollout_chunks(model, _repeat_members(constants, members), prescribed,
                                          _repeat_members(prognostic, members), n_steps, chunk_steps,
                                          noise_scheduler=noise_scheduler):
                yield s0, out.view(members, b, *out.shape[1:])
        finally:
            noise_scheduler.set_members(*before)

    return chunks()


def ensemble_forecast(model, noise_scheduler, constants: Optional[torch.Tensor], prescribed: Optional[torch.Tensor],
                      prognostic: torch.Tensor, members: int, first_member: int = 0) -> torch.Tensor:
    """The one-shot form: [members, B, K, C, ...] from `prognostic` with all ctx + K frames, as the model's forward takes it (only
    the first ctx are read).  One forward over the member-major batch with the scheduler in member mode, restored afterwards."""
    from . import lib as _lib

    members, first_member = _require_ensemble(model, noise_scheduler, members, first_member, "ensemble_forecast")
    _lib.require_cuda_tensor(prognostic, "prognostic")
    before = (noise_scheduler.members, noise_scheduler.first_member)
    noise_scheduler.set_members(members, first_member)
    try:
        out = model(constants=_repeat_members(constants, members), prescribed=_repeat_members(prescribed, members),
                    prognostic=_repeat_members(prognostic, members), noise_scheduler=noise_scheduler)
    finally:
        noise_scheduler.set_members(*before)
    return out.view(members, prognostic.shape[0], *out.shape[1:])


def insolation_forcing(dates, lat_deg, lon_deg, batch: int, mean: Optional[float] = None, std: Optional[float] = None,
                       S: float = 1.0, device=None):
    """The callable form of `prescribed` for rollout_chunks when the prescribed variable is TOA insolation (the only one of the
    reference configs): (frame_begin, frame_end) -> [batch, frame_end - frame_begin, 1, *grid], generated on the device by
    ops.insolation for dates[frame_begin:frame_end] (one date per frame, ctx + n_steps in all) with the dataset's
    normalisation folded in, and repeated over the batch.  A few KB of tables go to the device per call, no field does.  The
    tensor is a reused buffer: valid until the next call."""
    import numpy as np

    from . import ops

    dates = np.asarray(dates, dtype="datetime64[us]").reshape(-1)
    bufs = {}

    def forcing(frame_begin: int, frame_end: int) -> torch.Tensor:
        n = frame_end - frame_begin
        if n < 1 or frame_begin < 0 or frame_end > len(dates):
            from . import lib as _lib

            raise _lib.DlwpError(f"insolation_forcing: frames [{frame_begin}, {frame_end}) outside the {len(dates)} dates given")
        buf = bufs.get(n)
        if buf is None:
            first = ops.insolation(dates[frame_begin:frame_end], lat_deg, lon_deg, S=S, mean=mean, std=std, device=device)
            buf = bufs[n] = torch.empty((batch, n, 1) + tuple(first.shape[1:]), device=first.device, dtype=torch.float32)
            buf[0, :, 0].copy_(first)
        else:
            ops.insolation(dates[frame_begin:frame_end], lat_deg, lon_deg, S=S, mean=mean, std=std, out=buf[0, :, 0])
        if batch > 1:
            buf[1:].copy_(buf[:1].expand_as(buf[1:]))
        return buf

    return forcing


def rollout_train(one_step: Callable[[torch.Tensor], torch.Tensor], context_size: int, constants: Optional[torch.Tensor],
                  prescribed: Optional[torch.Tensor], prognostic: torch.Tensor) -> torch.Tensor:
    """The same loop with autograd alive (reference scripts/train.py:263-271 trains through it): nothing in place, the
    trajectory is stacked once at the end."""
    ctx = context_size
    outs = []
    for s in range(prognostic.shape[1] - ctx):
        t = s + ctx
        frames = [prognostic[:, f] if f < ctx else outs[f - ctx] for f in range(s, t)]
        x_t = assemble_input(constants, prescribed[:, t - ctx:t] if prescribed is not None else None, frames)
        outs.append(frames[-1] + one_step(x_t))
    return torch.stack(outs, dim=1)
