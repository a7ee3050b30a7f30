"""FNO2DModule / TFNO2DModule at channel widths outside the 32-channel kernels (csrc/spectral_any.hip) on the GPU:
rollouts against the restated oracle (oracle/restate/fno.py, the one the C2 tests use; network parity unpinned as
there), the properties the headline path guarantees (batch independence, bit determinism, one arithmetic for every
precision_form, HIP-graph replay), training against oracle autograd, and the edges of the domain.
Tolerance: per-step rel-L2 <= 1e-5 (fp32)."""
import pytest
import torch

from helpers import fno_std_fn, per_step_rel_l2, rel_l2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TOL = 1e-5


def _kw(hidden, lifting=64, projection=64, **over):
    kw = dict(n_modes=[12, 12], constant_channels=0, prescribed_channels=0, prognostic_channels=1,
              hidden_channels=hidden, lifting_channels=lifting, projection_channels=projection, n_layers=4,
              context_size=1)
    kw.update(over)
    return kw


def _pair(kw, gain=0.85):
    from dlwp_benchmark_amd.models import FNO2DModule
    from dlwp_benchmark_amd.weights import fill_state_dict
    from oracle.restate.fno import FNO2DModuleRef

    ref = FNO2DModuleRef(**kw).eval()
    fill_state_dict(ref, std_fn=fno_std_fn(gain), gain=gain)
    hip = FNO2DModule(**kw)
    hip.load_state_dict(ref.state_dict())
    return ref, hip.to(DEV).eval()


def _inputs(kw, b, t, h, w, seed=5):
    g = torch.Generator().manual_seed(seed)
    cc, cp, cg = kw["constant_channels"], kw["prescribed_channels"], kw["prognostic_channels"]
    const = torch.randn(b, 1, cc, h, w, generator=g) if cc else None
    presc = torch.randn(b, t, cp, h, w, generator=g) if cp else None
    prog = torch.randn(b, t, cg, h, w, generator=g)
    return const, presc, prog


def _dev(t):
    return t.to(DEV) if t is not None else None


@pytest.mark.parametrize("kw", [
    _kw(16), _kw(24), _kw(64), _kw(128, 128, 128),
    _kw(32, 40, 24),                                        # lifting / projection widths not multiples of 16
    _kw(24, 48, 40, n_modes=[10, 40]),                      # 21 kept columns
], ids=["h16", "h24", "h64", "h128", "lift40_proj24", "cols21"])
def test_rollout_matches_oracle(kw):
    from dlwp_benchmark_amd.synthetic import navier_stokes

    ref, hip = _pair(kw)
    _, _, prog = navier_stokes(2, 5)
    with torch.no_grad():
        want = ref(prognostic=prog)
    got = hip(prognostic=prog.to(DEV))
    torch.cuda.synchronize()
    errs = per_step_rel_l2(got, want)
    assert max(errs) <= TOL, errs


def test_wide_inputs_and_outputs_with_context():
    """in_channels = 2 + (1 + 17) * 3 = 56 > 32 and out_channels = 17 > 16: constants, prescribed and a three-frame
    context read straight from the rollout's segment table."""
    kw = _kw(24, 48, 40, n_modes=[8, 8], constant_channels=2, prescribed_channels=1, prognostic_channels=17,
             context_size=3)
    ref, hip = _pair(kw)
    c, p, g = _inputs(kw, 2, 6, 32, 64)
    with torch.no_grad():
        want = ref(constants=c, prescribed=p, prognostic=g)
    got = hip(constants=_dev(c), prescribed=_dev(p), prognostic=_dev(g))
    torch.cuda.synchronize()
    assert max(per_step_rel_l2(got, want)) <= TOL
    # dlwp_fno2d_forward_f32: one backbone step without the residual
    x = torch.cat([c[:, 0], p[:, :3].flatten(1, 2), g[:, :3].flatten(1, 2)], dim=1)
    with torch.no_grad():
        want1 = ref.fno(x)
    assert rel_l2(hip.one_step(x.to(DEV)), want1) <= TOL


def test_tfno_matches_fno_with_reconstructed_weights():
    from dlwp_benchmark_amd.models import FNO2DModule, TFNO2DModule
    from dlwp_benchmark_amd.synthetic import navier_stokes
    from dlwp_benchmark_amd.weights import fill_state_dict
    from oracle.restate.fno import FNO2DModuleRef

    kw = _kw(64)
    t = TFNO2DModule(rank=0.5, **kw)
    fill_state_dict(t, std_fn=lambda n, s: 0.3 if ("core" in n or "factor" in n) else None, gain=0.85)
    with torch.no_grad():
        for w in t.fno.fno_blocks.convs.weight:
            w.core.mul_(0.85 / 64 ** 0.5 / float(w.dense().abs().pow(2).mean().sqrt()))
    dense = FNO2DModule(**kw)
    sd = {k: v for k, v in t.state_dict().items() if ".core" not in k and ".factors." not in k}
    for l, w in enumerate(t.fno.fno_blocks.convs.weight):
        sd[f"fno.fno_blocks.convs.weight.{l}.tensor"] = w.dense().detach()
    dense.load_state_dict(sd)
    ref = FNO2DModuleRef(**kw).eval()
    ref.load_state_dict(sd)
    _, _, prog = navier_stokes(2, 4)
    with torch.no_grad():
        want = ref(prognostic=prog)
    a = t.to(DEV).eval()(prognostic=prog.to(DEV))
    b = dense.to(DEV).eval()(prognostic=prog.to(DEV))
    assert max(per_step_rel_l2(a, b)) <= 1e-6
    assert max(per_step_rel_l2(a, want)) <= TOL
    assert max(per_step_rel_l2(b, want)) <= TOL


def test_batch_independence_determinism_and_precision_forms():
    from dlwp_benchmark_amd.synthetic import navier_stokes

    _, hip = _pair(_kw(64))
    _, _, prog = navier_stokes(6, 4)
    p = prog.to(DEV)
    a = hip(prognostic=p)
    assert torch.equal(hip(prognostic=p), a)                          # run to run
    assert torch.equal(hip(prognostic=p[2:4].contiguous()), a[2:4])   # batch independence
    for form in ("bf16x6", "fp32_mfma", "f16x3"):                    # one fp32 arithmetic on the generic path
        for launch_form in (0, 3):
            hip.set_execution_form(precision_form=form, launch_form=launch_form)
            assert torch.equal(hip(prognostic=p), a), (form, launch_form)
    hip.verify()
    assert hip.fused_timeouts() == 0 and hip.range_reruns() == 0


def test_rollout_range_and_profiled_classes():
    import ctypes

    from dlwp_benchmark_amd import lib as L
    from dlwp_benchmark_amd.synthetic import navier_stokes

    _, hip = _pair(_kw(48))
    _, _, prog = navier_stokes(3, 6)
    p = prog.to(DEV)
    want = hip(prognostic=p)
    out = torch.zeros_like(want)
    hip.rollout_into(out, None, None, p, 0, 2)
    hip.rollout_into(out, None, None, p, 2, 5)
    assert torch.equal(out, want)
    lib = L.load()
    plan = hip._get_plan(64, 64, DEV)
    nbytes = lib.dlwp_fno2d_workspace_bytes(plan, 3)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ms = (ctypes.c_double * 5)()
    n = (ctypes.c_int32 * 5)()
    out2 = torch.empty_like(want)
    L.check(lib.dlwp_fno2d_rollout_profiled_f32(plan, None, 0, None, 0, p.data_ptr(), 1, 3, 6, 1, out2.data_ptr(),
                                                 ws.data_ptr(), nbytes, L.stream_ptr(), ms, n))
    assert torch.equal(out2, want)
    assert list(n) == [5, 5 * 4, 5 * 4, 5, 5]       # lifting, fwd + mix, inverse + epilogue per layer, projection, empty
    assert all(v >= 0.0 for v in ms)


def test_captured_step_replay_equals_eager():
    from dlwp_benchmark_amd.sharding import CapturedStep, ShardedRollout
    from dlwp_benchmark_amd.synthetic import navier_stokes

    _, model = _pair(_kw(64))
    runner = ShardedRollout(model, gather=False)
    _, _, prog = navier_stokes(4, 6, 64, 64, seed=99)
    prog = prog.to(DEV)
    want = runner(constants=None, prescribed=None, prognostic=prog).clone()
    cap = CapturedStep(lambda c, p, g: runner(constants=c, prescribed=p, prognostic=g), model=model)
    for i in range(4):
        got = cap(None, None, prog)
        torch.cuda.synchronize()
        assert torch.equal(got, want), i
    assert cap.replays >= 1
    model.verify()


def test_captured_step_replays_across_workspace_growth():
    """a recording made at batch 1 replays the same bits after an eager run at batch 4 has grown the model's workspace: the
    workspace it was recorded with stays allocated (lib.kept_workspace)"""
    from dlwp_benchmark_amd.sharding import CapturedStep, ShardedRollout
    from dlwp_benchmark_amd.synthetic import navier_stokes

    _, model = _pair(_kw(16))
    runner = ShardedRollout(model, gather=False)
    small = navier_stokes(1, 4, 32, 64, seed=7)[2].to(DEV)
    large = navier_stokes(4, 4, 32, 64, seed=8)[2].to(DEV)
    cap = CapturedStep(lambda c, p, g: runner(constants=c, prescribed=p, prognostic=g), model=model)
    cap(None, None, small)                      # eager
    got = cap(None, None, small)                # records and replays
    torch.cuda.synchronize()
    want = got.clone()
    cap(None, None, large)                      # eager at a larger batch: the workspace grows
    assert len(model._ws[str(DEV)]) == 2
    got = cap(None, None, small)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert cap.replays >= 2
    model.verify()


def test_a_larger_batch_keeps_the_first_workspace():
    """a recorded step replays against the workspace address it was recorded with, so a batch that needs a larger workspace
    must leave the first one allocated"""
    from dlwp_benchmark_amd import lib as L

    _, model = _pair(_kw(16))
    plan = model._get_plan(32, 64, DEV)
    need = {b: int(L.load().dlwp_fno2d_workspace_bytes(plan, b)) for b in (1, 4)}
    assert 256 <= need[1] < need[4], need
    model.one_step(torch.randn(1, 1, 32, 64, device=DEV))
    first = model._ws[str(DEV)][-1]
    ptr = first.data_ptr()
    assert first.numel() == need[1]
    model.one_step(torch.randn(4, 1, 32, 64, device=DEV))
    torch.cuda.synchronize()
    bufs = model._ws[str(DEV)]
    assert len(bufs) == 2 and bufs[0] is first and first.data_ptr() == ptr
    assert bufs[-1].numel() >= need[4] and bufs[-1].data_ptr() != ptr


def test_spectral_layers_keep_their_first_workspace():
    """the same for SpectralConv2d's inference workspace and for its training operator's (forward, backward-data and weight
    gradient share one)"""
    from dlwp_benchmark_amd import lib as L
    from dlwp_benchmark_amd.models import SpectralConv2d

    lib = L.load()
    layer = SpectralConv2d(4, 4, 4, 4).to(DEV).eval()
    x = {b: torch.randn(b, 4, 16, 16, device=DEV) for b in (1, 4)}
    plan = layer._get_plan(16, 16, DEV)
    need = {b: max(int(lib.dlwp_spectral_conv2d_workspace_bytes(plan, b)), 256) for b in (1, 4)}
    assert need[1] < need[4], need
    with torch.no_grad():
        layer(x[1])
        first = layer._ws[str(DEV)][-1]
        ptr = first.data_ptr()
        assert first.numel() == need[1]
        layer(x[4])
    bufs = layer._ws[str(DEV)]
    assert len(bufs) == 2 and bufs[0] is first and first.data_ptr() == ptr and bufs[-1].numel() >= need[4]

    layer.train()
    layer(x[1].clone().requires_grad_()).square().sum().backward()
    op = layer._train_op
    need = {b: max(int(lib.dlwp_spectral_conv2d_workspace_bytes(op._fwd, b)), int(lib.dlwp_spectral_conv2d_workspace_bytes(op._adj, b)),
                   int(lib.dlwp_spectral_conv2d_wgrad_workspace_bytes(op._fwd, b)), 256) for b in (1, 4)}
    assert need[1] < need[4], need
    kept = list(op._ws[str(DEV)])              # (the backward may have grown what the forward allocated)
    ptrs = [t.data_ptr() for t in kept]
    assert need[1] <= kept[-1].numel() < need[4]
    layer(x[4].clone().requires_grad_()).square().sum().backward()
    torch.cuda.synchronize()
    assert layer._train_op is op
    bufs = op._ws[str(DEV)]
    assert len(bufs) > len(kept) and bufs[-1].numel() >= need[4]
    assert all(a is b for a, b in zip(bufs, kept)) and [t.data_ptr() for t in kept] == ptrs
    assert all(bool(torch.isfinite(p.grad).all()) for p in layer.parameters())


def test_training_step_matches_oracle_autograd_at_hidden_16():
    from dlwp_benchmark_amd.models import FNO2DModule
    from dlwp_benchmark_amd.synthetic import navier_stokes
    from dlwp_benchmark_amd.weights import fill_state_dict
    from oracle.restate.fno import FNO2DModuleRef

    kw = dict(n_modes=[8, 8], constant_channels=0, prescribed_channels=0, prognostic_channels=2, hidden_channels=16,
              lifting_channels=40, projection_channels=24, n_layers=3, context_size=1)
    model = FNO2DModule(**kw)
    fill_state_dict(model, std_fn=lambda n, s: 0.85 / s[0] ** 0.5 if "convs.weight" in n else None, gain=0.85)
    ref = FNO2DModuleRef(**kw)
    ref.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    prog = navier_stokes(3, 4, 32, 64, channels=2, seed=11)[2]
    target = navier_stokes(3, 3, 32, 64, channels=2, seed=12)[2]

    def step(m, dev):
        m = m.to(dev).train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        opt.zero_grad()
        out = m(prognostic=prog.to(dev))
        loss = torch.nn.functional.mse_loss(out, target.to(dev))
        loss.backward()
        grads = {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}
        opt.step()
        with torch.no_grad():
            m.eval()
            after = m(prognostic=prog.to(dev)).cpu()
        return float(loss.detach()), grads, after

    loss_g, grads_g, after_g = step(model, DEV)
    loss_c, grads_c, after_c = step(ref, "cpu")
    assert abs(loss_g - loss_c) <= 1e-5 * abs(loss_c)
    assert set(grads_g) == set(grads_c)
    for k in grads_c:
        gg = torch.view_as_real(grads_g[k]) if grads_g[k].is_complex() else grads_g[k]
        gc = torch.view_as_real(grads_c[k]) if grads_c[k].is_complex() else grads_c[k]
        assert rel_l2(gg, gc) < 1e-4, k
    assert rel_l2(after_g, after_c) < 1e-4


@pytest.mark.parametrize("over", [dict(hidden_channels=513), dict(lifting_channels=600)])
def test_out_of_domain_is_unsupported(over):
    from dlwp_benchmark_amd.lib import DlwpError
    from dlwp_benchmark_amd.models import FNO2DModule

    kw = _kw(32)
    kw.update(over)
    hip = FNO2DModule(**kw).to(DEV).eval()
    with pytest.raises(DlwpError, match="status -2"):
        hip(prognostic=torch.zeros(1, 2, 1, 64, 64, device=DEV))


def test_generic_plan_keeps_the_width_rule():
    from dlwp_benchmark_amd.lib import DlwpError

    _, hip = _pair(_kw(64))
    with pytest.raises(DlwpError, match="status -2"):
        hip(prognostic=torch.zeros(1, 2, 1, 64, 48, device=DEV))
