"""Ensemble forecasts of the diffusion backbones on the GPU: rollout.rollout_chunks with a noise scheduler, ensemble_forecast,
ensemble_chunks, and the chunks fed to metrics.EnsembleMetrics.

The noise of a member is a function of (seed, member, per-member shape, call order): everything that only reorders or
regroups draws is bitwise.  Forecasts of the same members run in groups of another size are held to the project's fp32
bound (rel-L2 <= 1e-5 per step): the noise is identical, but the batch size may select another kernel variant."""
import numpy as np
import pytest
import torch

import ensemble_ref
from helpers import per_step_rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 3


def _perturbed(model, seed):
    """default initialisation plus a little noise on every parameter: no layer that starts at zero stays there"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    return model.to(DEV).eval()


@pytest.fixture(scope="module")
def latlon():
    """(model, constants, prescribed, prognostic [2, 1 + K, 2, 8, 16]) of a tiny DiffModernUNet"""
    import dlwp_benchmark_amd.models as M

    torch.manual_seed(0)
    model = M.DiffModernUNet(constant_channels=1, prescribed_channels=1, prognostic_channels=2, hidden_channels=[8, 16],
                             context_size=1, norm=False, use_scale_shift_norm=False, num_refinement_step=3)
    g = torch.Generator().manual_seed(1)
    cons = torch.randn(2, 1, 1, 8, 16, generator=g).to(DEV)
    presc = torch.randn(2, 1 + K, 1, 8, 16, generator=g).to(DEV)
    prog = torch.randn(2, 1 + K, 2, 8, 16, generator=g).to(DEV)
    return _perturbed(model, 2), cons, presc, prog


def _scheduler(seed=5):
    from dlwp_benchmark_amd.schedulers import RefinerScheduler

    s = RefinerScheduler.pde_refiner(3, 4e-3, seed=seed)
    s.set_timesteps(3)
    return s


@pytest.fixture(scope="module")
def one_shot(latlon):
    """the plain forward after reseed(): computed once, shared, left unchanged"""
    model, cons, presc, prog = latlon
    s = _scheduler()
    out = model(constants=cons, prescribed=presc, prognostic=prog, noise_scheduler=s)
    assert out.shape == (2, K, 2, 8, 16) and bool(torch.isfinite(out).all())
    return out, s.offset


@pytest.mark.parametrize("chunk_steps", [1, 2, 3])
@pytest.mark.parametrize("forcing", ["tensor", "callable"])
def test_chunked_rollout_is_the_one_shot_forward_bitwise(latlon, one_shot, chunk_steps, forcing):
    from dlwp_benchmark_amd.rollout import rollout_chunks

    model, cons, presc, prog = latlon
    want, want_offset = one_shot
    s = _scheduler(seed=99).reseed(5)
    presc_arg = presc if forcing == "tensor" else (lambda f0, f1: presc[:, f0:f1])
    seen = 0
    for s0, out in rollout_chunks(model, cons, presc_arg, prog[:, :1], K, chunk_steps, noise_scheduler=s):
        assert s0 == seen and torch.equal(out, want[:, s0:s0 + out.shape[1]]), (chunk_steps, s0)
        seen += out.shape[1]
    assert seen == K and s.offset == want_offset


def test_scheduler_for_a_deterministic_model_is_refused(latlon):
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd.lib import DlwpError
    from dlwp_benchmark_amd.rollout import ensemble_chunks, ensemble_forecast, rollout_chunks

    model, cons, presc, prog = latlon
    unet = M.UNet(constant_channels=2, prescribed_channels=1, prognostic_channels=2, hidden_channels=[4, 8], n_convolutions=2,
                  context_size=2)
    x = torch.zeros(1, 2, 2, 8, 16, device=DEV)
    with pytest.raises(DlwpError, match="no diffusion backbone"):
        rollout_chunks(unet, None, None, x, 2, 1, noise_scheduler=_scheduler())
    with pytest.raises(DlwpError, match="no diffusion backbone"):
        ensemble_chunks(unet, _scheduler(), None, None, x, 2, 1, 2)
    with pytest.raises(DlwpError, match="no diffusion backbone"):
        ensemble_forecast(unet, _scheduler(), None, None, x, 2)

    class TorchStyleScheduler:          # the part of diffusers' interface the model uses, and no member streams
        timesteps = torch.tensor([2, 1, 0])

        def step(self, pred, k, sample):
            raise AssertionError("not reached")

    for members in (1, 2):
        with pytest.raises(DlwpError, match="set_members"):
            ensemble_forecast(model, TorchStyleScheduler(), cons, presc, prog, members)
        with pytest.raises(DlwpError, match="set_members"):
            ensemble_chunks(model, TorchStyleScheduler(), cons, presc, prog[:, :1], K, 1, members)
    with pytest.raises(DlwpError, match="members"):
        ensemble_forecast(model, _scheduler(), cons, presc, prog, 0)


def test_one_member_is_the_plain_forward_bitwise(latlon, one_shot):
    from dlwp_benchmark_amd.rollout import ensemble_forecast

    model, cons, presc, prog = latlon
    s = _scheduler()
    ens = ensemble_forecast(model, s, cons, presc, prog, 1)
    assert ens.shape == (1, 2, K, 2, 8, 16) and torch.equal(ens[0], one_shot[0]) and s.offset == one_shot[1]


def test_three_members_differ_repeat_and_restore(latlon, one_shot):
    from dlwp_benchmark_amd.rollout import ensemble_forecast

    model, cons, presc, prog = latlon
    s = _scheduler()
    s.set_members(1, 9)                                   # whatever the caller had set comes back
    ens = ensemble_forecast(model, s, cons, presc, prog, 3)
    assert (s.members, s.first_member) == (1, 9)
    assert ens.shape == (3, 2, K, 2, 8, 16) and bool(torch.isfinite(ens).all())
    assert s.offset == one_shot[1]                        # the offset a single-member run uses
    for i in range(3):
        for j in range(i + 1, 3):
            assert not torch.equal(ens[i], ens[j]), (i, j)
    s.reseed()
    assert torch.equal(ensemble_forecast(model, s, cons, presc, prog, 3), ens)
    # member 0 of the ensemble has the noise of the plain forward; its batch neighbours may select another kernel variant
    errs = per_step_rel_l2(ens[0], one_shot[0])
    print(f"member 0 of 3 against the plain forward: per-step rel L2 {['%.2e' % e for e in errs]}")
    assert max(errs) <= 1e-5


def test_member_setting_is_restored_on_an_exception(latlon):
    from dlwp_benchmark_amd.rollout import ensemble_chunks, ensemble_forecast
    from dlwp_benchmark_amd.schedulers import RefinerScheduler

    class Failing(RefinerScheduler):
        def randn(self, shape, device):
            assert (self.members, self.first_member) == (2, 6)
            raise RuntimeError("no noise today")

    model, cons, presc, prog = latlon
    s = Failing.pde_refiner(3, 4e-3)
    s.set_timesteps(3)
    s.set_members(1, 4)
    with pytest.raises(RuntimeError, match="no noise today"):
        ensemble_forecast(model, s, cons, presc, prog, 2, first_member=6)
    assert (s.members, s.first_member) == (1, 4)
    with pytest.raises(RuntimeError, match="no noise today"):
        next(ensemble_chunks(model, s, cons, presc, prog[:, :1], K, 2, 2, first_member=6))
    assert (s.members, s.first_member) == (1, 4)


def test_group_invariance_of_forecasts(latlon):
    """members 0..3 at once against the groups (0, 2) and (2, 2): identical noise, rel-L2 <= 1e-5 per step"""
    from dlwp_benchmark_amd.rollout import ensemble_forecast

    model, cons, presc, prog = latlon
    s = _scheduler()
    whole = ensemble_forecast(model, s, cons, presc, prog, 4)
    groups = []
    for first in (0, 2):
        s.reseed()
        groups.append(ensemble_forecast(model, s, cons, presc, prog, 2, first_member=first))
    groups = torch.cat(groups)
    worst = 0.0
    for m in range(4):
        errs = per_step_rel_l2(groups[m], whole[m])
        worst = max(worst, max(errs))
        assert max(errs) <= 1e-5, (m, errs)
    print(f"group invariance, 4 members at once against 2 + 2: worst per-step rel L2 {worst:.3e}")
    assert not torch.equal(whole[2], whole[0])


def test_healpix_backbone(latlon):
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd.rollout import ensemble_chunks, ensemble_forecast

    torch.manual_seed(3)
    model = _perturbed(M.DiffMUNetHPX(constant_channels=1, prescribed_channels=0, prognostic_channels=2, hidden_channels=[8, 16],
                                      context_size=1, norm=True, num_refinement_step=3), 4)
    g = torch.Generator().manual_seed(6)
    cons = torch.randn(2, 1, 1, 12, 4, 4, generator=g).to(DEV)
    prog = torch.randn(2, 1 + K, 2, 12, 4, 4, generator=g).to(DEV)
    s = _scheduler()
    plain = model(constants=cons, prognostic=prog, noise_scheduler=s)
    s.reseed()
    ens = ensemble_forecast(model, s, cons, None, prog, 3)
    assert ens.shape == (3, 2, K, 2, 12, 4, 4) and bool(torch.isfinite(ens).all())
    assert max(per_step_rel_l2(ens[0], plain)) <= 1e-5 and not torch.equal(ens[1], ens[2])
    s.reseed()
    got = torch.cat([c.clone() for _, c in ensemble_chunks(model, s, cons, None, prog[:, :1], K, 2, 3)], dim=2)
    assert torch.equal(got, ens) and (s.members, s.first_member) == (1, 0)


def test_chunks_into_the_scores(latlon):
    """ensemble_chunks feeding EnsembleMetrics.update chunk by chunk against one update on the concatenated ensemble, and both
    against the float64 restatement"""
    from dlwp_benchmark_amd.metrics import EnsembleMetrics
    from dlwp_benchmark_amd.rollout import ensemble_chunks, ensemble_forecast

    model, cons, presc, prog = latlon
    m = 4
    lats = torch.linspace(-78.75, 78.75, 8)
    truth = prog[:, 1:].contiguous()
    s = _scheduler()
    streamed = EnsembleMetrics(lats, m, K, 2)
    kept = []
    for s0, chunk in ensemble_chunks(model, s, cons, lambda f0, f1: presc[:, f0:f1], prog[:, :1], K, 2, m):
        assert chunk.shape[:2] == (m, 2)
        streamed.update(chunk, truth[:, s0:s0 + chunk.shape[2]], step_begin=s0)
        kept.append(chunk.clone())
    assert (s.members, s.first_member) == (1, 0)
    ens = torch.cat(kept, dim=2)
    s.reseed()
    assert torch.equal(ens, ensemble_forecast(model, s, cons, presc, prog, m))
    once = EnsembleMetrics(lats, m, K, 2)
    once.update(ens, truth)
    a, b = streamed.state(), once.state()
    assert torch.equal(a["ranks"], b["ranks"]) and torch.equal(a["count"], b["count"])
    latw = once.latw.double().numpy()
    want, want_ranks = ensemble_ref.sums_and_ranks(ens.cpu().numpy(), truth.cpu().numpy(), latw)
    bound = ensemble_ref.bounds(ens.cpu().numpy(), truth.cpu().numpy(), latw)
    for name, st in (("streamed", a), ("once", b)):
        frac = np.abs(st["sums"].cpu().numpy() - want) / bound
        print(f"{name}: fraction of the bound used, per sum: {[f'{v:.3f}' for v in frac.max(axis=(1, 2))]}")
        assert (frac <= 1.0).all(), name
        assert np.array_equal(st["ranks"].cpu().numpy(), want_ranks), name
    sc = streamed.finalize()
    assert all(bool(torch.isfinite(sc[n]).all()) for n in ("rmse_mean", "spread", "spread_skill", "crps", "crps_ens"))
    assert bool((sc["crps"] <= sc["crps_ens"]).all()) and int(sc["rank_histogram"].sum()) == K * 2 * 2 * 8 * 16
