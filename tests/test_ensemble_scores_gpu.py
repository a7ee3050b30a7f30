"""csrc/ensemble_scores.hip on the GPU through metrics.EnsembleMetrics, against the float64 restatement of the definitions
(tests/ensemble_ref.py: pairwise |x_i - x_j|, two-pass variance).

Bound (computed from each case's inputs): with A = max(max_m |x_m|, |y|) per point and u = 2^-24,
  |sums[q] - ref| <= 4 (M + 4) u sum w s^2 A^2 for q = 0, 1;  4 (M + 4) u sum w s A for q = 2;  4 (M + 4) M u sum w s A for q = 3
-- what the kernel's fp32 per-point arithmetic allows (M roundings in a member sum, a few more around it, a factor 4).  The
rank counts are integers and must be exact.  Every case prints the largest fraction of the bound it used."""
import numpy as np
import pytest
import torch

import ensemble_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEMBERS = [2, 3, 5, 16, 33, 64]          # the minimum, odd counts, one just above a padded size, the maximum
SHAPES = {"rows_not_x4": (2, 3, 2, 6, 10), "w64": (1, 2, 2, 5, 64),
          "three_blocks": (1, 1, 1, 33, 64)}      # 2112 points: workgroups of 1024 + 1024 + 64 reduce one (k, c); 528 KiB at M = 64
KINDS = ["unit", "tight", "offset300"]


def _lats(h):
    return torch.linspace(-90 + 90 / h, 90 - 90 / h, h)


def _inputs(m, shape, kind, seed=0):
    g = torch.Generator().manual_seed(1000 * m + seed)
    y = torch.randn(shape, generator=g)
    noise = torch.randn((m,) + tuple(shape), generator=g)
    x = y + (1e-3 if kind == "tight" else 1.0) * noise
    if kind == "offset300":
        x, y = x + 300.0, y + 300.0
    # ties: the target is a copy of a member at the first point, two members are equal at the second
    xf, yf = x.view(m, -1), y.view(-1)
    yf[0] = xf[m // 2, 0]
    xf[1, 1] = xf[0, 1]
    return x, y


def _metric(h, m, steps, c, std=None, **kw):
    from dlwp_benchmark_amd.metrics import EnsembleMetrics
    return EnsembleMetrics(_lats(h), m, steps, c, std=std, **kw)


def _check(em, x, y, scale, step_begin, label):
    """the metric's accumulators against the restatement of (x, y) at steps [step_begin, step_begin + K)"""
    k = x.shape[2]
    latw = em.latw.double().numpy()
    want, want_ranks = ensemble_ref.sums_and_ranks(x.numpy(), y.numpy(), latw, scale)
    bound = ensemble_ref.bounds(x.numpy(), y.numpy(), latw, scale)
    st = em.state()
    got, got_ranks = st["sums"].cpu().numpy(), st["ranks"].cpu().numpy()
    frac = np.abs(got[:, step_begin:step_begin + k] - want) / bound
    print(f"{label}: fraction of the bound used, per sum: {[f'{v:.3f}' for v in frac.max(axis=(1, 2))]}")
    assert (frac <= 1.0).all(), (label, frac.max(axis=(1, 2)))
    assert np.array_equal(got_ranks[step_begin:step_begin + k], want_ranks), label
    outside = np.ones(got.shape[1], dtype=bool)
    outside[step_begin:step_begin + k] = False
    assert not got[:, outside].any() and not got_ranks[outside].any(), f"{label}: wrote outside its steps"
    return want, want_ranks, bound


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("m", MEMBERS)
def test_sums_and_ranks(m, shape, kind):
    b, k, c, h, w = SHAPES[shape]
    x, y = _inputs(m, SHAPES[shape], kind)
    # (a) no scale, contiguous members, the chunk is the whole horizon
    em = _metric(h, m, k, c)
    em.update(x.to(DEV), y.to(DEV))
    _check(em, x, y, None, 0, f"M={m} {shape} {kind} plain")
    # (b) a scale, members a wider stride apart (a group view of a wider buffer), steps [2, 2 + K) of K + 2
    scale = np.array([2.0, 0.5])[:c]
    wide = torch.full((m + 1, x[0].numel() + 12), float("nan"), device=DEV)
    view = wide[1:, 4:4 + x[0].numel()].view(x.shape)
    view.copy_(x)
    assert view.stride(0) > x[0].numel() and not view.is_contiguous()
    em = _metric(h, m, k + 2, c, std=torch.from_numpy(scale))
    em.update(view, y.to(DEV), step_begin=2)
    _check(em, x, y, scale, 2, f"M={m} {shape} {kind} scale, stride, step_begin")
    assert em.state()["count"].tolist() == [0.0, 0.0] + [float(b)] * k


def test_steps_total_five_step_begin_two():
    m, (b, k, c, h, w) = 5, SHAPES["rows_not_x4"]
    x, y = _inputs(m, SHAPES["rows_not_x4"], "unit", seed=4)
    em = _metric(h, m, 5, c)
    em.update(x.to(DEV), y.to(DEV), step_begin=2)
    _check(em, x, y, None, 2, "steps_total 5, step_begin 2")
    sc = em.finalize()
    assert sc["rmse_mean"].shape == (5, c) and sc["rank_histogram"].shape == (5, c, m + 1)
    assert bool(torch.isfinite(sc["crps"][2:]).all()) and bool(torch.isnan(sc["crps"][:2]).all())
    want = ensemble_ref.scores(em.state()["sums"].cpu().numpy()[:, 2:], None, np.full(3, float(b)), m, h * w)
    for name in ("rmse_mean", "spread", "spread_skill", "crps", "crps_ens"):
        assert np.allclose(sc[name][2:].cpu().numpy(), want[name], rtol=1e-12), name


@pytest.mark.parametrize("m", [3, 64])
def test_two_runs_give_the_same_bits(m):
    shape = SHAPES["three_blocks"]
    x, y = _inputs(m, shape, "offset300", seed=1)
    xd, yd = x.to(DEV), y.to(DEV)
    runs = []
    for _ in range(2):
        em = _metric(shape[3], m, shape[1], shape[2])
        em.update(xd, yd)
        runs.append((em.state()["sums"].clone(), em.state()["ranks"].clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("m", [5, 33])
def test_two_halves_of_the_batch(m):
    shape = (4, 3, 2, 6, 10)
    x, y = _inputs(m, shape, "unit", seed=2)
    xd, yd = x.to(DEV), y.to(DEV)
    whole = _metric(6, m, 3, 2)
    whole.update(xd, yd)
    halves = _metric(6, m, 3, 2)
    halves.update(xd[:, :2], yd[:2])          # a view whose members are not contiguous: goes through one copy
    halves.update(xd[:, 2:], yd[2:])
    _, _, bound = _check(whole, x, y, None, 0, f"M={m} whole batch")
    _check(halves, x, y, None, 0, f"M={m} two halves")
    a, b = whole.state(), halves.state()
    assert torch.equal(a["ranks"], b["ranks"]) and torch.equal(a["count"], b["count"])
    assert (np.abs(a["sums"].cpu().numpy() - b["sums"].cpu().numpy()) <= bound).all()
    fa, fb = whole.finalize(), halves.finalize()
    assert torch.allclose(fa["crps"], fb["crps"], rtol=1e-5)


def test_a_larger_chunk_keeps_the_first_workspace():
    """a recorded step replays against the workspace address it was recorded with, so a chunk that needs a larger workspace
    must leave the first one allocated (and the scores what a fresh scorer gives for the same two chunks)"""
    from dlwp_benchmark_amd import lib as L

    m, c, h, w = 2, 1, 4, 8
    (b1, k1), (b2, k2) = (1, 1), (2, 2)
    need = [int(L.load().dlwp_ensemble_sums_workspace_bytes(b, k, c, h, w)) for b, k in ((b1, k1), (b2, k2))]
    assert 8 <= need[0] < need[1], need
    x1, y1 = (t.to(DEV) for t in _inputs(m, (b1, k1, c, h, w), "unit", seed=5))
    x2, y2 = (t.to(DEV) for t in _inputs(m, (b2, k2, c, h, w), "unit", seed=6))
    em = _metric(h, m, k1 + k2, c)
    em.update(x1, y1, step_begin=0)
    first = em._ws[DEV][-1]
    ptr = first.data_ptr()
    assert first.numel() == need[0]
    em.update(x2, y2, step_begin=k1)
    bufs = em._ws[DEV]
    assert len(bufs) == 2 and bufs[0] is first and first.data_ptr() == ptr
    assert bufs[-1].numel() >= need[1] and bufs[-1].data_ptr() != ptr
    fresh = _metric(h, m, k1 + k2, c)
    fresh.update(x1, y1, step_begin=0).update(x2, y2, step_begin=k1)
    got, want = em.finalize(), fresh.finalize()
    for name, v in want.items():
        assert torch.equal(got[name], v), name
    assert bool(torch.isfinite(got["crps"]).all()) and em.state()["count"].tolist() == [1.0, 2.0, 2.0]


def test_refusals():
    from dlwp_benchmark_amd import lib as L
    from dlwp_benchmark_amd.metrics import EnsembleMetrics

    h, w = 6, 10
    for m in (1, 65):
        with pytest.raises(L.DlwpError) as e:
            EnsembleMetrics(_lats(h), m, 3, 2)
        assert e.value.status == L.ERR_UNSUPPORTED
        # and at the entry point itself
        ens, tar = torch.zeros(m, 1, 1, 1, h, w, device=DEV), torch.zeros(1, 1, 1, h, w, device=DEV)
        sums = torch.zeros(4, 1, 1, dtype=torch.float64, device=DEV)
        ranks = torch.zeros(1, 1, m + 1, dtype=torch.int64, device=DEV)
        ws = torch.zeros(64, dtype=torch.uint8, device=DEV)
        with pytest.raises(L.DlwpError) as e:
            L.launch("dlwp_ensemble_sums_acc_f32", ens.device, ens, tar, torch.ones(h, device=DEV), None, sums, ranks, m, h * w,
                     1, 1, 1, h, w, 1, 0, ws, ws.numel())
        assert e.value.status == L.ERR_UNSUPPORTED
        assert not sums.any() and not ranks.any()
    em = EnsembleMetrics(_lats(h), 4, 3, 2)
    x, y = torch.zeros(4, 2, 3, 2, h, w, device=DEV), torch.zeros(2, 3, 2, h, w, device=DEV)
    with pytest.raises(L.DlwpError, match="no CPU fallback"):
        em.update(x.cpu(), y.cpu())
    with pytest.raises(L.DlwpError, match="no CPU fallback"):
        em.update(x, y.cpu())
    with pytest.raises(L.DlwpError, match="target shape"):
        em.update(x, y[:, :2])
    with pytest.raises(L.DlwpError, match="expected an ensemble"):
        em.update(x[:3], y)
    with pytest.raises(L.DlwpError, match="steps"):
        em.update(x, y, step_begin=1)
    with pytest.raises(L.DlwpError, match="HEALPix"):
        em.update(torch.zeros(4, 1, 3, 2, 12, 4, 4, device=DEV), torch.zeros(1, 3, 2, 12, 4, 4, device=DEV))
    assert em.state()["sums"] is None
    good = {"sums": torch.zeros(4, 3, 2, dtype=torch.float64, device=DEV),
            "ranks": torch.zeros(3, 2, 5, dtype=torch.int64, device=DEV),
            "count": torch.zeros(3, dtype=torch.float64, device=DEV), "width": w}
    with pytest.raises(L.DlwpError, match="sums"):
        em.load_state(dict(good, sums=good["sums"].float()))
    with pytest.raises(L.DlwpError, match="sums"):
        em.load_state(dict(good, sums=torch.zeros(4, 3, 3, dtype=torch.float64, device=DEV)))
    with pytest.raises(L.DlwpError, match="ranks"):
        em.load_state(dict(good, ranks=good["ranks"].cpu()))
    em.load_state(good).update(x, y)
    assert int(em.state()["ranks"].sum()) == 2 * 3 * 2 * h * w
    # a workspace that is too small is refused by the entry point
    with pytest.raises(L.DlwpError) as e:
        L.launch("dlwp_ensemble_sums_acc_f32", x.device, x, y, torch.ones(h, device=DEV), None, good["sums"], good["ranks"], 4,
                 x[0].numel(), 2, 3, 2, h, w, 3, 0, torch.zeros(8, dtype=torch.uint8, device=DEV), 8)
    assert e.value.status == -4      # DLWP_ERR_WORKSPACE


def test_healpix_ensemble_in_chunks():
    """[3, 2, 2, 1, 12, 4, 4] onto an 8 x 16 grid with a workspace that holds one sample (all members and the target) only"""
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd.metrics import EnsembleMetrics

    m, b, k, c, h, w = 3, 2, 2, 1, 8, 16
    g = torch.Generator().manual_seed(8)
    y = torch.randn(b, k, c, 12, 4, 4, generator=g)
    x = y + torch.randn(m, b, k, c, 12, 4, 4, generator=g)
    lats, lons = _lats(h), torch.arange(w) * (360.0 / w)
    per_sample = 4 * (m + 1) * k * c * h * w
    em = EnsembleMetrics(lats, m, k, c, lons_deg=lons, max_workspace_bytes=per_sample + per_sample // 2)
    em.update(x.to(DEV), y.to(DEV))
    xl = ops.healpix_to_latlon(x.to(DEV), em._lats, em._lons).cpu()
    yl = ops.healpix_to_latlon(y.to(DEV), em._lats, em._lons).cpu()
    assert xl.shape == (m, b, k, c, h, w)
    _check(em, xl, yl, None, 0, "HEALPix, two chunks of one sample")
    assert em.state()["count"].tolist() == [2.0, 2.0] and em._remap_ws[DEV].numel() == (m + 1) * k * c * h * w
    from dlwp_benchmark_amd.lib import DlwpError
    with pytest.raises(DlwpError, match="max_workspace_bytes"):
        EnsembleMetrics(lats, m, k, c, lons_deg=lons, max_workspace_bytes=per_sample - 4).update(x.to(DEV), y.to(DEV))
