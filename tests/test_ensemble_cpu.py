"""Ensembles without a GPU: the member streams' definition, identities of the score restatement (tests/ensemble_ref.py),
metrics.EnsembleMetrics.finalize on hand-made sums (and across two gloo ranks), the scheduler's member bookkeeping, the new
entry points' declarations and the drivers' shape arithmetic."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ensemble_ref
import philox_ref
from dlwp_benchmark_amd import lib as L
from dlwp_benchmark_amd import schedulers as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dlwp_philox_normal_members_f32", "dlwp_ddpm_step_members_f32", "dlwp_ensemble_sums_acc_f32",
               "dlwp_ensemble_sums_workspace_bytes")


# ---- the member streams ---------------------------------------------------------------------------------------------------
def test_member_zero_is_the_plain_stream():
    for seed, offset, n in [(2024, 0, 4099), ((1 << 63) + 12345, (1 << 34) + 8, 257), (7, 4096, 5)]:
        assert np.array_equal(ensemble_ref.member_normals(seed, 0, offset, n), philox_ref.normals(seed, offset, n))


def test_members_differ():
    plain = philox_ref.normals(2024, 0, 256)
    one, last = ensemble_ref.member_normals(2024, 1, 0, 256), ensemble_ref.member_normals(2024, 2 ** 31 - 1, 0, 256)
    assert not np.array_equal(one, plain) and not np.array_equal(last, plain) and not np.array_equal(one, last)
    # no element in common either: the member reaches every word of the block
    assert not (one == plain).any() and not (last == plain).any() and not (one == last).any()
    # the member sits in counter word 2: the known-answer vector with that word set goes through the same function
    counter, key, want = philox_ref.KNOWN_ANSWERS[2]
    got = philox_ref.philox4x32_10(counter, key)
    assert tuple(int(g[0]) for g in got) == want


def test_member_stream_moments():
    z = ensemble_ref.member_normals(2024, 3, 0, 1 << 18)
    n = z.size
    assert abs(z.mean()) <= 5 / math.sqrt(n) and abs((z ** 2).mean() - 1) <= 5 * math.sqrt(2 / n)


# ---- the score restatement ------------------------------------------------------------------------------------------------
def _case(m, seed=0, shape=(2, 3, 2, 6, 10)):
    g = np.random.default_rng(seed)
    y = g.standard_normal(shape)
    x = y + g.standard_normal((m,) + shape)
    return x, y


@pytest.mark.parametrize("m", [2, 3, 5, 16])
def test_sorted_form_equals_pairwise_form(m):
    x, _ = _case(m, seed=m)
    pairs = np.zeros(x.shape[1:])
    for i in range(m):
        for j in range(i + 1, m):
            pairs += np.abs(x[i] - x[j])
    assert np.allclose(ensemble_ref.sorted_pairs(x), pairs, rtol=1e-12, atol=1e-12)


def test_fair_crps_of_two_members():
    x, y = _case(2, seed=5)
    lats = np.linspace(-75, 75, 6)
    w = ensemble_ref.latitude_weights(lats)
    sums, ranks = ensemble_ref.sums_and_ranks(x, y, w)
    sc = ensemble_ref.scores(sums, ranks, np.full(3, 2.0), 2, 60)
    want = (np.abs(x[0] - y) + np.abs(x[1] - y)) / 2 - np.abs(x[0] - x[1]) / 2
    want = (w.reshape(1, 1, 1, 6, 1) * want).sum(axis=(0, 3, 4)) / (2 * 60)
    assert np.allclose(sc["crps"], want, rtol=1e-12, atol=1e-14)


def test_rank_counts_and_the_strict_convention():
    x, y = _case(5, seed=9)
    y[0, 0, 0, 0, 0] = x[2, 0, 0, 0, 0, 0]                         # the target is a copy of a member
    x[4, 1, 1, 1, 1, 1] = x[0, 1, 1, 1, 1, 1]                      # two equal members
    _, ranks = ensemble_ref.sums_and_ranks(x, y, np.ones(6))
    assert ranks.shape == (3, 2, 6) and (ranks.sum(axis=-1) == 2 * 6 * 10).all()
    # a constructed tie: members {0, 1, 1, 2} against y = 1 -- one member strictly below, so rank 1 (not 3)
    xs = np.array([0.0, 1.0, 1.0, 2.0]).reshape(4, 1, 1, 1, 1, 1)
    _, r = ensemble_ref.sums_and_ranks(xs, np.ones((1, 1, 1, 1, 1)), np.ones(1))
    assert r.reshape(-1).tolist() == [0, 1, 0, 0, 0]


# ---- EnsembleMetrics.finalize on CPU tensors ------------------------------------------------------------------------------
def _hand_state(m=4, k=2, c=3, seed=3, samples=(5.0, 2.0)):
    g = torch.Generator().manual_seed(seed)
    sums = torch.rand(4, k, c, generator=g, dtype=torch.float64) * 100 + 1
    ranks = torch.randint(0, 50, (k, c, m + 1), generator=g)
    return {"sums": sums, "ranks": ranks, "count": torch.tensor(samples, dtype=torch.float64), "width": 16}


def test_finalize_on_cpu_sums():
    from dlwp_benchmark_amd.metrics import EnsembleMetrics

    m, k, c, h, w = 4, 2, 3, 8, 16
    st = _hand_state(m, k, c)
    em = EnsembleMetrics(torch.linspace(-78.75, 78.75, h), m, k, c).load_state(st)
    got = em.finalize()
    s, n = st["sums"], (st["count"] * h * w).view(k, 1)
    assert torch.allclose(got["rmse_mean"], (s[0] / n).sqrt(), rtol=1e-14)
    assert torch.allclose(got["spread"], (s[1] / n).sqrt(), rtol=1e-14)
    assert torch.allclose(got["spread_skill"], math.sqrt(5 / 4) * (s[1] / s[0]).sqrt(), rtol=1e-13)
    assert torch.allclose(got["crps"], (s[2] - s[3] / 12) / n, rtol=1e-14)
    assert torch.allclose(got["crps_ens"], (s[2] - s[3] / 16) / n, rtol=1e-14)
    assert got["rank_histogram"].dtype == torch.int64 and torch.equal(got["rank_histogram"], st["ranks"])
    want = ensemble_ref.scores(s.numpy(), st["ranks"].numpy(), st["count"].numpy(), m, h * w)
    for name in ("rmse_mean", "spread", "spread_skill", "crps", "crps_ens"):
        assert np.allclose(got[name].numpy(), want[name], rtol=1e-13), name
    assert em.state()["sums"] is st["sums"]
    with pytest.raises(L.DlwpError, match="finalize"):
        em.reset().finalize()


def test_state_and_construction_refusals():
    from dlwp_benchmark_amd.metrics import EnsembleMetrics

    lats = torch.linspace(-78.75, 78.75, 8)
    for m in (1, 65):
        with pytest.raises(L.DlwpError, match="members") as e:
            EnsembleMetrics(lats, m, 2, 3)
        assert e.value.status == L.ERR_UNSUPPORTED
    em = EnsembleMetrics(lats, 4, 2, 3)
    st = _hand_state()
    with pytest.raises(L.DlwpError, match="sums"):
        em.load_state(dict(st, sums=st["sums"].float()))
    with pytest.raises(L.DlwpError, match="sums"):
        em.load_state(dict(st, sums=st["sums"][:, :1]))
    with pytest.raises(L.DlwpError, match="ranks"):
        em.load_state(dict(st, ranks=st["ranks"].int()))
    with pytest.raises(L.DlwpError, match="count"):
        em.load_state(dict(st, count=st["count"][:1]))
    x = torch.zeros(4, 1, 2, 3, 8, 16)
    with pytest.raises(L.DlwpError, match="no CPU fallback"):
        em.update(x, x[0])


def _finalize_worker(rank, world, port, ret):
    from dlwp_benchmark_amd.metrics import EnsembleMetrics

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        st = _hand_state(seed=3 + rank, samples=(5.0, 2.0) if rank == 0 else (3.0, 3.0))      # unequal shards
        em = EnsembleMetrics(torch.linspace(-78.75, 78.75, 8), 4, 2, 3).load_state(st)
        ret[rank] = em.finalize(world_size=world)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_two_rank_finalize_is_one_sum_of_the_states():
    from dlwp_benchmark_amd.metrics import EnsembleMetrics

    world = 2
    ret = mp.Manager().dict()
    port = 33500 + (os.getpid() % 2000)
    mp.spawn(_finalize_worker, args=(world, port, ret), nprocs=world, join=True)
    a, b = _hand_state(seed=3, samples=(5.0, 2.0)), _hand_state(seed=4, samples=(3.0, 3.0))
    whole = {"sums": a["sums"] + b["sums"], "ranks": a["ranks"] + b["ranks"], "count": a["count"] + b["count"], "width": 16}
    single = EnsembleMetrics(torch.linspace(-78.75, 78.75, 8), 4, 2, 3).load_state(whole).finalize()
    for r in range(world):
        for name, want in single.items():
            if name == "rank_histogram":
                assert ret[r][name].dtype == torch.int64 and torch.equal(ret[r][name], want)
            else:
                assert torch.allclose(ret[r][name], want, rtol=1e-13, atol=0), (r, name)


# ---- the scheduler's member bookkeeping -----------------------------------------------------------------------------------
def _fakes(monkeypatch):
    calls = []

    def fake_normal(shape, seed, offset, device=None):
        calls.append(("normal", seed, offset))
        return torch.zeros(shape)

    def fake_members(shape, seed, members, first_member=0, offset=0, device=None):
        calls.append(("members", seed, members, first_member, offset))
        return torch.zeros(shape)

    def fake_step(sample, model_output, coef, noise=None, seed=0, offset=0, out=None, **kw):
        calls.append(("step", seed, offset, kw))
        return torch.zeros_like(sample)

    monkeypatch.setattr(S._ops, "philox_normal", fake_normal)
    monkeypatch.setattr(S._ops, "philox_normal_members", fake_members)
    monkeypatch.setattr(S._ops, "ddpm_step", fake_step)
    monkeypatch.setattr(L, "require_cuda_tensor", lambda t, name: None)
    return calls


def test_default_members_leave_the_bookkeeping_alone(monkeypatch):
    calls = _fakes(monkeypatch)
    s = S.RefinerScheduler(trained_betas=[0.4, 0.2, 0.1], seed=11)
    s.set_timesteps(2)
    assert (s.members, s.first_member) == (1, 0)
    assert s.set_members(1, 0) is s
    x = torch.zeros(3, 1, 3, 5, 7)                      # 315 elements: 316 per draw
    s.randn(x.shape, "cpu")
    assert s.offset == 316
    s.step(x, 1, x)
    assert s.offset == 632
    s.step(x, 0, x)
    assert s.offset == 632
    assert calls == [("normal", 11, 0), ("step", 11, 316, {}), ("step", 11, 0, {})]      # today's calls, no member keyword
    with pytest.raises(AttributeError):
        s.members = 2


def test_member_mode_advances_by_one_member(monkeypatch):
    calls = _fakes(monkeypatch)
    s = S.RefinerScheduler(trained_betas=[0.4, 0.2, 0.1], seed=11)
    s.set_timesteps(2)
    s.set_members(3)
    assert (s.members, s.first_member) == (3, 0)
    x = torch.zeros(3, 1, 3, 5, 7)                      # 105 elements per member: 108 per draw
    s.randn(x.shape, "cpu")
    assert s.offset == 108
    s.step(x, 1, x)
    assert s.offset == 216
    s.step(x, 0, x)                                     # t = 0: no advance
    assert s.offset == 216
    s.step(x, 1, x, noise=x)                            # explicit noise: no advance
    assert s.offset == 216
    s.set_members(1, 5)                                 # one member that is not member 0 is member mode too
    s.randn((2, 5), "cpu")
    assert s.offset == 228
    member_kw = {"members": 3, "first_member": 0}
    assert calls == [("members", 11, 3, 0, 0), ("step", 11, 108, member_kw), ("step", 11, 0, member_kw),
                     ("step", 11, 0, member_kw), ("members", 11, 1, 5, 216)]
    # the single-member run of the per-member shape uses the same offsets
    t = S.RefinerScheduler(trained_betas=[0.4, 0.2, 0.1], seed=11)
    t.set_timesteps(2)
    t.randn((1, 1, 3, 5, 7), "cpu")
    t.step(x[:1], 1, x[:1])
    assert t.offset == 216


def test_member_mode_refusals(monkeypatch):
    _fakes(monkeypatch)
    s = S.RefinerScheduler(trained_betas=[0.4, 0.2, 0.1]).set_members(3)
    at = s.offset
    with pytest.raises(L.DlwpError, match="divisible"):
        s.randn((4, 2), "cpu")
    with pytest.raises(L.DlwpError, match="divisible"):
        s.step(torch.zeros(4, 2), 1, torch.zeros(4, 2))
    assert s.offset == at                               # a refused draw takes nothing
    for count, first in [(0, 0), (1, -1), (2, 2 ** 31 - 1)]:
        with pytest.raises(L.DlwpError, match="set_members"):
            s.set_members(count, first)
    s.set_members(1, 2 ** 31 - 1)
    h = S.RefinerScheduler(trained_betas=[0.4, 0.2, 0.1], noise="host")
    h.set_members(1, 0)
    with pytest.raises(L.DlwpError, match="host"):
        h.set_members(2)
    with pytest.raises(L.DlwpError, match="host"):
        h.set_members(1, 1)


# ---- symbols and shapes ---------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_mirrored_and_exported():
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "dlwp_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/dlwp_hip.h"
        assert name in L.SIGNATURES and hasattr(lib, name), name
        if name.endswith("_f32"):
            assert L.SIGNATURES[name][1][-1] is L.c_void_p, f"{name}: the stream comes last"
    block = code[code.index("dlwp_refiner_grid_span"):]
    assert "dlwp_philox_normal_members_f32" in block and "dlwp_ddpm_step_members_f32" in block      # the scheduler block
    assert lib.dlwp_ensemble_sums_workspace_bytes(2, 3, 2, 6, 10) == 8 * 4 * 3 * 2 * 2
    assert lib.dlwp_ensemble_sums_workspace_bytes(2, 3, 2, 0, 10) == 0


def test_member_major_repeat_and_view():
    from dlwp_benchmark_amd.rollout import _repeat_members

    x = torch.arange(2 * 3 * 4, dtype=torch.float32).view(2, 3, 4)
    r = _repeat_members(x, 3)
    assert r.shape == (6, 3, 4) and r.is_contiguous()
    v = r.view(3, 2, 3, 4)
    for m in range(3):
        assert torch.equal(v[m], x) and torch.equal(r[2 * m:2 * m + 2], x)
    assert _repeat_members(x, 1) is x and _repeat_members(None, 3) is None


def test_drivers_refuse_without_a_gpu():
    from dlwp_benchmark_amd import models as M
    from dlwp_benchmark_amd.rollout import ensemble_chunks, ensemble_forecast

    x = torch.zeros(1, 2, 2, 8, 16)
    diff = M.DiffModernUNet(constant_channels=0, prescribed_channels=0, prognostic_channels=2, hidden_channels=[8, 16],
                            context_size=1, norm=False, use_scale_shift_norm=False)
    s = S.RefinerScheduler(trained_betas=[0.4, 0.2, 0.1])
    with pytest.raises(L.DlwpError, match="members"):
        ensemble_forecast(diff, s, None, None, x, 0)
    with pytest.raises(L.DlwpError, match="set_members"):
        ensemble_chunks(diff, object(), None, None, x[:, :1], 2, 1, 2)
    with pytest.raises(L.DlwpError, match="no CPU fallback"):
        ensemble_forecast(diff, s, None, None, x, 2)
    assert (s.members, s.first_member) == (1, 0)
