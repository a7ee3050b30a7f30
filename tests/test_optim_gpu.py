"""The multi-tensor kernels of csrc/optim.hip through dlwp_benchmark_amd/optim.py on the GPU: FusedAdamW, clip_grad_norm_,
zero_grad and ExponentialMovingAverage against torch itself run in float64 on the CPU on the same fp32 inputs
(tests/test_optim_cpu.py builds the cases and the oracles).

Bounds.  AdamW: twice the error of torch's own fp32 CPU AdamW against the float64 run, per quantity (adamw_bound).  Total
norm: 1e-6 relative -- positive terms, at most a chunk's worth of fp32 adds in a tree, the cross-chunk sum in double.  EMA:
2^-22 of the tensor's max magnitude (three steps of two roundings).  Everything else is bitwise.

Measured on MI355X, 5 steps of the standard list: p 5.9e-07 (absolute) against a bound of 1.2e-06, exp_avg 1.6e-07 against
3.9e-07, exp_avg_sq 2.1e-07 against 7.7e-07; total norm 2.7e-08 relative."""
import numpy as np
import pytest
import torch

from dlwp_benchmark_amd import lib as L
from dlwp_benchmark_amd import optim as O
from test_optim_cpu import (FROZEN, LR, MAX_NORM, NO_GRAD, STEPS, VIEW, VIEW_ELEMS, WD, adamw_bound, chunk, make_case, run_errors,
                            torch_run)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class Rig:
    """the tensors of a case on the GPU: the VIEW parameter is base[1:1 + n] of a larger tensor (4-byte aligned only), and so
    is its gradient"""

    def __init__(self, case):
        self.case = case
        self.base = None
        self.params = []
        for p, role in zip(case["params"], case["roles"]):
            if role == VIEW:
                self.base = torch.full((p.numel() + 2,), 7.25, device=DEV)
                q = self.base[1:1 + p.numel()]
                q.copy_(p)
                assert q.data_ptr() % 16 == 4
                self.params.append(q.requires_grad_(True))
            else:
                self.params.append(p.to(DEV).clone().requires_grad_(role != FROZEN))
        self.initial = [p.detach().clone() for p in self.params]

    def set_grads(self, step):
        for p, g, role in zip(self.params, self.case["grads"][step], self.case["roles"]):
            if g is None:
                continue
            if p.grad is None:
                if role == VIEW:
                    self.gbase = torch.full((g.numel() + 2,), -3.5, device=DEV)
                    p.grad = self.gbase[1:1 + g.numel()]
                else:
                    p.grad = torch.empty_like(p)
            p.grad.copy_(g)


def hip_run(case, steps=None, lr=LR, wd=WD, max_norm=MAX_NORM, fused_clip=False, cosine_t_max=None, clip_with_list=False):
    steps = len(case["grads"]) if steps is None else steps
    rig = Rig(case)
    opt = O.FusedAdamW(rig.params, lr=lr, weight_decay=wd)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=cosine_t_max) if cosine_t_max else None
    norms = []
    for s in range(steps):
        rig.set_grads(s)
        if max_norm is not None and fused_clip:
            opt.step(clip_max_norm=max_norm)
            norms.append(opt.last_total_norm)
        else:
            if max_norm is not None:
                norms.append(O.clip_grad_norm_(rig.params if clip_with_list else opt, max_norm))
            opt.step()
        if sched is not None:
            sched.step()
    torch.cuda.synchronize()
    return {"p": [p.detach() for p in rig.params], "exp_avg": [opt.state[p]["exp_avg"] for p in rig.params],
            "exp_avg_sq": [opt.state[p]["exp_avg_sq"] for p in rig.params], "norms": norms, "opt": opt, "rig": rig}


@pytest.fixture(scope="module")
def standard():
    """the standard case, its float64 oracle and bound, and one HIP run: shared and left unchanged"""
    case = make_case()
    bound, want = adamw_bound(case)
    return case, bound, want, hip_run(case)


def assert_within(got, want, bound, label):
    err = run_errors(got, want)
    print(f"{label}: p {err[0]:.2e} (bound {bound[0]:.2e}), exp_avg {err[1]:.2e} ({bound[1]:.2e}), "
          f"exp_avg_sq {err[2]:.2e} ({bound[2]:.2e})")
    for e, b, name in zip(err, bound, ("p", "exp_avg", "exp_avg_sq")):
        assert e <= b, f"{label}: {name} {e:.3e} above {b:.3e}"


def test_adamw_five_steps_match_float64(standard):
    case, bound, want, got = standard
    assert_within(got, want, bound, "AdamW 5 steps")
    for n_got, n_want in zip(got["norms"], want["norms"]):
        assert abs(float(n_got) - float(n_want)) <= 1e-6 * float(n_want)
    rig, opt = got["rig"], got["opt"]
    steps = opt.steps()
    for i, role in enumerate(case["roles"]):
        if role in (NO_GRAD, FROZEN):             # bit-unchanged, state untouched, step 0
            assert torch.equal(rig.params[i], rig.initial[i]) and steps[i] == 0
            assert not got["exp_avg"][i].any() and not got["exp_avg_sq"][i].any()
        else:
            assert steps[i] == STEPS
    # the neighbours of the unaligned view, in the parameter's base and in the gradient's
    assert rig.base[0] == 7.25 and rig.base[-1] == 7.25 and rig.gbase[0] == -3.5 and rig.gbase[-1] == -3.5
    # the arenas beyond the tensors (the padding between states) stay zero
    t = opt.table()
    used = torch.zeros(opt.exp_avg.numel(), dtype=torch.bool, device=DEV)
    for off, n in zip(t.host["state_off"], t.host["numel"]):
        used[off:off + n] = True
    assert not opt.exp_avg[~used].any() and not opt.exp_avg_sq[~used].any()


def test_clip_with_a_parameter_list_is_the_optimizer_table(standard):
    case, _, _, got = standard
    again = hip_run(case, clip_with_list=True)
    assert all(torch.equal(a, b) for a, b in zip(again["p"], got["p"]))
    assert all(torch.equal(a, b) for a, b in zip(again["norms"], got["norms"]))


def test_total_norm_and_clip():
    case = make_case(steps=1)
    rig = Rig(case)
    rig.set_grads(0)
    before = [None if p.grad is None else p.grad.clone() for p in rig.params]
    want = torch.sqrt(sum((g.double() ** 2).sum() for g in case["grads"][0] if g is not None))
    norm = O.clip_grad_norm_(rig.params, MAX_NORM)
    assert norm.is_cuda and norm.dim() == 0 and norm.dtype == torch.float32
    rel = abs(float(norm) - float(want)) / float(want)
    print(f"total norm: relative error {rel:.2e}")
    assert rel <= 1e-6
    coef = torch.tensor(MAX_NORM, dtype=torch.float32) / (norm.cpu() + torch.tensor(1e-6, dtype=torch.float32))
    assert float(coef) < 1
    for p, g0 in zip(rig.params, before):
        if g0 is None:
            assert p.grad is None
            continue
        exp = (g0.cpu() * coef).numpy()
        assert np.all(np.abs(p.grad.cpu().numpy() - exp) <= np.spacing(np.abs(exp)))      # 1 ulp
    # above the norm: the multiply by 1 leaves every bit
    now = [None if p.grad is None else p.grad.clone() for p in rig.params]
    n2 = O.clip_grad_norm_(rig.params, 1e6)
    assert float(n2) < 1e6
    for p, g0 in zip(rig.params, now):
        assert g0 is None or torch.equal(p.grad, g0)
    assert rig.base[0] == 7.25 and rig.base[-1] == 7.25 and rig.gbase[0] == -3.5 and rig.gbase[-1] == -3.5


def test_clip_with_an_inf_gradient_equals_torch():
    case = make_case(steps=1)
    case["grads"][0][4][17] = float("inf")
    rig = Rig(case)
    rig.set_grads(0)
    cpu = [p.clone().requires_grad_(True) for p in case["params"]]
    for p, g in zip(cpu, case["grads"][0]):
        p.grad = None if g is None else g.clone()
    n_want = torch.nn.utils.clip_grad_norm_(cpu, MAX_NORM)
    n_got = O.clip_grad_norm_(rig.params, MAX_NORM)
    assert torch.isinf(n_want) and torch.isinf(n_got.cpu())
    for p, q in zip(rig.params, cpu):
        if q.grad is None:
            continue
        got, want = p.grad.cpu(), q.grad
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.isnan(want).sum() == int(q is cpu[4])
        assert torch.equal(got[~torch.isnan(got)], want[~torch.isnan(want)])


def test_whole_numbers_give_the_exact_sum_of_squares():
    case = make_case(steps=1, integer_grads=True)
    rig = Rig(case)
    rig.set_grads(0)
    exact = sum(int((g.long() ** 2).sum()) for g in case["grads"][0] if g is not None)
    norm = O.clip_grad_norm_(rig.params, 1e9)
    assert float(norm) == float(torch.tensor(exact, dtype=torch.float64).sqrt().float())      # rounded once
    assert round(float(norm.double() ** 2)) == exact


def test_past_the_grid_cap():
    """more chunks than the 2048-workgroup cap of the multi-tensor kernels: a workgroup takes several chunks"""
    sizes = [3_000_001, 2_900_000, 2_600_003]
    assert sum(-(-n // chunk()) for n in sizes) > 2048
    case = make_case(sizes, steps=2, extras=False, seed=5)
    bound, want = adamw_bound(case)
    got = hip_run(case)
    assert_within(got, want, bound, "past the grid cap, 2 steps")
    for n_got, n_want in zip(got["norms"], want["norms"]):
        assert abs(float(n_got) - float(n_want)) <= 1e-6 * float(n_want)


def test_reruns_are_bitwise_identical(standard):
    case, _, _, got = standard
    again = hip_run(case)
    for key in ("p", "exp_avg", "exp_avg_sq", "norms"):
        assert all(torch.equal(a, b) for a, b in zip(again[key], got[key])), key


def test_fused_last_clip_gives_the_same_bits(standard):
    case, _, _, got = standard
    fused = hip_run(case, fused_clip=True)
    for key in ("p", "exp_avg", "exp_avg_sq", "norms"):
        assert all(torch.equal(a, b) for a, b in zip(fused[key], got[key])), key
    # .grad holds the unclipped values
    rig = fused["rig"]
    for p, g in zip(rig.params, case["grads"][-1]):
        assert g is None or torch.equal(p.grad.cpu(), g)


def _torch_gpu_optimizer(case, source_params):
    params = [p.detach().clone().requires_grad_(role != FROZEN) for p, role in zip(source_params, case["roles"])]
    return params, torch.optim.AdamW(params, lr=LR, weight_decay=WD, foreach=False)


def _step_torch(params, opt, grads):
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.to(DEV).clone()
    torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
    opt.step()
    return {"p": params, "exp_avg": [opt.state.get(p, {}).get("exp_avg") for p in params],
            "exp_avg_sq": [opt.state.get(p, {}).get("exp_avg_sq") for p in params]}


def test_checkpoints_interchange_with_torch_adamw():
    case = make_case(steps=3)
    bound, _ = adamw_bound(case)
    # FusedAdamW -> torch.optim.AdamW
    fused = hip_run(case, steps=2)
    sd = fused["opt"].state_dict()
    t_params, t_opt = _torch_gpu_optimizer(case, fused["p"])
    t_opt.load_state_dict(sd)
    rig = fused["rig"]
    rig.set_grads(2)
    O.clip_grad_norm_(fused["opt"], MAX_NORM)
    fused["opt"].step()
    want = _step_torch(t_params, t_opt, case["grads"][2])
    got = {"p": rig.params, "exp_avg": fused["exp_avg"], "exp_avg_sq": fused["exp_avg_sq"]}
    assert_within(got, want, bound, "fused state into torch, one more step")
    # the layout is torch's: keys, shapes, dtypes
    sd_f, sd_t = fused["opt"].state_dict(), t_opt.state_dict()
    assert sorted(sd_f) == sorted(sd_t) and sorted(sd_f["state"]) == sorted(sd_t["state"])
    for k, st in sd_t["state"].items():
        assert sorted(sd_f["state"][k]) == sorted(st)
        for name, v in st.items():
            w = sd_f["state"][k][name]
            assert w.shape == v.shape and w.dtype == v.dtype, (k, name)
        assert float(sd_f["state"][k]["step"]) == float(st["step"]) == 3
    assert [sorted(g) for g in sd_f["param_groups"]] == [sorted(g) for g in sd_t["param_groups"]]
    assert [g["params"] for g in sd_f["param_groups"]] == [g["params"] for g in sd_t["param_groups"]]
    # torch.optim.AdamW -> FusedAdamW
    t_params, t_opt = _torch_gpu_optimizer(case, [p.to(DEV) for p in case["params"]])
    for s in range(2):
        _step_torch(t_params, t_opt, case["grads"][s])
    case2 = dict(case, params=[p.detach().cpu() for p in t_params])
    rig2 = Rig(case2)
    opt2 = O.FusedAdamW(rig2.params, lr=LR, weight_decay=WD)
    opt2.load_state_dict(t_opt.state_dict())
    assert opt2.steps() == [0 if r in (NO_GRAD, FROZEN) else 2 for r in case["roles"]]
    rig2.set_grads(2)
    O.clip_grad_norm_(opt2, MAX_NORM)
    opt2.step()
    want = _step_torch(t_params, t_opt, case["grads"][2])
    got = {"p": rig2.params, "exp_avg": [opt2.state[p]["exp_avg"] for p in rig2.params],
           "exp_avg_sq": [opt2.state[p]["exp_avg_sq"] for p in rig2.params]}
    assert_within(got, want, bound, "torch state into fused, one more step")
    assert rig2.base[0] == 7.25 and rig2.base[-1] == 7.25


def test_cosine_scheduler_reaches_the_device():
    case = make_case(steps=4, seed=2)
    bound, want = adamw_bound(case, cosine_t_max=4)
    got = hip_run(case, cosine_t_max=4)
    assert got["opt"].param_groups[0]["lr"] < 1e-9 * LR + 1e-12          # the schedule ran to its end
    assert_within(got, want, bound, "CosineAnnealingLR, 4 steps")
    stale = run_errors(got, torch_run(case, torch.float64))               # a run whose lr never changed is far away
    assert stale[0] > 100 * bound[0]


def test_parameter_groups_have_their_own_hyperparameters():
    case = make_case(steps=2, seed=3, extras=False)
    half = len(case["params"]) // 2

    def groups(params):
        return [{"params": params[:half], "lr": 3e-3, "weight_decay": 0.0, "betas": (0.8, 0.99)},
                {"params": params[half:], "eps": 1e-6}]

    def run(dtype):
        params = [p.to(dtype).clone().requires_grad_(True) for p in case["params"]]
        opt = torch.optim.AdamW(groups(params), lr=LR, weight_decay=WD, foreach=False)
        for s in range(2):
            for p, g in zip(params, case["grads"][s]):
                p.grad = g.to(dtype).clone()
            opt.step()
        return {"p": params, "exp_avg": [opt.state[p]["exp_avg"] for p in params],
                "exp_avg_sq": [opt.state[p]["exp_avg_sq"] for p in params]}

    want = run(torch.float64)
    bound = tuple(2.0 * e for e in run_errors(run(torch.float32), want))
    rig = Rig(case)
    opt = O.FusedAdamW(groups(rig.params), lr=LR, weight_decay=WD)
    for s in range(2):
        rig.set_grads(s)
        opt.step()
    got = {"p": rig.params, "exp_avg": [opt.state[p]["exp_avg"] for p in rig.params],
           "exp_avg_sq": [opt.state[p]["exp_avg_sq"] for p in rig.params]}
    assert_within(got, want, bound, "two parameter groups, 2 steps")


def test_recorded_step_replays():
    """clip + step captured once on one stream and replayed with new gradients in the same storage: the parameters of three
    eager steps bit for bit, also across a change of lr between replays (the learning rate is read from device memory)"""
    case = make_case(steps=3, seed=4)
    eager, rec = Rig(case), Rig(case)
    opt_e = O.FusedAdamW(eager.params, lr=LR, weight_decay=WD)
    opt_r = O.FusedAdamW(rec.params, lr=LR, weight_decay=WD)
    warm = Rig(make_case(steps=1, seed=9))                 # every kernel has run once before anything is captured
    warm.set_grads(0)
    warm_opt = O.FusedAdamW(warm.params)
    O.clip_grad_norm_(warm_opt, MAX_NORM)
    warm_opt.step()
    rec.set_grads(0)
    opt_r.sync()                                           # pointers and hyper-parameters reach the device before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        norm = O.clip_grad_norm_(opt_r, MAX_NORM)
        opt_r.step()
    assert all(torch.equal(p, q) for p, q in zip(rec.params, rec.initial)), "the capture itself ran the step"
    for s in range(3):
        if s == 2:
            opt_e.param_groups[0]["lr"] = opt_r.param_groups[0]["lr"] = 2.5e-4
            opt_r.sync()
        eager.set_grads(s)
        n_e = O.clip_grad_norm_(opt_e, MAX_NORM)
        opt_e.step()
        rec.set_grads(s)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(n_e, norm), s
        for p, q in zip(eager.params, rec.params):
            assert torch.equal(p, q), s
    assert opt_r.steps() == opt_e.steps()
    changed = Rig(case)                                    # and the lr change mattered
    opt_c = O.FusedAdamW(changed.params, lr=LR, weight_decay=WD)
    for s in range(3):
        changed.set_grads(s)
        O.clip_grad_norm_(opt_c, MAX_NORM)
        opt_c.step()
    assert not torch.equal(changed.params[3], rec.params[3])


def test_ema():
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(67, 129), torch.nn.Linear(129, 2 * chunk() // 129 + 3)).to(DEV)
    model[0].bias.requires_grad_(False)
    decay = 0.995
    ema = O.ExponentialMovingAverage(model, decay)
    ema.register()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    assert sorted(ema.shadow) == sorted(n for n, _ in named) and "0.bias" not in ema.shadow
    want = {n: p.detach().double().cpu() for n, p in named}
    for n, p in named:
        assert torch.equal(ema.shadow[n], p)
    for _ in range(3):
        with torch.no_grad():
            for _, p in named:
                p.add_(0.1 * torch.randn_like(p))
        ema.update()
        for n, p in named:
            want[n] = (1.0 - decay) * p.detach().double().cpu() + decay * want[n]
    for n, _ in named:
        err = float((ema.shadow[n].double().cpu() - want[n]).abs().max()) / float(want[n].abs().max())
        assert err <= 2.0 ** -22, (n, err)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    ema.apply_shadow()
    for n, p in named:
        assert torch.equal(p, ema.shadow[n]) and not torch.equal(p, before[n])
    ema.restore()
    for n, p in model.named_parameters():
        assert torch.equal(p, before[n]), n


def test_zero_grad_keeps_the_storage():
    case = make_case(steps=1)
    rig = Rig(case)
    rig.set_grads(0)
    opt = O.FusedAdamW(rig.params)
    ptrs = [None if p.grad is None else p.grad.data_ptr() for p in rig.params]
    opt.zero_grad()
    for p, ptr in zip(rig.params, ptrs):
        if ptr is None:
            assert p.grad is None
        else:
            assert p.grad.data_ptr() == ptr and p.grad.numel() == p.numel() and not p.grad.any()
    assert rig.gbase[0] == -3.5 and rig.gbase[-1] == -3.5 and rig.gbase.numel() == VIEW_ELEMS + 2
    opt.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in rig.params)


def test_refusals_on_the_device():
    with pytest.raises(L.DlwpError, match="float32"):
        O.FusedAdamW([torch.zeros(8, device=DEV, dtype=torch.bfloat16, requires_grad=True)])
    with pytest.raises(L.DlwpError, match="contiguous"):
        O.FusedAdamW([torch.zeros(8, 8, device=DEV).t()[1:].requires_grad_(True)])


def test_complex64_parameters_are_their_float_pairs():
    """the FNO's spectral weights: torch.optim.AdamW steps a complex parameter through view_as_real, and the 2-norm and the EMA
    are those of the pairs as well"""
    g = torch.Generator().manual_seed(11)
    shapes = [((6, 5, 12, 7), torch.complex64), ((chunk() // 2 + 3,), torch.complex64), ((33,), torch.float32)]
    p0 = [torch.randn(s, generator=g, dtype=d) for s, d in shapes]
    grads = [[torch.randn(s, generator=g, dtype=d) * 1e-2 for s, d in shapes] for _ in range(3)]
    wide = {torch.complex64: torch.complex128, torch.float32: torch.float64}

    def run(widen):
        params = [p.to(wide[p.dtype] if widen else p.dtype).clone().requires_grad_(True) for p in p0]
        opt = torch.optim.AdamW(params, lr=LR, weight_decay=WD, foreach=False)
        norms = []
        for row in grads:
            for p, gr in zip(params, row):
                p.grad = gr.to(p.dtype).clone()
            norms.append(torch.nn.utils.clip_grad_norm_(params, MAX_NORM))
            opt.step()
        real = lambda t: torch.view_as_real(t) if t.is_complex() else t
        return {"p": [real(p.detach()) for p in params], "exp_avg": [real(opt.state[p]["exp_avg"]) for p in params],
                "exp_avg_sq": [real(opt.state[p]["exp_avg_sq"]) for p in params], "norms": norms}

    want = run(True)
    bound = tuple(2.0 * e for e in run_errors(run(False), want))
    params = [p.to(DEV).clone().requires_grad_(True) for p in p0]
    opt = O.FusedAdamW(params, lr=LR, weight_decay=WD)
    norms = []
    for row in grads:
        for p, gr in zip(params, row):
            p.grad = gr.to(DEV)
        norms.append(O.clip_grad_norm_(opt, MAX_NORM))
        opt.step()
    real = lambda t: torch.view_as_real(t) if t.is_complex() else t
    assert opt.state[params[0]]["exp_avg"].dtype == torch.complex64 and opt.state[params[0]]["exp_avg"].shape == params[0].shape
    got = {"p": [real(p.detach()) for p in params], "exp_avg": [real(opt.state[p]["exp_avg"]) for p in params],
           "exp_avg_sq": [real(opt.state[p]["exp_avg_sq"]) for p in params]}
    assert_within(got, want, bound, "complex64 parameters, 3 steps")
    for a, b in zip(norms, want["norms"]):
        assert abs(float(a) - float(b)) <= 1e-6 * float(b)
    sd = opt.state_dict()
    assert sd["state"][0]["exp_avg"].dtype == torch.complex64 and float(sd["state"][0]["step"]) == 3
