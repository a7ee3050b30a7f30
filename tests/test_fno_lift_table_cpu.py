"""Table of the one-input-channel lifting MLP, host side: the builder the plans use
(dlwp_fno2d_lift_table_build) and the host evaluation with the device's arithmetic (dlwp_fno2d_lift_table_eval_host) against
the fp64 function, with the filler weights of the headline model, biases as filled and zeroed.  Bound everywhere: per-point
relative vector error <= 2^-22, the operand precision of the f16x3 form (measured: <= 8.7e-8)."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import fno_std_fn

R, LOG2 = 32, 4
N_SIDE = R << LOG2
BOUND = 2.0 ** -22
NS_KW = dict(n_modes=[12, 12], constant_channels=0, prescribed_channels=0, prognostic_channels=1,
             hidden_channels=32, lifting_channels=256, projection_channels=256, n_layers=4, context_size=1)


@functools.lru_cache(maxsize=None)
def _filler():
    from dlwp_benchmark_amd.weights import fill_state_dict
    from oracle.restate.fno import FNO2DModuleRef

    ref = FNO2DModuleRef(**NS_KW).eval()
    fill_state_dict(ref, std_fn=fno_std_fn(0.85), gain=0.85)
    sd = ref.state_dict()
    return (sd["fno.lifting.fcs.0.weight"].reshape(256).float().contiguous(), sd["fno.lifting.fcs.0.bias"].float().contiguous(),
            sd["fno.lifting.fcs.1.weight"].reshape(32, 256).float().contiguous(), sd["fno.lifting.fcs.1.bias"].float().contiguous())


def _weights(zero_bias, w1_scale=1.0):
    w1, b1, w2, b2 = _filler()
    if zero_bias:
        b1, b2 = torch.zeros_like(b1), torch.zeros_like(b2)
    return (w1 * w1_scale).contiguous(), b1, w2, b2


def _build(weights):
    from dlwp_benchmark_amd import lib as L

    lib = L.load()
    w1, b1, w2, b2 = weights
    tab = np.zeros((2 * N_SIDE, 6, 32), dtype=np.float32)
    err, ok = ctypes.c_double(-1.0), ctypes.c_int32(-1)
    L.check(lib.dlwp_fno2d_lift_table_build(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), w1.numel(), R, LOG2,
                                            tab.ctypes.data, tab.size, ctypes.byref(err), ctypes.byref(ok)),
            "dlwp_fno2d_lift_table_build")
    return tab, err.value, ok.value


@functools.lru_cache(maxsize=None)
def _table(zero_bias):
    return _build(_weights(zero_bias))


def _eval(tab, x):
    from dlwp_benchmark_amd import lib as L

    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty((x.size, 32), dtype=np.float32)
    v = np.empty(x.size, dtype=np.float32)
    idx = np.empty(x.size, dtype=np.int32)
    L.check(L.load().dlwp_fno2d_lift_table_eval_host(tab.ctypes.data, R, LOG2, x.ctypes.data, x.size, out.ctypes.data,
                                                     v.ctypes.data, idx.ctypes.data), "dlwp_fno2d_lift_table_eval_host")
    return out, v, idx


def _lift64(weights, x):
    w1, b1, w2, b2 = (t.double() for t in weights)
    x = torch.from_numpy(np.asarray(x, dtype=np.float32)).double()
    return (F.gelu(x[:, None] * w1 + b1) @ w2.T + b2).numpy()


def _worst(got, want):
    return float((np.linalg.norm(got.astype(np.float64) - want, axis=1) / np.linalg.norm(want, axis=1)).max())


@pytest.mark.parametrize("zero_bias", [False, True])
def test_table_matches_fp64_function_at_every_magnitude(zero_bias):
    tab, err, ok = _table(zero_bias)
    print(f"zero_bias {zero_bias}: guard figure {err:.3e}")
    assert ok == 1 and err <= BOUND
    rng = np.random.default_rng(7)
    for mag in (1.0, 0.1, 1e-2, 1e-3, 1e-4, 1e-6):
        x = (1.5 * mag * rng.standard_normal(20000)).astype(np.float32)
        x = np.concatenate([x, -x])                       # both signs of every magnitude
        x = x[np.abs(x) < R]
        got, _, idx = _eval(tab, x)
        assert (idx >= 0).all()
        e = _worst(got, _lift64(_weights(zero_bias), x))
        print(f"  |x| ~ 1.5 * {mag:g}: worst per-point relative vector error {e:.3e}")
        assert e <= BOUND, (mag, e)


@pytest.mark.parametrize("zero_bias", [False, True])
def test_knots_zeros_and_domain_ends(zero_bias):
    tab, _, _ = _table(zero_bias)
    w = _weights(zero_bias)
    k = np.arange(-N_SIDE + 1, N_SIDE)
    knots = (k / 2.0 ** LOG2).astype(np.float32)
    got, v, idx = _eval(tab, knots)
    assert (v == 0.0).all()                               # a knot is its interval's end nearer zero: p = c0 = fl32(lift(knot))
    assert (idx == np.where(k >= 0, N_SIDE + k, N_SIDE + k - 1)).all()
    want = _lift64(w, knots).astype(np.float32)            # (one fp32 ulp: two fp64 evaluations may round apart)
    assert (np.abs(got - want) <= np.spacing(np.abs(want))).all()
    got, v, idx = _eval(tab, np.array([0.0, -0.0], dtype=np.float32))
    assert (v == 0.0).all() and (idx == N_SIDE).all() and np.array_equal(got[0], got[1])
    if zero_bias:
        assert (got == 0.0).all()
    edge = np.nextafter(np.float32(R), np.float32(0))
    x = np.array([edge, -edge], dtype=np.float32)
    got, v, idx = _eval(tab, x)
    assert list(idx) == [2 * N_SIDE - 1, 0] and (v < 1.0).all() and (v > 0.99).all()
    assert _worst(got, _lift64(w, x)) <= BOUND
    got, v, idx = _eval(tab, np.array([R, -R, np.inf, -np.inf, np.nan, 1e30], dtype=np.float32))
    assert (idx == -1).all() and np.isnan(got).all()      # outside the domain: the kernel evaluates the MLP instead


def test_coordinate_is_exact():
    tab, _, _ = _table(False)
    rng = np.random.default_rng(11)
    x = np.concatenate([(1.5 * m * rng.standard_normal(5000)).astype(np.float32) for m in (10.0, 1.0, 1e-2, 1e-4, 1e-6, 1e-30)])
    x = x[np.abs(x) < R]
    _, v, idx = _eval(tab, x)
    u = np.abs(x.astype(np.float64)) * 2.0 ** LOG2
    fl = np.floor(u)
    assert np.array_equal(v.astype(np.float64), u - fl)   # fp32 result == the fp64 arithmetic on the same fp32 x
    assert np.array_equal(idx, np.where(x < 0, N_SIDE - 1 - fl, N_SIDE + fl).astype(np.int32))
    assert (v >= 0).all() and (v < 1).all()


@pytest.mark.parametrize("zero_bias", [False, True])
def test_guard_rejects_weights_the_table_cannot_resolve(zero_bias):
    """|w1| scaled up until one interval of the table spans several units of the GELU's argument: the guard must say so."""
    rejected = None
    for k in range(0, 13):
        _, err, ok = _build(_weights(zero_bias, 2.0 ** k))
        print(f"w1 x 2^{k}: guard figure {err:.3e} accepted {ok}")
        assert ok == (1 if err <= BOUND else 0)
        if not ok:
            rejected = k
            break
    assert rejected is not None and rejected >= 1
    w1, b1, w2, b2 = _weights(zero_bias)
    w1 = w1.clone()
    w1[3] = float("nan")
    _, err, ok = _build((w1, b1, w2, b2))
    assert ok == 0 and np.isnan(err)
