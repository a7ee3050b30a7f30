"""The derivation rule of dlwp_benchmark_amd/derived.py on CPU tensors: when a cached value is re-derived (source_key,
Derived) and how long a tensor's holders live (derived_for)."""
import gc
import weakref

import torch

from dlwp_benchmark_amd import derived
from dlwp_benchmark_amd.derived import Derived, bump_pack_epoch, derived_for, live_holders, source_key


class _Counter:
    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return object()


def test_rebuilds_exactly_when_the_key_changes():
    w, b = torch.ones(4), torch.ones(2)
    d, build = Derived(), _Counter()
    first = d.get(source_key(w, None, extra=(False,)), build)
    assert d.get(source_key(w, None, extra=(False,)), build) is first and build.calls == 1
    w.mul_(2)                                                                   # an in-place write
    second = d.get(source_key(w, None, extra=(False,)), build)
    assert second is not first and build.calls == 2
    bump_pack_epoch()                                                           # invalidate_packed()
    assert d.get(source_key(w, None, extra=(False,)), build) is not second and build.calls == 3
    d.get(source_key(w, None, extra=(True,)), build)                            # another `extra`
    assert build.calls == 4
    d.get(source_key(w, b, extra=(True,)), build)                               # a None source becomes a tensor
    assert build.calls == 5
    assert d.get(source_key(w, b, extra=(True,)), build) is d.get(source_key(w, b, extra=(True,)), build) and build.calls == 5


def test_a_failed_build_is_not_cached():
    w, d = torch.ones(4), Derived()

    def fail():
        raise ValueError("no")

    for _ in range(2):
        try:
            d.get(source_key(w), fail)
        except ValueError:
            continue
        raise AssertionError("the build did not run again")


def test_holders_live_and_die_with_their_tensor():
    w, v = torch.ones(4), torch.ones(4)
    gc.collect()                    # (garbage of earlier tests would take its holders along at a moment of its own)
    n = live_holders()
    a, b = derived_for(w, "a"), derived_for(w, ("b", True))
    assert derived_for(w, "a") is a and derived_for(w, ("b", True)) is b and a is not b
    assert derived_for(w, ("b", False)) is not b and derived_for(v, "a") is not a
    made = derived_for(w, "made", make=lambda: Derived(eager_only="x"))         # the factory runs on first use only
    assert derived_for(w, "made", make=dict) is made
    assert live_holders() == n + 5
    del w
    assert live_holders() == n + 1                                              # w's four slots, not v's
    del v
    assert live_holders() == n


def test_a_reused_id_gets_a_fresh_holder():
    w, dead = torch.ones(4), torch.ones(1)
    stale_ref, stale = weakref.ref(dead), Derived()
    del dead
    k = (id(w), "slot")
    derived._HOLDERS[k] = (stale_ref, stale)                                    # what a freed tensor of the same id left
    fresh = derived_for(w, "slot")
    assert fresh is not stale and derived_for(w, "slot") is fresh
    derived._drop(k, stale_ref)                                                 # the dead tensor's finalizer, running late
    assert derived_for(w, "slot") is fresh
    gc.collect()
    n = live_holders()
    del w
    assert live_holders() == n - 1


def test_many_live_holders_evict_none():
    first_bias = torch.zeros(8)
    first = derived_for(first_bias, "bias_bf16").get(source_key(first_bias), object)
    more = [torch.zeros(8) for _ in range(300)]
    values = [derived_for(t, "bias_bf16").get(source_key(t), object) for t in more]
    assert live_holders() >= 301
    assert derived_for(first_bias, "bias_bf16").get(source_key(first_bias), object) is first
    assert all(derived_for(t, "bias_bf16").get(source_key(t), object) is v for t, v in zip(more, values))
