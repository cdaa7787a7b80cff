"""The bounds of bn_ref.py checked without a GPU: an fp32 emulation of the three BatchNorm
backward kernels (the kernels' summation order, casts and fmas) lies inside every bound at
every element and channel, and each deliberately broken variant of it lies outside one.  This
is what keeps test_bn_conformance_gpu.py honest: its bounds are neither so tight that a correct
fp32 evaluation misses them nor so wide that a dropped mean-correction term, a missing row or a
wrong divisor passes."""
import pytest
import torch

import bn_ref as R
from dfu_hip import _lib as L

_CASES = {}


def case(M, C):
    """Inputs, givens and the fp64 reference of one shape, computed once."""
    if (M, C) not in _CASES:
        d = R.inputs(M, C)
        y64 = d["y"].double()
        mu = y64.mean(0)
        var = ((y64 - mu) ** 2).mean(0)
        d["mean"] = mu.float()
        d["invstd"] = (var + R.f32(1e-5)).rsqrt().float()
        scale = d["gamma"] * d["invstd"]
        shift = d["beta"] - d["mean"] * scale
        d["keep"] = d["y"].float() * scale + shift > 0  # a ReLU mask correlated with y
        d["ref"] = R.bwd_ref(d["dout"], d["y"], d["keep"], d["mean"], d["invstd"], d["gamma"],
                             True, d["dgamma0"], d["dbeta0"])
        _CASES[(M, C)] = d
    return _CASES[(M, C)]


def emulate(d, mutation=None):
    dy, dres, dg, db = R.emulate_bwd(d["dout"], d["y"], d["keep"], d["mean"], d["invstd"],
                                     d["gamma"], True, d["dgamma0"], d["dbeta0"], mutation)
    ref = d["ref"]
    assert torch.equal(dres.double(), ref["dres"])
    return {q: R.worst(got, ref[q]) for q, got in (("dy", dy), ("dgamma", dg), ("dbeta", db))}


@pytest.mark.parametrize("M,C", [(300, 64), (2053, 128), (16533, 64)])
def test_emulation_inside_every_bound(M, C):
    """No element and no channel excluded; (2053, 128) is the big-mean case."""
    res = emulate(case(M, C))
    print(f"bn emulation ({M}, {C}): worst err/bound " +
          ", ".join(f"{q} {r:.3f}" for q, (r, _) in res.items()))
    for q, (ratio, n_bad) in res.items():
        assert n_bad == 0, f"{q}: {n_bad} outside the bound, worst err/bound {ratio:.3f}"


def test_emulation_inside_every_bound_eval_mode():
    """batch_stats = 0: m1 = m2 = 0, the bound collapses to one bf16 rounding of k g."""
    d = case(300, 64)
    ref = R.bwd_ref(d["dout"], d["y"], None, d["mean"], d["invstd"], None, False)
    dy, _, dg, db = R.emulate_bwd(d["dout"], d["y"], None, d["mean"], d["invstd"], None, False)
    for q, got in (("dy", dy), ("dgamma", dg), ("dbeta", db)):
        R.check(got, ref[q], f"eval {q}")


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_is_rejected_small(mutation):
    res = emulate(case(300, 64), mutation)
    print(f"bn emulation (300, 64) {mutation}: " +
          ", ".join(f"{q} {n} bad, worst {r:.3g}" for q, (r, n) in res.items()))
    assert any(n_bad for _, n_bad in res.values()), f"{mutation} passes every bound"


@pytest.mark.parametrize("mutation", ["drop_m1", "drop_row", "reduce_ignores_mask"])
def test_row_mask_and_m1_mutations_are_rejected_large(mutation):
    """At M = 16533 (130 row-blocks, a 21-row last block) too.  A division by M - 1 changes
    m1 and m2 by 1 / 16532 of themselves there, below one bf16 rounding of almost every dy: it is
    expected to hide at this size (M = 300 is where it shows), so it is printed, not asserted."""
    d = case(16533, 64)
    res = emulate(d, mutation)
    print(f"bn emulation (16533, 64) {mutation}: " +
          ", ".join(f"{q} {n} bad, worst {r:.3g}" for q, (r, n) in res.items()))
    assert any(n_bad for _, n_bad in res.values()), f"{mutation} passes every bound"
    if mutation == "drop_m1":
        hid = emulate(d, "div_m_minus_1")
        print("bn emulation (16533, 64) div_m_minus_1 (not asserted): " +
              ", ".join(f"{q} {n} bad, worst {r:.3g}" for q, (r, n) in hid.items()))


def test_a_nan_or_inf_output_is_outside_every_bound():
    """An unwritten or poisoned output must not compare clean: NaN fails `err > bound` as well
    as `err <= bound`, so the comparison has to be the second."""
    ref = (torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64))
    assert R.worst(torch.zeros(4), ref) == (0.0, 0)
    for poison in (float("nan"), float("inf"), -float("inf")):
        got = torch.zeros(4)
        got[2] = poison
        ratio, n_bad = R.worst(got, ref)
        assert n_bad == 1 and ratio == float("inf"), (poison, ratio, n_bad)
        with pytest.raises(AssertionError):
            R.check(got, ref, "poisoned")
        # a NaN given makes the reference NaN: that is outside too, whatever the output
        assert R.worst(torch.zeros(4), (got.double(), ref[1]))[1] == 1
        assert R.worst(torch.zeros(4), (ref[0], got.double().abs() * 0))[1] >= 1
    # through the whole backward reference: one NaN in dy, one NaN in the given mean
    d = case(300, 64)
    dy, _, dg, db = R.emulate_bwd(d["dout"], d["y"], d["keep"], d["mean"], d["invstd"],
                                  d["gamma"], True, d["dgamma0"], d["dbeta0"])
    dy = dy.clone()
    dy[17, 5] = float("nan")
    assert R.worst(dy, d["ref"]["dy"])[1] == 1
    mean = d["mean"].clone()
    mean[3] = float("nan")
    ref = R.bwd_ref(d["dout"], d["y"], d["keep"], mean, d["invstd"], d["gamma"], True,
                    d["dgamma0"], d["dbeta0"])
    nan_dy = torch.full_like(dy, float("nan"))
    assert R.worst(nan_dy, ref["dy"])[1] == nan_dy.numel()
    assert R.worst(dg, ref["dgamma"])[1] == 1


@pytest.mark.parametrize("M,C", R.SHAPES)
def test_rows_per_block_mirrors_the_library(M, C):
    lib = L.load()
    rpb = R.bwd_rows_per_block(M, C)
    assert (M + rpb - 1) // rpb == lib.dfu_bn_bwd_blocks(M, C)


def test_shapes_reach_the_paths_they_are_there_for():
    """The table of test_bn_conformance_gpu.py's docstring, as arithmetic on the mirrors."""
    rl = R.bwd_row_lanes
    assert R.bwd_rows_per_block(300, 64) == rl(64) * R.RED_U          # one trip, tail block
    assert not R.bwd_admits(72) and R.bwd_admits(8)
    assert R.slices(16384 // 128) == 1 and 16384 % 128 == 0           # last unsliced size
    assert R.slices((16533 + 127) // 128) == 2 and 16533 % 128 == 21  # both finalizes sliced
    assert R.bwd_rows_per_block(16533, 64) == 128
    for M, C, tail in ((8200, 2048, 8), (10930, 1536, 18)):
        rpb = R.bwd_rows_per_block(M, C)
        assert rpb == 2 * rl(C) * R.RED_U == 32 and M % rpb == tail   # two trips of the loop
        assert R.slices((M + rpb - 1) // rpb) == 3
