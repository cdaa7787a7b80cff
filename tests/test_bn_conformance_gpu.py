"""The BatchNorm kernels of csrc/bn.hip against the fp64 references and derived bounds of
bn_ref.py (test_bn_ref_cpu.py shows those bounds accept a faithful fp32 evaluation everywhere
and reject a dropped mean-correction term, a missing row, a wrong divisor and an ignored mask).
Every element of every output is compared; the references are plain torch operations on the
device.

    M, C          reaches
    1, 8  2, 8    var = 0 and n = 1 (running_var without Bessel), one vector per row,
                  k_bn_finalize<16> with 8 of its 16 channel lanes idle
    300, 64       the unsliced finalizes, a one-trip reduce with a tail block, FIXED apply
    257, 72       k_bn_finalize<32> with a ragged channel group, the general apply, a one-row
                  last tile; the backward refuses the width
    2053, 128     y = 8 + 0.25 randn: the cancellation in shift and in kb y + kc
    16384, 64     exactly 128 tiles and row-blocks: the last unsliced size, inv_last = 1 / 128
    16533, 64     130 tiles and row-blocks: both finalizes sliced (S = 2), 21-row last tile/block
    8200, 2048    rpb doubled to 32: two trips of the reduce loop, an 8-row last block with
                  masked reload rows, 4 column groups, sliced backward finalize S = 3, FIXED
                  with 256 vectors per row
    10930, 1536   the general apply and backward-apply with a doubled rpb

Every output buffer starts filled with NaN (the bitmask with 0xA5), so an element a kernel never
writes is outside its bound instead of showing what the allocator left there.  Each test prints
its worst error / bound per quantity.
"""
import pytest
import torch

import bn_ref as R
from dfu_hip import _lib as L
from dfu_hip import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
EPS, MOMENTUM = 1e-5, 0.1
SHAPES = R.SHAPES

_CASES = {}


def P(t):
    return None if t is None else t.data_ptr()


def fresh(*shape, dtype=F32):
    """An output buffer no kernel has written: NaN everywhere (bn_ref.check rejects NaN)."""
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def fresh_mask(M, C):
    return torch.full((M * C // 8,), 0xA5, dtype=torch.uint8, device=DEV)


def same_bits(a, b):
    v = torch.int16 if a.element_size() == 2 else torch.int32 if a.element_size() == 4 else None
    return a.shape == b.shape and a.dtype == b.dtype and (
        torch.equal(a, b) if v is None else torch.equal(a.view(v), b.view(v)))


def counters_are_zero(dev):
    torch.cuda.synchronize()
    return int(ops.tile_counters(dev).count_nonzero()) == 0


def finalize(stats, M, C, gamma, beta, rm, rv, nbt, direct=False):
    """ops.bn_finalize (sliced when there are more than 128 tiles), or dfu_bn_finalize itself
    with no workspace (one slice).  Returns mean, invstd, scale, shift."""
    o = [fresh(C) for _ in range(4)]
    if direct:
        L.check(L.load().dfu_bn_finalize(P(stats), ops.stats_tiles(M), M, C, P(gamma), P(beta),
                                         EPS, MOMENTUM, P(rm), P(rv), P(nbt), *map(P, o), None,
                                         None, 0, ops.stream_ptr()), "dfu_bn_finalize")
    else:
        ops.bn_finalize(stats, M, C, gamma, beta, EPS, MOMENTUM, rm, rv, nbt, *o)
    return o


def case(M, C):
    """One shape's inputs on the device, its tile records and the kernel's own mean / invstd /
    scale / shift (the givens of the apply and backward references), made once."""
    if (M, C) not in _CASES:
        d = {k: v.to(DEV) for k, v in R.inputs(M, C).items()}
        d["stats"] = ops.bn_tile_stats(d["y"], M, C)
        d["mean"], d["invstd"], d["scale"], d["shift"] = finalize(
            d["stats"], M, C, d["gamma"], d["beta"], None, None, None)
        _CASES[(M, C)] = d
    return _CASES[(M, C)]


# ------------------------------------------------------------------------------ forward
FIN_NAMES = ("mean", "invstd", "scale", "shift", "running_mean", "running_var")


@pytest.mark.parametrize("M,C", SHAPES)
def test_bn_finalize(M, C):
    d = case(M, C)
    stats, dev = d["stats"], d["y"].device
    sliced = R.slices(ops.stats_tiles(M)) > 1
    gen = torch.Generator().manual_seed(600 + M)
    rm0 = torch.randn(C, generator=gen).to(DEV)
    rv0 = (0.5 + torch.rand(C, generator=gen)).to(DEV)

    def run(gamma, beta, direct=False):
        rm, rv = rm0.clone(), rv0.clone()
        nbt = torch.tensor([41], dtype=torch.int64, device=DEV)
        got = finalize(stats, M, C, gamma, beta, rm, rv, nbt, direct) + [rm, rv]
        assert nbt.item() == 42, f"num_batches_tracked 41 -> {nbt.item()}"
        if sliced:
            assert counters_are_zero(dev), "finalize left a slice counter non-zero"
        return got

    e2e = R.finalize_from_data(d["y"], EPS)
    for gamma, beta, what in ((d["gamma"], d["beta"], "affine"), (None, None, "gamma=beta=None")):
        ref = R.finalize_from_records(stats, M, gamma, beta, EPS, MOMENTUM, rm0, rv0)
        runs = [("", False)] + ([("one slice ", True)] if sliced else [])
        for tag, direct in runs:
            got = run(gamma, beta, direct)
            worst = {n: R.check(t, ref[n], f"finalize {tag}{what} {n}")
                     for n, t in zip(FIN_NAMES, got)}
            worst["e2e mean"] = R.check(got[0], e2e["mean"], f"finalize {tag}{what} mean from data")
            worst["e2e invstd"] = R.check(got[1], e2e["invstd"],
                                          f"finalize {tag}{what} invstd from data")
            print(f"bn_finalize ({M}, {C}) {tag}{what}: worst err/bound " +
                  ", ".join(f"{n} {r:.3f}" for n, r in worst.items()))
            for a, b, n in zip(got, run(gamma, beta, direct), FIN_NAMES):
                assert same_bits(a, b), f"finalize {tag}{what}: {n} differs between two calls"


@pytest.mark.parametrize("M,C", SHAPES)
def test_bn_apply(M, C):
    d = case(M, C)
    y, scale, shift = d["y"], d["scale"], d["shift"]
    for res, relu in ((None, False), (None, True), (d["res"], True)):
        what = f"apply ({M}, {C}) res={res is not None} relu={relu}"
        out = fresh(M, C, dtype=BF16)
        ops.bn_apply(y, scale, shift, res, relu, out, M, C)
        ratio = R.check(out, R.apply_ref(y, scale, shift, res, relu), what)
        print(f"bn_{what}: worst err/bound {ratio:.3f}")
        masked, mask = fresh(M, C, dtype=BF16), fresh_mask(M, C)
        ops.bn_apply(y, scale, shift, res, relu, masked, M, C, mask=mask)
        assert same_bits(masked, out), f"{what}: bn_apply_mask != bn_apply"
        assert torch.equal(R.mask_bits(mask, M, C), out.float() > 0), f"{what}: mask != (out > 0)"


# ------------------------------------------------------------------------------ backward
BWD_NAMES = ("dy", "dres", "dgamma", "dbeta")


def bwd(d, M, C, relu, out, batch_stats, dres=True, dgamma=True, dbeta=True):
    """ops.bn_bwd into fresh outputs, dgamma / dbeta preloaded with the case's random values;
    returns dy, dres, dgamma, dbeta (None where not asked for)."""
    y = d["y"]
    dy = fresh(M, C, dtype=BF16)
    dr = fresh(M, C, dtype=BF16) if dres else None
    dg = d["dgamma0"].clone() if dgamma else None
    db = d["dbeta0"].clone() if dbeta else None
    ops.bn_bwd(d["dout"], y, out, relu, d["mean"], d["invstd"], d["gamma"], M, C, dy, dr, dg, db,
               batch_stats=batch_stats, scale=d["scale"], shift=d["shift"])
    return dy, dr, dg, db


@pytest.mark.parametrize("batch_stats", [True, False])
@pytest.mark.parametrize("M,C", SHAPES)
def test_bn_bwd(M, C, batch_stats):
    d = case(M, C)
    y, dout, dev = d["y"], d["dout"], d["y"].device
    if not R.bwd_admits(C):
        dy, dres = torch.full_like(y, 7.0), torch.full_like(y, 7.0)
        dg, db = torch.full((C,), 7.0, device=DEV), torch.full((C,), 7.0, device=DEV)
        with pytest.raises(L.DfuError) as e:
            ops.bn_bwd(dout, y, None, 0, d["mean"], d["invstd"], d["gamma"], M, C, dy, dres, dg,
                       db, batch_stats=batch_stats)
        assert e.value.code == L.DFU_E_INVALID and "unsupported" in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert all((t == 7.0).all() for t in (dy, dres, dg, db)), "a refused call wrote an output"
        return
    rpb = R.bwd_rows_per_block(M, C)
    sliced = R.slices((M + rpb - 1) // rpb) > 1

    out_res, out, mask = fresh(M, C, dtype=BF16), fresh(M, C, dtype=BF16), fresh_mask(M, C)
    ops.bn_apply(y, d["scale"], d["shift"], d["res"], True, out_res, M, C)
    ops.bn_apply(y, d["scale"], d["shift"], None, True, out, M, C, mask=mask)
    assert out_res.isfinite().all() and out.isfinite().all()  # bounds: test_bn_apply
    assert torch.equal(R.mask_bits(mask, M, C), out.float() > 0)

    def against_ref(got, keep, what):
        ref = R.bwd_ref(dout, y, keep, d["mean"], d["invstd"], d["gamma"], batch_stats,
                        d["dgamma0"], d["dbeta0"])
        worst = {q: R.check(t, ref[q], f"bn_bwd ({M}, {C}) {what} {q}")
                 for q, t in (("dy", got[0]), ("dgamma", got[2]), ("dbeta", got[3]))}
        if got[1] is not None:
            want = dout if keep is None else torch.where(keep, dout, torch.zeros_like(dout))
            assert same_bits(got[1], want), f"{what}: dres != mask ? dout : 0"
        print(f"bn_bwd ({M}, {C}) batch_stats={int(batch_stats)} {what}: worst err/bound " +
              ", ".join(f"{q} {r:.3f}" for q, r in worst.items()))
        if sliced:
            assert counters_are_zero(dev), f"{what}: a slice counter is left non-zero"

    against_ref(bwd(d, M, C, 0, None, batch_stats), None, "relu=0")
    full = bwd(d, M, C, 1, out_res, batch_stats)
    against_ref(full, out_res.float() > 0, "relu=1 residual")
    r1 = bwd(d, M, C, 1, out, batch_stats)
    against_ref(r1, out.float() > 0, "relu=1")
    for mode, o in ((2, None), (3, mask)):
        for a, b, q in zip(r1, bwd(d, M, C, mode, o, batch_stats), BWD_NAMES):
            assert same_bits(a, b), f"relu={mode}: {q} differs from relu=1"
    # an output not asked for leaves the others as they were
    for drop in ("dgamma", "dbeta", "dres"):
        got = bwd(d, M, C, 1, out_res, batch_stats, **{drop: False})
        for a, b, q in zip(full, got, BWD_NAMES):
            if q == drop:
                assert b is None
            else:
                assert same_bits(a, b), f"{drop}=None changes {q}"
    if sliced:
        assert counters_are_zero(dev)
