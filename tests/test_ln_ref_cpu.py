"""The bounds of ln_ref.py checked without a GPU: an fp32 emulation of the LayerNorm forwards and
of the backward (the kernels' summation order; every a * b + c once rounded twice and once as an
fma) lies inside every bound at every element of every output, over every shape and regime of
the GPU test, and each deliberately broken variant lies outside one.  This is what keeps
test_ln_conformance_gpu.py honest.  The last test reproduces why the bounds exist: what the
tolerances of the older LayerNorm tests accept."""
import pytest
import torch

import ln_ref as R
from dfu_hip import _lib as L

BF16 = R.BF16
MUT_SHAPE = (40, 768)   # the edge shape of the workload's width, where the older tolerances
#                         accept the most (the last test)

_IN, _FWD, _BWD = {}, {}, {}


def inp(rows, D, regime):
    if (rows, D, regime) not in _IN:
        _IN[(rows, D, regime)] = R.inputs(rows, D, regime)
    return _IN[(rows, D, regime)]


def fwd_case(rows, D, regime, kind):
    """Inputs and the fp64 forward reference of one case, computed once."""
    key = (rows, D, regime, kind)
    if key not in _FWD:
        d = inp(rows, D, regime)
        _FWD[key] = (d, R.fwd_ref(d["x"], d["gamma"], d["beta"], R.LN_EPS, kind))
    return _FWD[key]


def bwd_case(rows, D, regime, dyk, shifted):
    """Inputs, givens (the fp64 statistics cast to fp32, or those moved by a few hundred ulps)
    and the fp64 backward reference from those givens, computed once."""
    key = (rows, D, regime, dyk, shifted)
    if key not in _BWD:
        d = inp(rows, D, regime)
        ref = R.fwd_ref(d["x"], d["gamma"], d["beta"], R.LN_EPS, "f32")
        mean, rstd = ref["mean"][0].float(), ref["rstd"][0].float()
        if shifted:
            mean, rstd = R.perturbed(mean, rstd)
        _BWD[key] = (d, mean, rstd,
                     R.bwd_ref(d["x"], d[dyk], d["gamma"], mean, rstd, d["gx0"]))
    return _BWD[key]


def fwd_ratios(got, ref):
    return {q: R.worst(got[q], ref[q]) for q in ref}


def bwd_ratios(got, ref):
    return {"gx": R.worst(got["gx"], ref["gx"]),
            "dgamma_p": R.worst(got["partial"][:, 0], ref["dgamma_p"]),
            "dbeta_p": R.worst(got["partial"][:, 1], ref["dbeta_p"]),
            "gsum_p": R.worst(got["gsum_p"], ref["gsum_p"])}


def bwd_exact(got, dy, rows):
    """The bit-for-bit checks of the GPU test, on an emulation's outputs."""
    return {"gx_bf16 == rne(gx)": torch.equal(got["gx_bf"], R.bf16_rne_bits(got["gx"])),
            "gsum == rows of own gx": R.same_bits(got["gsum_p"],
                                                  R.block_row_sums(got["gx"], rows)),
            "dbeta == rows of dy": R.same_bits(got["partial"][:, 1].contiguous(),
                                               R.block_row_sums(dy.float(), rows))}


def show(tag, res):
    print(f"{tag}: worst err/bound " + ", ".join(f"{q} {r:.3f}" for q, (r, _) in res.items()))


def inside(tag, res):
    show(tag, res)
    for q, (ratio, n_bad) in res.items():
        assert n_bad == 0, f"{tag} {q}: {n_bad} outside the bound, worst err/bound {ratio:.3g}"


# ------------------------------------------------------------------ the emulation is inside
@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("rows,D,ld,regime", R.FWD_CASES)
def test_forward_emulation_inside_every_bound(rows, D, ld, regime, kind, contract):
    d, ref = fwd_case(rows, D, regime, kind)
    got = R.emulate_fwd(d["x"], d["gamma"], d["beta"], R.LN_EPS, kind, contract)
    inside(f"ln fwd {kind} ({rows}, {D}) {regime} fma={int(contract)}", fwd_ratios(got, ref))


@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("kind", ["x3", "h16"])
@pytest.mark.parametrize("rows,D,ld,regime", R.X3_CASES)
def test_forward_x3_h16_emulation_inside_every_bound(rows, D, ld, regime, kind, contract):
    d, ref = fwd_case(rows, D, regime, kind)
    got = R.emulate_fwd(d["x"], d["gamma"], d["beta"], R.LN_EPS, kind, contract)
    inside(f"ln fwd {kind} ({rows}, {D}) {regime} fma={int(contract)}", fwd_ratios(got, ref))


@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("dyk", ["dy16", "dy32"])
@pytest.mark.parametrize("rows,D,ld,regime", R.BWD_CASES)
def test_backward_emulation_inside_every_bound(rows, D, ld, regime, dyk, contract):
    """From both sets of givens; the bit-for-bit checks hold on the emulation too."""
    for shifted in (False, True):
        d, mean, rstd, ref = bwd_case(rows, D, regime, dyk, shifted)
        got = R.emulate_bwd(d["x"], d[dyk], d["gamma"], mean, rstd, d["gx0"], contract)
        inside(f"ln bwd {dyk} ({rows}, {D}) {regime} fma={int(contract)} shifted={int(shifted)}",
               bwd_ratios(got, ref))
        for what, ok in bwd_exact(got, d[dyk], rows).items():
            assert ok, what


@pytest.mark.parametrize("kind", R.FWD_KINDS)
def test_a_constant_row_gives_beta_bit_for_bit(kind):
    D = 264 if kind in ("x3", "h16") else 260
    d = inp(5, D, "const")
    for contract in (False, True):
        got = R.emulate_fwd(d["x"], d["gamma"], d["beta"], R.LN_EPS, kind, contract)
        assert torch.equal(got["mean"], d["x"][:, 0])
        want = d["beta"].expand(5, D)
        if kind == "f32":
            assert R.same_bits(got["out"], want.contiguous())
        elif kind == "x3":
            hi = want.to(BF16)
            assert R.same_bits(got["hi"], hi)
            assert R.same_bits(got["lo"], (want - hi.float()).to(BF16))
        else:
            assert R.same_bits(got["out"], want.to(got["out"].dtype))


# ------------------------------------------------------------------ every mutation is outside
def fwd_mutant(rows, D, regime, kind, mutation, contract):
    d, ref = fwd_case(rows, D, regime, kind)
    res = fwd_ratios(R.emulate_fwd(d["x"], d["gamma"], d["beta"], R.LN_EPS, kind, contract,
                                   mutation), ref)
    print(f"ln fwd {kind} ({rows}, {D}) {regime} fma={int(contract)} {mutation}: " +
          ", ".join(f"{q} {n} bad, worst {r:.3g}" for q, (r, n) in res.items()))
    return any(n_bad for _, n_bad in res.values())


@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("kind", ["bf16", "f32", "x3", "h16"])
@pytest.mark.parametrize("mutation", R.FWD_MUTATIONS)
def test_every_forward_mutation_is_rejected(mutation, kind, contract):
    """At (40, 768) gauss, and in the regime named for it.  A one-pass variance on 3 randn + 1
    (E x^2 = 10 against var = 9) loses no more than the two-pass form's own roundings: it is
    printed there and asserted in `offset`, where E x^2 = 64 stands against var = 1 / 16."""
    rejected = fwd_mutant(*MUT_SHAPE, "gauss", kind, mutation, contract)
    if mutation != "one_pass_variance":
        assert rejected, f"{mutation} passes every bound at {MUT_SHAPE} gauss"
    regime = {"eps_x1000": "flat", "one_pass_variance": "offset"}.get(mutation)
    if regime:
        assert fwd_mutant(*MUT_SHAPE, regime, kind, mutation, contract), \
            f"{mutation} passes every bound at {MUT_SHAPE} {regime}"


@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("mutation", R.BWD_MUTATIONS)
def test_every_backward_mutation_is_rejected(mutation, contract):
    """At (40, 768) gauss (row 31 exists, a second block of 8 rows), by a bound or by one of the
    bit-for-bit checks; never on both sets of givens by accident: each set is asserted."""
    rows, D = MUT_SHAPE
    dyk = "dy32" if mutation == "dy_rounded_to_bf16" else "dy16"
    for shifted in (False, True):
        d, mean, rstd, ref = bwd_case(rows, D, "gauss", dyk, shifted)
        got = R.emulate_bwd(d["x"], d[dyk], d["gamma"], mean, rstd, d["gx0"], contract, mutation)
        res = bwd_ratios(got, ref)
        exact = bwd_exact(got, d[dyk], rows)
        print(f"ln bwd {MUT_SHAPE} fma={int(contract)} shifted={int(shifted)} {mutation}: " +
              ", ".join(f"{q} {n} bad, worst {r:.3g}" for q, (r, n) in res.items()) +
              "; bitwise failing: " + (", ".join(k for k, ok in exact.items() if not ok) or "-"))
        assert any(n for _, n in res.values()) or not all(exact.values()), \
            f"{mutation} passes every check"


def test_a_backward_that_recomputes_the_statistics_is_rejected_on_shifted_givens():
    """The reason for the second set of givens: outputs computed from the unshifted statistics
    are inside the bounds of the unshifted reference and outside those of the shifted one."""
    rows, D = MUT_SHAPE
    d, mean, rstd, ref = bwd_case(rows, D, "gauss", "dy16", False)
    _, _, _, ref_s = bwd_case(rows, D, "gauss", "dy16", True)
    got = R.emulate_bwd(d["x"], d["dy16"], d["gamma"], mean, rstd, d["gx0"])
    assert not any(n for _, n in bwd_ratios(got, ref).values())
    res = bwd_ratios(got, ref_s)
    show("ln bwd recomputed statistics against shifted givens", res)
    assert res["gx"][1] > 0 and res["dgamma_p"][1] > 0


def test_a_nan_or_inf_output_is_outside_every_bound():
    d, mean, rstd, ref = bwd_case(*MUT_SHAPE, "gauss", "dy16", False)
    got = R.emulate_bwd(d["x"], d["dy16"], d["gamma"], mean, rstd, d["gx0"])
    for poison in (float("nan"), float("inf")):
        gx = got["gx"].clone()
        gx[17, 5] = poison
        assert R.worst(gx, ref["gx"]) == (float("inf"), 1)
    nan_mean = mean.clone()
    nan_mean[3] = float("nan")
    bad = R.bwd_ref(d["x"], d["dy16"], d["gamma"], nan_mean, rstd, d["gx0"])
    assert R.worst(got["gx"], bad["gx"])[1] == MUT_SHAPE[1]
    _, fref = fwd_case(*MUT_SHAPE, "gauss", "bf16")
    assert R.worst(torch.full(MUT_SHAPE, float("nan")), fref["out"])[1] == 40 * 768


# ------------------------------------------------------------------ mirrors and exact orders
def test_block_count_and_template_mirror_the_library():
    lib = L.load()
    for rows in R.BWD_ROWS + (64, 1024, 12608):
        assert R.bwd_blocks(rows) == lib.dfu_ln_bwd_blocks(rows), rows
    assert R.bwd_blocks(1100) == 35                      # a reduce lane takes a second partial
    assert [R.bwd_nv(D) for D in (764, 768, 772, 1024)] == [3, 3, 4, 4]


def test_bf16_rne_bits_is_round_to_nearest_even():
    gen = torch.Generator().manual_seed(3)
    v = torch.randn(4096, generator=gen) * 100
    ties = torch.tensor([1.00390625, 1.01171875, -1.00390625, 3.0e38, 0.0, -0.0])  # odd/even ties
    v = torch.cat([v, ties])
    assert torch.equal(R.bf16_rne_bits(v), v.to(BF16).view(torch.int16))
    assert R.bf16_rne_bits(ties[:2]).tolist() == [0x3F80, 0x3F82]


def test_reduce_partials_order():
    """35 blocks: lanes 0..2 add two partials; the result is within G(depth) of fp64 and the
    order is the documented one (checked on integers, where every order agrees, and on a
    hand-made case where it does not)."""
    gen = torch.Generator().manual_seed(4)
    p = torch.randn(35, 16, generator=gen)
    out0 = torch.randn(16, generator=gen)
    got = R.reduce_partials(p, out0)
    exact = out0.double() + p.double().sum(0)
    bound = R.G(1 + 31 + 1) * (out0.double().abs() + p.double().abs().sum(0))
    assert R.worst(got, (exact, bound))[1] == 0
    q = torch.zeros(33, 1)
    q[0], q[1], q[32] = 1.0, 2.0 ** -24, 2.0 ** -24
    # lane 0: 1 + 2^-24 (block 32) rounds to 1, then + lane 1's 2^-24 rounds to 1 again;
    # any order that adds the two small terms first gives 1 + 2^-23
    assert R.reduce_partials(q, torch.zeros(1)).item() == 1.0


# ------------------------------------------------------------------ why: the older tolerances
OLD_SHAPES = ((1000, 768, 768), (33, 260, 264), (40, 768, 772))
DRAWS = 8


@pytest.mark.parametrize("mutation", R.OLD_TOL_MUTATIONS)
def test_the_older_tolerances_accept_these_wrong_kernels(mutation):
    """atol = 3e-2 / rtol = 1e-2 on out, 1e-3 / 1e-3 on dx and 2e-2 / 1e-2 on gx_bf16.  Every
    statistics and rounding-mode error passes them at every shape, on the edge tests' own inputs
    and on every other draw.  A tail-chunk error moves a row by what its last four columns
    happen to hold: at the one edge shape of the workload's width, (40, 768), it is within a
    factor of three of the tolerance either way, so whether the older tests catch it is a
    property of the seed (the forward's passes on the edge test's own inputs; some draws of the
    backward's pass too).  Documents the gap the derived bounds close."""
    own = [R.old_tolerance_ratio(*s, mutation) for s in OLD_SHAPES]
    print(f"old tolerance, {mutation}, the edge tests' inputs: worst err/tol " +
          ", ".join(f"{r:.3g}" for r in own))
    draws = [R.old_tolerance_ratio(*OLD_SHAPES[2], mutation, draw=k) for k in range(DRAWS)]
    print(f"old tolerance, {mutation}, (40, 768) over {DRAWS} draws: " +
          ", ".join(f"{r:.3g}" for r in draws))
    if "skip_last" not in mutation:
        assert max(own + draws) < 1
    else:
        assert min(draws) < 1 and max(draws) < 10
        if mutation.startswith("fwd"):
            assert own[2] < 1
