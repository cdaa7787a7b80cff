"""The limits of attn_ref.py checked without a GPU: an fp32 emulation of k_attn_fwd and
k_attn_bwd_fused (padding to NPAD, the masks, the roundings at the kernel's points) lies inside
every limit at every element, and each deliberately broken variant of it lies outside one.  This
is what keeps test_attn_conformance_gpu.py honest: its limits are neither so tight that a
faithful fp32 evaluation misses them nor so wide that a lost key, a lost query, a leaked padding
key or a short Delta passes.  The backward is emulated twice: as the dQ pass stood before it
masked the padding keys of a partly filled tile, and with the mask; the `far` regime is where
the two differ."""
import pytest
import torch

import attn_ref as R
from dfu_hip import _lib as L

B, H = 1, 2
SCALE = R.DH ** -0.5
NS = [2, 17, 33, 97, 193, 197, 225, 255]
OLD_O_ATOL, OLD_D_ATOL = 2e-2, 3e-2  # test_attention / test_attention_bf16_every_length
WORST = R.Worst()
_CASES = {}


def case(N, regime):
    """Inputs, the unmutated forward emulation (the backward's givens) and both references of
    one shape and regime, computed once and left unchanged."""
    if (N, regime) not in _CASES:
        qkv, dout = R.inputs(B, H, N, regime)
        o, lse = R.emulate_fwd(qkv, SCALE, B, H, N)
        q, k, v = R.heads(qkv, B, H, N)
        _CASES[(N, regime)] = {
            "qkv": qkv, "dout": dout, "o": o, "lse": lse,
            "fwd": R.fwd_ref(q, k, v, SCALE, "bf16"),
            "bwd": R.bwd_ref(qkv, o, lse, dout, SCALE, B, H, N)}
    return _CASES[(N, regime)]


def fwd_worst(d, N, mutation=None):
    o, lse = R.emulate_fwd(d["qkv"], SCALE, B, H, N, mutation)
    return {"o": R.worst(R.rows(o, B, H, N), d["fwd"]["o"]),
            "lse": R.worst(lse[:, :N].reshape(B, H, N), d["fwd"]["lse"])}


def bwd_worst(d, N, mutation=None, mask=False):
    dqkv = R.emulate_bwd(d["qkv"], d["o"], d["lse"], d["dout"], SCALE, B, H, N, mutation, mask)
    return {n: R.worst(t, d["bwd"][n]) for n, t in zip(("dq", "dk", "dv"), R.heads(dqkv, B, H, N))}


def show(tag, res):
    print(f"attn emulation {tag}: " +
          ", ".join(f"{q} {n} bad, worst {r:.3g}" for q, (r, n) in res.items()))


@pytest.mark.parametrize("regime", ["gauss", "two_peak", "shifted"])
@pytest.mark.parametrize("N", NS)
def test_emulation_inside_every_limit(N, regime):
    """No element excluded, forward and backward, the backward with and without the padding
    mask (in these regimes exp2(-Ls) is finite, so the unmasked dS is finite and its product
    with the zero K rows is an exact zero: the two are the same numbers)."""
    d = case(N, regime)
    res = fwd_worst(d, N)
    res.update(bwd_worst(d, N))
    masked = bwd_worst(d, N, mask=True)
    show(f"N={N} {regime}", res)
    for q, (ratio, n_bad) in list(res.items()) + list(masked.items()):
        WORST.add(q, ratio)
        assert n_bad == 0, f"{q}: {n_bad} outside the limit, worst err/limit {ratio:.3f}"
    a = R.emulate_bwd(d["qkv"], d["o"], d["lse"], d["dout"], SCALE, B, H, N)
    b = R.emulate_bwd(d["qkv"], d["o"], d["lse"], d["dout"], SCALE, B, H, N, mask_pad_keys=True)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_worst_ratios_report():
    """Runs after the cases above in file order; prints what they collected."""
    print(WORST.report("fp32 emulation, gauss / two_peak / shifted"))


@pytest.mark.parametrize("N", NS)
def test_forward_mutations_are_rejected(N):
    """drop_last_key in two_peak (query 0 puts half its mass on key N - 1); leak_pad_key in
    shifted (a zero score among scores of -30 takes the whole row) wherever a padding key
    exists."""
    res = fwd_worst(case(N, "two_peak"), N, "drop_last_key")
    show(f"N={N} two_peak drop_last_key", res)
    assert res["o"][1] > 0 and res["lse"][1] > 0
    res = fwd_worst(case(N, "shifted"), N, "leak_pad_key")
    show(f"N={N} shifted leak_pad_key", res)
    if N % 32:
        assert res["o"][1] > 0 and res["lse"][1] > 0
    else:
        assert res["o"][1] == 0 and res["lse"][1] == 0  # no padding key to leak


@pytest.mark.parametrize("N", NS)
def test_backward_mutations_are_rejected(N):
    """two_peak: drop_last_query acts in the dK/dV pass (dk and dv must each reject it; dq
    comes from the other pass and is unchanged), drop_last_key_dq in the dQ pass (dq), delta_56
    in the staging (dq and dk; dv does not use Delta)."""
    d = case(N, "two_peak")
    for mutation, outs in (("drop_last_query", ("dk", "dv")), ("drop_last_key_dq", ("dq",)),
                           ("delta_56", ("dq", "dk"))):
        res = bwd_worst(d, N, mutation)
        show(f"N={N} two_peak {mutation}", res)
        for q in outs:
            assert res[q][1] > 0, f"{mutation} passes the {q} limit (worst {res[q][0]:.3g})"


def test_what_the_old_tolerances_let_through():
    """For the record: the largest absolute error of each mutation on gauss data against the
    fp64 reference, beside the tolerances of test_attention (o 2e-2, dq / dk / dv 3e-2), and
    whether the derived limits reject it.  A Gaussian row spreads over all keys, so one lost key
    or query moves an output by about 1 / N of itself."""
    print(f"{'N':>4s} {'mutation':<17s} {'out':<3s} {'max err':>9s} {'old tol':>8s} old   derived")
    seen = {}
    for N in NS:
        d = case(N, "gauss")
        for mutation in R.FWD_MUTATIONS + R.BWD_MUTATIONS:
            if mutation in R.FWD_MUTATIONS:
                o, _ = R.emulate_fwd(d["qkv"], SCALE, B, H, N, mutation)
                got, refs, tol = {"o": R.rows(o, B, H, N)}, d["fwd"], OLD_O_ATOL
            else:
                dqkv = R.emulate_bwd(d["qkv"], d["o"], d["lse"], d["dout"], SCALE, B, H, N, mutation)
                got = dict(zip(("dq", "dk", "dv"), R.heads(dqkv, B, H, N)))
                refs, tol = d["bwd"], OLD_D_ATOL
            for q, t in got.items():
                err = (t.double() - refs[q][0]).abs().max().item()
                n_bad = R.worst(t, refs[q])[1]
                seen[(N, mutation, q)] = (err, tol, n_bad)
                print(f"{N:4d} {mutation:<17s} {q:<3s} {err:9.2e} {tol:8.0e} "
                      f"{'pass' if err <= tol else 'FAIL'}  {'pass' if n_bad == 0 else 'FAIL'}")
    # What holds by construction is asserted; the rest is the printed record.  A leaked padding
    # key (score 0 among N unit-normal scores) moves o by about 1 / N of itself: the old 2e-2
    # accepts it at every length of the workload's size, and on this data so does the derived o
    # limit at most of them -- only lse sees it on gauss, and the shifted regime is what makes o
    # see it (test_forward_mutations_are_rejected).  A lost last key or query is caught by the
    # old tolerances on this draw (the maximum over all queries finds one that gives key N - 1
    # several percent of its mass), but by two orders less margin than in two_peak.
    for N in (197, 225, 255):
        err, tol, _ = seen[(N, "leak_pad_key", "o")]
        assert err < tol, f"leak_pad_key at N = {N} on gauss data: {err:.2e} is outside 2e-2"
        _, lse = R.emulate_fwd(case(N, "gauss")["qkv"], SCALE, B, H, N, "leak_pad_key")
        assert R.worst(lse[:, :N].reshape(B, H, N), case(N, "gauss")["fwd"]["lse"])[1] > 0


def test_a_nan_or_inf_is_outside_every_limit():
    """In an output, in o_given or in lse_given."""
    ref = (torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64))
    assert R.worst(torch.zeros(4), ref) == (0.0, 0)
    for poison in (float("nan"), float("inf"), -float("inf")):
        got = torch.zeros(4)
        got[2] = poison
        ratio, n_bad = R.worst(got, ref)
        assert n_bad == 1 and ratio == float("inf"), (poison, ratio, n_bad)
        with pytest.raises(AssertionError):
            R.check(got, ref, "poisoned")
    N = 33
    d = case(N, "gauss")
    dqkv = R.emulate_bwd(d["qkv"], d["o"], d["lse"], d["dout"], SCALE, B, H, N)
    dq = R.heads(dqkv, B, H, N)[0].clone()
    dq[0, 1, 5, 7] = float("nan")
    assert R.worst(dq, d["bwd"]["dq"])[1] == 1
    for poison in (float("nan"), float("inf"), -float("inf")):
        for name in ("o", "lse"):
            givens = {"o": d["o"].clone(), "lse": d["lse"].clone()}
            givens[name][1, 3] = poison
            ref = R.bwd_ref(d["qkv"], givens["o"], givens["lse"], d["dout"], SCALE, B, H, N)
            for q, t in zip(("dq", "dk", "dv"), R.heads(dqkv, B, H, N)):
                assert R.worst(t, ref[q])[1] == t.numel(), (poison, name, q)
    # the lse columns >= N are no givens: whatever they hold, the reference is the same
    lse = d["lse"].clone()
    lse[:, N:] = float("inf")
    ref = R.bwd_ref(d["qkv"], d["o"], lse, d["dout"], SCALE, B, H, N)
    assert torch.equal(ref["dq"][1], d["bwd"]["dq"][1])


@pytest.mark.parametrize("N", [33, 197, 208, 224])
def test_far_regime_needs_the_padding_mask(N):
    """Scores near -110: exp2(-Ls) of a padding key overflows to +inf, dS = inf (0 - Delta) is
    +-inf (NaN where Delta = 0), and the product with the zero K row is NaN in every dq element
    of that query -- whenever N is no multiple of 16.  With the mask the emulation is inside
    every limit."""
    d = case(N, "far")
    assert d["lse"][:, :N].max().item() < -88.8
    res = fwd_worst(d, N)
    show(f"N={N} far forward", res)
    assert all(n == 0 for _, n in res.values())
    dqkv = R.emulate_bwd(d["qkv"], d["o"], d["lse"], d["dout"], SCALE, B, H, N)
    dq, dk, dv = R.heads(dqkv, B, H, N)
    assert dk.isfinite().all() and dv.isfinite().all()
    if N % 16:
        assert dq.isnan().any(), "the unmasked dQ pass was expected to produce NaN"
    else:
        assert dq.isfinite().all()
    masked = bwd_worst(d, N, mask=True)
    show(f"N={N} far backward, padding keys masked", masked)
    assert all(n == 0 for _, n in masked.values())


def test_npad_mirrors_the_library():
    lib = L.load()
    for N in range(1, 257):
        assert R.npad(N) == lib.dfu_attention_npad(N), N
