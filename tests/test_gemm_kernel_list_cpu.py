"""The list of compiled dfu_gemm kernels (tests/golden/gemm_kernels.json, tools/
gemm_kernel_list.py) against the built library, and the GPU matrix's coverage of it: every entry
has a case builder that returns cases of that very kernel (tile forced, no fallback)."""
import importlib.util
import os

import pytest

import gemm_ref as R
from dfu_hip import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location(
        "gemm_kernel_list", os.path.join(REPO, "tools", "gemm_kernel_list.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_live_probe_equals_the_committed_list():
    """A kernel added to or dropped from a dispatch table without regenerating the list fails
    here (and the tool reproduces the committed file byte for byte)."""
    tool = _tool()
    live = tool.probe(L.load())
    assert [tuple(k) for k in live] == R.kernels()
    with open(R.KERNELS_JSON) as f:
        assert tool.dumps(live) == f.read()
    assert len(set(map(tuple, live))) == len(live)


def _uncovered(kernels):
    """Entries of the list the matrix would not launch with their own tile forced."""
    bad = []
    for k in kernels:
        try:
            cases = R.cases_for(k)
        except LookupError:
            bad.append(k)
            continue
        if not cases or any(c.kernel != k or c.tile != k[0] for c in cases):
            bad.append(k)
    return bad


def test_every_kernel_has_a_forced_case():
    """The GPU matrix is parametrised over the same list, one test per entry, and each test runs
    gemm_ref.cases_for(entry): a case of that kernel for every entry, never a fallback."""
    import test_gemm_matrix_gpu as T
    assert T.KERNELS == R.kernels()
    assert not _uncovered(R.kernels())
    for k in R.kernels():
        cases = R.cases_for(k)
        regimes = {c.regime for c in cases}
        assert "gauss" in regimes and (k[3] in R.GELU_EPIS or "int" in regimes), R.kernel_id(k)
        if k[3] in R.BIAS_EPIS and k[1] < L.OPND_CONV_FWD:
            assert {c.bias for c in cases} == {False, True}, R.kernel_id(k)


def test_the_check_notices_a_deleted_case_builder(monkeypatch):
    """Without the builder of the conv weight-gradient kernels, exactly they are reported."""
    key = (L.OPND_MNMAJOR, L.OPND_CONV_WGRAD_X)
    builders = dict(R.BUILDERS)
    del builders[key]
    monkeypatch.setattr(R, "BUILDERS", builders)
    missing = _uncovered(R.kernels())
    assert missing and all((k[1], k[2]) == key for k in missing)
    assert len(missing) == sum((k[1], k[2]) == key for k in R.kernels())
    # and a builder that answers with another tile's kernel is no cover either
    monkeypatch.setattr(R, "BUILDERS", {**builders, key: lambda k: R.conv_cases((1,) + k[1:])})
    assert [k for k in _uncovered(R.kernels())] == [k for k in missing if k[0] != 1]
    with pytest.raises(LookupError):
        R.cases_for(next(k for k in missing if k[0] != 1))


def test_tail_split_cases_reach_the_tail_split():
    """The tail-split cases assert a non-zero workspace themselves (Case.expect_ws); here: both
    tiles have them, for every non-ACC epilogue of theirs."""
    for tile in (1, 5):
        ks = [k for k in R.kernels() if k[0] == tile and k[1] < L.OPND_CONV_FWD and k[2] < 2
              and k[3] != L.EPI_F32_ACC]
        assert ks
        for k in ks:
            assert any(c.expect_ws for c in R.cases_for(k)), R.kernel_id(k)
