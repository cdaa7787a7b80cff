"""Implicit-GEMM convolution kernels on geometries that are square in nothing: H != W, R != S,
pad != R / 2, P != Q, stride phases of unequal extent or without a tap.  Forward (CONV_FWD with
BF16_STATS and BF16), input gradient (CONV_DGRAD x CONV_DGRAD_W with BF16, BF16_ADD, BF16_ADD in
place) and weight gradient (MNMAJOR x CONV_WGRAD_X, F32_ACC at split 1 and 3), each on every tile
of tests/golden/gemm_kernels.json that has the kernel, tile forced.  The reference is the
unfolded product in fp64; both data regimes, guards and NaN poison as in test_gemm_matrix_gpu.py
(gemm_ref.py): the NHWC tensors sit in guarded buffers, so a gather that steps off the image
reads NaN.

N = 2; H x W, R x S / stride / pad (gemm_ref.GEOMS): 9x13 3x3/1/1; 9x14 3x3/2/1 (H odd, W even:
P != Q, unequal phase extents); 7x10 3x3/1/0; 9x14 1x1/2/0 (three phases without a tap, the
phase fill on unequal Hs, Ws); 10x7 5x5/2/2 (3 and 2 live taps); 8x11 3x3/3/1; 6x9 1x3/1/0 and
3x1/1/0.  C = 64, K = 128; the gradients also at C = 72 (conv_c % 8 == 0 but % 64 != 0: the
weight gradient's N = R S 72), the forward also with 72 filters."""
import pytest

import gemm_ref as R
from dfu_hip import _lib as L

pytestmark = pytest.mark.gpu

FWD = [k for k in R.kernels() if k[1] == L.OPND_CONV_FWD and k[4] == "bf16"
       and k[3] in (L.EPI_BF16_STATS, L.EPI_BF16)]
DGRAD = [k for k in R.kernels() if k[1] == L.OPND_CONV_DGRAD]
WGRAD = [k for k in R.kernels() if k[2] == L.OPND_CONV_WGRAD_X]
ODD = [R.GEOMS[0], R.GEOMS[1], R.GEOMS[4]]  # the geometries of the C = 72 / 72-filter cases


def _geoms(direction):
    gs = [R.Geom(*g) for g in R.GEOMS]
    if direction == "fwd":
        return gs + [R.Geom(*g, k=72) for g in ODD]
    return gs + [R.Geom(*g, c=72) for g in ODD]


def _params(kernels, direction):
    return [pytest.param(k, g, id=f"{R.kernel_id(k)}-{g}".replace(" ", "_"))
            for k in kernels for g in _geoms(direction)]


@pytest.fixture(scope="module", autouse=True)
def _ratios():
    yield
    print("\n" + R.RATIOS.report("test_conv_geometry_gpu (and the modules before it)"))


def test_the_lists_are_not_empty():
    assert len(FWD) == 12 and len(DGRAD) == 10 and len(WGRAD) == 5


@pytest.mark.parametrize("kernel,geom", _params(FWD, "fwd"))
def test_forward(kernel, geom):
    for regime in ("int", "gauss"):
        R.run_case(R.conv_case(kernel, geom, regime, bias=kernel[3] == L.EPI_BF16))


@pytest.mark.parametrize("kernel,geom", _params(DGRAD, "dgrad"))
def test_input_gradient(kernel, geom):
    for regime in ("int", "gauss"):
        R.run_case(R.conv_case(kernel, geom, regime))
        if kernel[3] == L.EPI_BF16_ADD:
            R.run_case(R.conv_case(kernel, geom, regime, inplace=True))


@pytest.mark.parametrize("kernel,geom", _params(WGRAD, "wgrad"))
def test_weight_gradient(kernel, geom):
    for regime in ("int", "gauss"):
        for split in (1, 3):
            R.run_case(R.conv_case(kernel, geom, regime, split_k=split))
