"""One test per compiled dfu_gemm kernel (tests/golden/gemm_kernels.json): the kernel's tile is
forced, dfu_gemm_plan must answer that tile before the launch, and there is no fallback to the
automatic plan.  Each test loops over the small shapes of gemm_ref.cases_for and names the
failing one.  With (TM, TN) the tile's size:

  M in {24, TM + 37}; N in {TN + 8, TN + 12, TN + 13} (the 16-byte merged, 4-column vector and
  scalar store classes, every leading dimension in the same class), once with ldaux / ldaux_out
  in another class, once N = 2 for a bf16 output; K-contiguous operands K in {8, 64, 136, 200}
  with ld = K + 8, MN x MN kernels K in {5, 64, 150}, MN-major ld = round8(MN) + 8; PATCH with 59
  tokens and the smallest batch with M > TM (class-token rows untouched); x3-pair kernels
  a_seg in {32, 96}; bias NULL and given; BF16_ADD / F32_RESID also in place; F32_ACC on a
  non-zero C, split-K (slabs with each reduce kernel, in-kernel reduction, fp32 atomics); the tail
  split on tiles 1 and 5.  Guards, NaN poison and the zeroed tile counters are checked after
  every launch; values against fp64, bit for bit in the integer regime and within the derived
  bound in the Gaussian one (gemm_ref.py)."""
import pytest

import gemm_ref as R

KERNELS = R.kernels()

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _ratios():
    yield
    print("\n" + R.RATIOS.report("test_gemm_matrix_gpu"))


@pytest.mark.parametrize("kernel", KERNELS, ids=[R.kernel_id(k) for k in KERNELS])
def test_kernel(kernel):
    for case in R.cases_for(kernel):
        R.run_case(case)


@pytest.mark.parametrize("kernel", R.ALIGN_KERNELS, ids=[R.kernel_id(k) for k in R.ALIGN_KERNELS])
def test_output_pointer_alignment(kernel):
    """C, aux and aux_out at 8, 4, 2 and 1 elements from an aligned base: a vector store class
    holds only while every access of it is naturally aligned, anything else runs the scalar
    class (the rule of include/dfu_hip.h); values and guards as everywhere."""
    assert kernel in KERNELS
    for case in R.alignment_cases(kernel):
        R.run_case(case)
