"""Shared by the column-sum tests of the weight-gradient GEMM (tests/test_gemm_tn_colsum_gpu.py,
tests/test_bias_from_dw_cpu.py): the N(0,1) cases of the bounded test, generated on the CPU so that both files
see the same data, and their float64 reference.  Plain torch, no dltb import."""
import torch

from gemm_ref import bound

BF16, F16, F64 = torch.bfloat16, torch.float16, torch.float64

# (K, M, N, batch) of the bounded test: the ring of four stages exactly full (also the smallest K the kernel
# takes), a K that is no multiple of 128, and the largest K at which the bound still rejects a dropped term
# (tests/gemm_ref.py); 1 and 4 n-tiles
BOUNDED = [(128, 768, 256, 3), (192, 768, 1024, 3), (1152, 256, 1024, 1), (1152, 768, 256, 1)]


def bounded_seed(dtype, K, M, N, batch):
    return 4100 + K + M // 256 + 3 * (N // 256) + 7 * batch + (dtype == F16)


def bounded_case(dtype, K, M, N, batch):
    """(a [batch, K, M], x [batch, K, N], prev [batch, M]) N(0,1) in ``dtype`` on the CPU."""
    g = torch.Generator().manual_seed(bounded_seed(dtype, K, M, N, batch))
    a = torch.randn(batch, K, M, generator=g).to(dtype)
    x = torch.randn(batch, K, N, generator=g).to(dtype)
    prev = torch.randn(batch, M, generator=g).to(dtype)
    return a, x, prev


def colsum64(a):
    """(want, abs_sum): the float64 column sums of a [batch, K, M] over K, and the sums of the magnitudes."""
    a = a.double()
    return a.sum(-2), a.abs().sum(-2)


def colsum_bound(want, abs_sum, K, dtype, prev=None):
    """Half an ulp of the output format at ``want`` plus the order-free fp32 summation bound of
    tests/gemm_ref.py (a column sum is a product with a column of ones: K exact terms, plus the accumulate)."""
    return bound(want, abs_sum, K, dtype, 0.0 if prev is None else prev.double().abs())
