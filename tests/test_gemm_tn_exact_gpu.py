"""csrc/gemm_tn.hip in bf16 and fp16, bit-exactly on small integers and inside the float64 bounds of
tests/gemm_ref.py on N(0,1) data -- at the edges of its ring of four 32-deep stages (K = 128: exactly full, every
refill clamped; partly wrapped; wrapped once; more than twice), across tiles and batches at tile counts that
are and are not multiples of 8, through operand views surrounded by NaN and a batched, row-strided output, and
at fp16 operand magnitudes whose products overflow the format (the accumulation must be fp32)."""
import pytest
import torch

import dltb  # noqa: F401
from dltb.ops._ext import ext

from gemm_ref import (EXACT_LIMIT, TN, bound, ints, one_hot_blame, one_hot_probe, poisoned_view, product64,
                      report)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F64 = torch.bfloat16, torch.float16, torch.float64
FORMATS = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
RING_K = [128, 192, 256, 320, 576]          # 4, 6, 8, 10, 18 k-steps of 32 against a ring of four stages
SENTINEL = -7.0


def gen(seed):
    return torch.Generator(DEV).manual_seed(seed)


def bits(t):
    return t.contiguous().view(torch.int16)


def to16(x64, dtype):
    """The one rounding of an exact float64 integer result (below 2^24: torch's conversion through fp32 is exact)."""
    assert float(x64.abs().max()) < EXACT_LIMIT
    return x64.to(dtype)


def nan_out(shape, dtype):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def differs(what, out, ref):
    bad = (out != ref) | torch.isnan(out)
    return (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ ({int(torch.isnan(out).sum())} NaN = never "
            f"written), largest difference {float((out.double() - ref.double()).nan_to_num(0).abs().max())}")


# ================================================================================ exact small integers
# (batch, M, N): one tile; wm / wn addressing across tiles; 6 tiles (tiles & 7 != 0); 8 tiles
SHAPES = [(0, 256, 256), (0, 512, 256), (0, 256, 512), (3, 512, 256), (2, 512, 512)]


@FORMATS
@pytest.mark.parametrize("batch,M,N", SHAPES, ids=lambda v: str(v))
def test_exact_ring_edges(dtype, batch, M, N):
    C = ext()
    lead = (batch,) if batch else ()
    seed = M + 2 * N + 7 * batch
    for K in RING_K:
        assert C.gemm_tn_supported(M, N, K)
        for accumulate in (False, True):
            seed += 1
            g = gen(seed)
            a, b = ints(g, lead + (K, M), dtype), ints(g, lead + (K, N), dtype)
            assert K * 2 * 2 + 8 < EXACT_LIMIT
            want, _ = product64(a, b, TN)
            if accumulate:
                out = ints(g, lead + (M, N), dtype, -8, 8)
                want = want + out.double()
            else:
                out = nan_out(lead + (M, N), dtype)
            C.gemm_tn(a, b, out, accumulate)
            torch.cuda.synchronize()
            ref = to16(want, dtype)
            assert torch.equal(out, ref), differs(f"batch {batch} {M} x {N} x {K} accumulate {accumulate}", out, ref)


@FORMATS
def test_one_hot(dtype):
    """Each output element is one B value picked by a one-hot column of A: a k-step read twice, skipped, or from a
    ring slot refilled too early names the k it read."""
    M, N, K = 512, 256, 320
    a, b, want = one_hot_probe(M, N, K, dtype, TN, DEV)
    out = nan_out((M, N), dtype)
    ext().gemm_tn(a, b, out, False)
    torch.cuda.synchronize()
    assert torch.equal(out.double(), want.double()), one_hot_blame(out, want, K)


# ===================================================================== poisoned and strided operands
@FORMATS
@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("batch", [0, 3], ids=["2d", "batch3"])
def test_poisoned_strided(dtype, accumulate, batch):
    """a [K, M] and b [K, N] lie inside NaN-filled buffers (64 rows after K -- a refill that ran past the last
    stage would load them -- and 64 columns left and right), batched with a batch stride that is not rows x row
    stride; out is a (batched) view into a flat buffer with ldc = N + 8 and a slot larger than M rows: the
    result is exact, finite, and nothing between the rows or the slots is written."""
    C = ext()
    M, N, K = 512, 256, 192
    lead = (batch,) if batch else ()
    g = gen(900 + batch + accumulate)
    a, abuf = poisoned_view(ints(g, lead + (K, M), dtype), (0, 64), 64)
    b, bbuf = poisoned_view(ints(g, lead + (K, N), dtype), (0, 64), 64)
    assert a.stride(-2) == M + 128 and b.stride(-2) == N + 128
    if batch:
        assert a.stride(0) == (K + 64) * (M + 128) and b.stride(0) == (K + 64) * (N + 128)
    a_bits, b_bits = bits(abuf).clone(), bits(bbuf).clone()
    ldc, nb = N + 8, max(batch, 1)
    slot = M * ldc + 64
    flat = torch.full((nb * slot,), SENTINEL, device=DEV, dtype=dtype)
    out = flat.as_strided((nb, M, N), (slot, ldc, 1))
    mine = torch.zeros(nb * slot, dtype=torch.bool, device=DEV)
    mine.as_strided((nb, M, N), (slot, ldc, 1)).fill_(True)
    assert int(mine.sum()) == nb * M * N
    want, _ = product64(a, b, TN)
    want = want.reshape(nb, M, N)
    if accumulate:
        prev = ints(g, (nb, M, N), dtype, -8, 8)
        out.copy_(prev)
        want = want + prev.double()
    else:
        out.fill_(float("nan"))
    C.gemm_tn(a, b, out if batch else out[0], accumulate)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all(), f"{int((~torch.isfinite(out)).sum())} non-finite elements in out"
    ref = to16(want, dtype)
    assert torch.equal(out, ref), differs("strided", out, ref)
    assert torch.equal(bits(flat[~mine]), bits(torch.full_like(flat[~mine], SENTINEL))), "a gap was written"
    assert torch.equal(bits(abuf), a_bits) and torch.equal(bits(bbuf), b_bits)


# ========================================================================= float64-bounded random data
@FORMATS
@pytest.mark.parametrize("K", [128, 1152])
def test_bounded_random(dtype, K):
    C = ext()
    M, N = 512, 256
    name = "bf16" if dtype == BF16 else "fp16"
    g = gen(700 + K + (dtype == F16))
    a = torch.randn(K, M, device=DEV, generator=g).to(dtype)
    b = torch.randn(K, N, device=DEV, generator=g).to(dtype)
    prev = torch.randn(M, N, device=DEV, generator=g).to(dtype)
    want, abs_sum = product64(a, b, TN)
    out = nan_out((M, N), dtype)
    C.gemm_tn(a, b, out, False)
    torch.cuda.synchronize()
    report(f"gemm_tn {name} K {K}", out, want, bound(want, abs_sum, K, dtype))
    out = prev.clone()
    C.gemm_tn(a, b, out, True)
    torch.cuda.synchronize()
    wp = want + prev.double()
    report(f"gemm_tn {name} K {K} accumulate", out, wp, bound(wp, abs_sum, K, dtype, prev.double().abs()))


# ========================================================================================== fp16 range
def test_fp16_products_beyond_the_format():
    """fp16 operands of magnitude 1024: every product is +-2^20 (fp16's largest finite value is 65504), paired so
    that they cancel down to multiples of 1024 of at most 32768.  With sa [j, m] = +-1, sb [j, n] = +-1 and
    dl [j, n] in {-1, 0, 1} (non-zero for j < 32 only):

        a[2j] = a[2j + 1] = 1024 sa[j],   b[2j] = 1024 sb[j],   b[2j + 1] = -1024 sb[j] + dl[j]

    so out[m, n] = 1024 sum_j sa[j, m] dl[j, n].  1024 +- 1 is exact in fp16; every partial sum is a multiple of
    1024 below 2^27, exact in fp32 in any order.  An accumulation (or an operand product) that passed through
    fp16 overflows to inf."""
    C = ext()
    M, N, K = 512, 256, 128
    g = gen(77)
    J = K // 2
    sa = ints(g, (J, M), F16, 0, 1) * 2 - 1
    sb = ints(g, (J, N), F16, 0, 1) * 2 - 1
    dl = ints(g, (J, N), F16, -1, 1)
    dl[32:] = 0
    a = (1024 * sa).repeat_interleave(2, 0)
    b = torch.stack([1024 * sb, -1024 * sb + dl], 1).reshape(K, N)
    assert a.dtype == F16 and b.dtype == F16 and a.shape == (K, M) and b.shape == (K, N)
    assert torch.equal(b[1::2].double(), -1024 * sb.double() + dl.double())        # 1023 .. 1025 exact in fp16
    want, abs_sum = product64(a, b, TN)
    assert torch.equal(want, 1024 * (sa.double().t() @ dl.double()))
    assert float(want.abs().max()) <= 32768 < 60000 and float(want.abs().max()) >= 8192
    assert float((a.double()[:, :1] * b.double()[:, :1]).abs().min()) >= 2 ** 20 - 1024 > 65504
    assert float(abs_sum.max()) < 2 ** 28
    out = nan_out((M, N), F16)
    C.gemm_tn(a, b, out, False)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all(), f"{int((~torch.isfinite(out)).sum())} non-finite elements: fp16 overflow"
    assert torch.equal(out.double(), want), differs("fp16 range", out, want.to(F16))
