"""The column-sum output of csrc/gemm_tn.hip (the bias gradient dY^T 1 beside dW = dY^T X) in bf16 and fp16:
bit-exactly on small integers -- colsum against the once-rounded integer column sum, dW against the same call
without colsum -- with operands and outputs inside NaN-filled buffers, and inside the float64 bound of
tests/gemm_ref.py on N(0,1) data (the cases of tests/colsum_ref.py, whose reference tests/test_bias_from_dw_cpu.py
checks on the CPU).  K: 128 (the ring of four 32-deep stages exactly full, and the smallest K the kernel takes), 192
and 320 (no multiples of 128); M 256 / 768; N 256 / 1024 (1 and 4 n-tiles: only n-tile 0 forms the sums); batch 1
(2-D operands) and 3 (strided views); accumulate off / on independently for dW and colsum."""
import itertools

import pytest
import torch

import dltb  # noqa: F401
from dltb.ops._ext import ext

from colsum_ref import BOUNDED, bounded_case, colsum64, colsum_bound
from gemm_ref import EXACT_LIMIT, TN, ints, poisoned_view, product64, report

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
FORMATS = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
EXACT_K = [128, 192, 320]


def bits(t):
    return t.contiguous().view(torch.int16)


def to16(x64, dtype):
    assert float(x64.abs().max()) < EXACT_LIMIT
    return x64.to(dtype)


def strided_out(nb, shape, gap, dtype):
    """(view [nb, *shape], flat NaN-filled buffer, mask of the view's elements): rows padded by 8 elements and
    slots ``gap`` elements apart, so a store outside the view lands on a NaN that must stay."""
    if len(shape) == 2:
        ld = shape[1] + 8
        slot, strides = shape[0] * ld + gap, (ld, 1)
    else:
        slot, strides = shape[0] + gap, (1,)
    flat = torch.full((nb * slot,), float("nan"), device=DEV, dtype=dtype)
    view = flat.as_strided((nb,) + tuple(shape), (slot,) + strides)
    mine = torch.zeros(nb * slot, dtype=torch.bool, device=DEV)
    mine.as_strided(view.shape, view.stride()).fill_(True)
    assert int(mine.sum()) == view.numel()
    return view, flat, mine


@FORMATS
@pytest.mark.parametrize("batch", [1, 3], ids=["2d", "batch3"])
@pytest.mark.parametrize("N", [256, 1024])
@pytest.mark.parametrize("M", [256, 768])
def test_exact_poisoned(dtype, M, N, batch):
    C = ext()
    lead = (batch,) if batch > 1 else ()
    seed = 10 * M + N + batch
    for K, acc_w, acc_c in itertools.product(EXACT_K, (False, True), (False, True)):
        assert C.gemm_tn_supported(M, N, K) and K * 31 * 2 + 8 < EXACT_LIMIT
        seed += 1
        g = torch.Generator(DEV).manual_seed(seed)
        # dY in [-3, 31]: column sums near 14 K, past the 256 (bf16) and, from K = 192, the 2048 (fp16) up to
        # which every integer is a value of the format -- the one rounding of the store shows
        a, abuf = poisoned_view(ints(g, lead + (K, M), dtype, -3, 31), (0, 64), 64)
        x, xbuf = poisoned_view(ints(g, lead + (K, N), dtype), (0, 64), 64)
        a_bits, x_bits = bits(abuf).clone(), bits(xbuf).clone()
        prev_w = ints(g, (batch, M, N), dtype, -8, 8)
        prev_c = ints(g, (batch, M), dtype, -8, 8)
        outs = []
        for with_colsum in (False, True):
            dw, wflat, wmine = strided_out(batch, (M, N), 64, dtype)
            if acc_w:
                dw.copy_(prev_w)
            if with_colsum:
                cs, cflat, cmine = strided_out(batch, (M,), 24, dtype)
                if acc_c:
                    cs.copy_(prev_c)
                C.gemm_tn(a, x, dw if batch > 1 else dw[0], acc_w, cs if batch > 1 else cs[0], acc_c)
            else:
                C.gemm_tn(a, x, dw if batch > 1 else dw[0], acc_w)
            torch.cuda.synchronize()
            outs.append(dw)
            assert torch.isnan(wflat[~wmine]).all(), "a gap of the dW buffer was written"
        what = f"{M} x {N} x {K} batch {batch} accumulate dW {acc_w} colsum {acc_c}"
        want_w, _ = product64(a, x, TN)
        want_w = want_w.reshape(batch, M, N) + (prev_w.double() if acc_w else 0)
        assert torch.equal(outs[0], to16(want_w, dtype)), f"{what}: dW without colsum is not the exact product"
        assert torch.equal(bits(outs[1]), bits(outs[0])), f"{what}: dW differs between the calls with and without colsum"
        want_c = a.double().sum(-2).reshape(batch, M) + (prev_c.double() if acc_c else 0)
        ref = to16(want_c, dtype)
        assert float(want_c.abs().max()) > 1024, "the sums stay where every integer is exact in bf16"
        bad = (cs != ref) | torch.isnan(cs)
        assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} column sums differ ({int(torch.isnan(cs).sum())} "
                               f"NaN), first at {bad.nonzero()[0].tolist()}")
        assert torch.isnan(cflat[~cmine]).all(), "a gap of the colsum buffer was written"
        assert torch.equal(bits(abuf), a_bits) and torch.equal(bits(xbuf), x_bits)


@FORMATS
@pytest.mark.parametrize("K,M,N,batch", BOUNDED, ids=lambda v: str(v))
def test_bounded_random(dtype, K, M, N, batch):
    C = ext()
    name = "bf16" if dtype == BF16 else "fp16"
    a, x, prev = (t.to(DEV) for t in bounded_case(dtype, K, M, N, batch))
    want, abs_sum = colsum64(a)
    dw = torch.empty(batch, M, N, device=DEV, dtype=dtype)
    cs = torch.full((batch, M), float("nan"), device=DEV, dtype=dtype)
    C.gemm_tn(a, x, dw, False, cs, False)
    torch.cuda.synchronize()
    report(f"colsum {name} K {K} {M} x {N} batch {batch}", cs, want, colsum_bound(want, abs_sum, K, dtype))
    cs = prev.clone()
    C.gemm_tn(a, x, dw, False, cs, True)
    torch.cuda.synchronize()
    wp = want + prev.double()
    report(f"colsum {name} K {K} {M} x {N} batch {batch} accumulate", cs, wp,
           colsum_bound(wp, abs_sum, K, dtype, prev))


def test_queue_takes_bias_from_the_own_kernel():
    """parallel/wgrad.py: a batch of layer-strided products that fills the GPU runs on gemm_tn with the bias
    slots as its colsum output (one launch), and gives the per-block results."""
    from dltb.parallel.runtime import Unit
    from dltb.parallel.wgrad import WgradQueue
    L, M, N, K = 16, 1024, 1024, 128
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L = max(L, -(-cus // ((M // 256) * (N // 256))))
    g = torch.Generator(DEV).manual_seed(5)
    dyb, xb = ints(g, (L, K, M), BF16), ints(g, (L, K, N), BF16)
    slot = M * N + M + 64
    flat = torch.full((L * slot,), float("nan"), device=DEV, dtype=BF16)
    units = [Unit(f"b{i}", [(f"w{i}", torch.nn.Parameter(torch.zeros(1)))], i) for i in range(L)]
    q = WgradQueue()
    for i in reversed(range(L)):
        dw = flat[i * slot:i * slot + M * N].view(M, N)
        db = flat[i * slot + M * N:i * slot + M * N + M]
        q.add(units[i], 0, dyb[i], xb[i], dw, False, (db, False))
    q.flush()
    torch.cuda.synchronize()
    assert q.tn_bias_calls == 1 and q.batched_calls == 1 and q.single_calls == 0
    want_w, _ = product64(dyb, xb, TN)
    for i in range(L):
        assert torch.equal(flat[i * slot:i * slot + M * N].view(M, N), to16(want_w[i], BF16))
        assert torch.equal(flat[i * slot + M * N:i * slot + M * N + M], to16(dyb[i].double().sum(0), BF16))
        assert torch.isnan(flat[i * slot + M * N + M:(i + 1) * slot]).all()
