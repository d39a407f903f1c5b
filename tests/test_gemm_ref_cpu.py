"""The comparison of tests/gemm_ref.py has teeth: on the CPU, with N(0,1) operands in both 16-bit formats, its
bound accepts fp32 products in two summation orders and rejects planted defects (a dropped 32-wide k-step, a
dropped single term, a bias on the wrong 4-column group, a double rounding); the exact-test generators meet
their own exactness conditions.

The floors on the rejected shares were fixed from the bound's structure before being measured: a dropped
k-step removes 32 of K terms of unit variance (|defect| ~ sqrt(32), tens of half-ulps of a result of
magnitude sqrt(K)), so nearly every element must leave its bound; one dropped term is |a b| with median 0.43
against a bound of about one half-ulp of a value of magnitude sqrt(K) (2^-5 .. 2^-3 in bf16 at K <= 256,
more slack from the K-proportional term at K = 1152), so a clear majority must.  Measured: k-step 97.3 % or
more in all six cases; single term 90.6 - 98.0 % at K <= 256 and 63.8 - 78.3 % at K = 1152.  At K = 4096 the
order-free term is ten or more half-ulps wide and a dropped term is flagged in under 20 % of elements: the
bounded GPU tests therefore stay at K <= 1152."""
import pytest
import torch

from gemm_ref import (EXACT_LIMIT, MARGIN, NT, TN, U, bound, flagged, half_ulp, ints, one_hot_blame, one_hot_k,
                      one_hot_probe, poisoned_view, product64, report, round16)

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
FORMATS = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
DEPTHS = pytest.mark.parametrize("K", [128, 256, 1152])
M = N = 128


def gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


_cache = {}


def operands(dtype, K):
    """a [M, K], b [N, K], bias [N], prev [M, N] ~ N(0,1) in ``dtype``, the float64 product and abs_sum: computed
    once per (dtype, K) and never modified."""
    key = (dtype, K)
    if key not in _cache:
        g = gen(1000 + K + (dtype == F16))
        a = torch.randn(M, K, generator=g).to(dtype)
        b = torch.randn(N, K, generator=g).to(dtype)
        bias = torch.randn(N, generator=g).to(dtype)
        prev = torch.randn(M, N, generator=g).to(dtype)
        want, abs_sum = product64(a, b, NT)
        _cache[key] = (a, b, bias, prev, want, abs_sum)
    return _cache[key]


def test_constants():
    assert U == 2.0 ** -24 and MARGIN == 2.0 and EXACT_LIMIT == 2 ** 24


@FORMATS
@DEPTHS
def test_accepts_fp32_products(dtype, K):
    a, b, bias, prev, want, abs_sum = operands(dtype, K)
    bnd = bound(want, abs_sum, K, dtype)
    whole = (a.float() @ b.float().t()).to(dtype)
    r1 = report(f"torch fp32 product K {K}", whole, want, bnd)
    acc = torch.zeros(M, N, dtype=F32)
    for k0 in range(0, K, 32):
        acc = acc + a[:, k0:k0 + 32].float() @ b[:, k0:k0 + 32].float().t()
    r2 = report(f"32-wide k-steps K {K}", acc.to(dtype), want, bnd)
    assert 0.0 < r1 <= 1.0 and 0.0 < r2 <= 1.0
    # the epilogues: bias and accumulate in fp32, rounded once
    full = acc + bias.float() + prev.float()
    want_full = want + bias.double() + prev.double()
    report(f"bias + prev K {K}", full.to(dtype), want_full,
           bound(want_full, abs_sum, K, dtype, bias.double().abs() + prev.double().abs()))


@FORMATS
@DEPTHS
def test_rejects_dropped_k_step(dtype, K):
    a, b, _, _, want, abs_sum = operands(dtype, K)
    bnd = bound(want, abs_sum, K, dtype)
    k0 = 32 * ((K // 32) // 2)
    part, _ = product64(a[:, k0:k0 + 32], b[:, k0:k0 + 32], NT)
    share = flagged(round16(want - part, dtype), want, bnd)
    print(f"dropped k-step [{k0}, {k0 + 32}) of K {K}: {100 * share:.1f} % of elements flagged")
    assert share >= 0.95


@FORMATS
@DEPTHS
def test_rejects_dropped_term(dtype, K):
    a, b, _, _, want, abs_sum = operands(dtype, K)
    bnd = bound(want, abs_sum, K, dtype)
    k = K // 2 + 5
    term = a[:, k].double()[:, None] * b[:, k].double()[None, :]
    share = flagged(round16(want - term, dtype), want, bnd)
    print(f"dropped term k = {k} of K {K}: {100 * share:.1f} % of elements flagged")
    assert share >= (0.60 if K <= 256 else 0.50)


@FORMATS
@DEPTHS
def test_rejects_shifted_bias(dtype, K):
    """The bias of the neighbouring 4-column group: the difference of two N(0,1) values against a bound of a few
    percent of one, so four fifths of the elements at least."""
    a, b, bias, _, want, abs_sum = operands(dtype, K)
    want_b = want + bias.double()
    bnd = bound(want_b, abs_sum, K, dtype, bias.double().abs())
    share = flagged(round16(want + torch.roll(bias.double(), 4), dtype), want_b, bnd)
    print(f"bias shifted by 4 columns, K {K}: {100 * share:.1f} % of elements flagged")
    assert share >= 0.8
    assert flagged(round16(want_b, dtype), want_b, bnd) == 0.0


@FORMATS
@DEPTHS
def test_rejects_double_rounding(dtype, K):
    """Rounding the product to 16 bits BEFORE adding prev rounds twice: off by up to half_ulp(product) +
    half_ulp(sum).  At least one element must be flagged wherever the bound can see that at all.  It cannot in
    fp16 at K = 1152: there the order-free fp32 term alone (2 * 1154 * 2^-24 * abs_sum, about 0.09 with abs_sum
    about 730) exceeds the largest possible double-rounding error wherever |product| < 128 (2^-6 + 2^-6), and a
    product of standard deviation 34 reaches 128 in fewer than 1 % of the elements -- which is what is asserted
    there instead: the limit of an order-free bound, stated rather than skipped.  The exact GPU tests catch a
    double rounding at any K."""
    a, b, _, prev, want, abs_sum = operands(dtype, K)
    want_p = want + prev.double()
    bnd = bound(want_p, abs_sum, K, dtype, prev.double().abs())
    twice = round16(round16(want, dtype) + prev.double(), dtype)
    nbad = int(((twice - want_p).abs() > bnd).sum())
    print(f"double rounding, K {K}: {nbad} of {want.numel()} elements flagged")
    worst_possible = half_ulp(want, dtype) + 2 * half_ulp(want_p, dtype)   # 2: the once-rounded sum may cross a binade
    could_show = float((worst_possible > bnd).double().mean())             # share of elements that could be flagged
    print(f"double rounding, K {K}: {100 * could_show:.2f} % of elements could exceed their bound")
    if dtype == F16 and K == 1152:
        assert could_show < 0.01
    else:
        assert could_show > 0.5 and nbad >= 1
    assert flagged(round16(want_p, dtype), want_p, bnd) == 0.0


def test_report_rejects_nan_and_out_of_bound():
    want = torch.ones(4, 4, dtype=F64)
    bnd = half_ulp(want, BF16)
    assert report("exact", want.to(BF16), want, bnd) == 0.0
    for bad in (float("nan"), 1.0 + 2.0 ** -7):
        got = want.clone()
        got[2, 1] = bad
        with pytest.raises(AssertionError, match="1 of 16 elements"):
            report("planted", got, want, bnd)


# ------------------------------------------------------------------------------------- generators
@FORMATS
def test_ints_exact_in_any_order(dtype):
    g = gen(7)
    K = 2560                                               # the longest K of the exact GPU tests
    a, b = ints(g, (64, K), dtype), ints(g, (48, K), dtype)
    bias, prev = ints(g, (48,), dtype, -8, 8), ints(g, (64, 48), dtype, -8, 8)
    assert set(a.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert K * 2 * 2 + 8 + 8 < EXACT_LIMIT
    want, abs_sum = product64(a, b, NT)
    assert float(abs_sum.max()) + 16 < EXACT_LIMIT
    fwd = torch.zeros(64, 48, dtype=F32)
    rev = torch.zeros(64, 48, dtype=F32)
    for k0 in range(0, K, 64):
        fwd += a[:, k0:k0 + 64].float() @ b[:, k0:k0 + 64].float().t()
        k1 = K - 64 - k0
        rev += a[:, k1:k1 + 64].float() @ b[:, k1:k1 + 64].float().t()
    assert torch.equal(fwd.double(), want) and torch.equal(rev.double(), want)
    full = want + bias.double() + prev.double()
    assert torch.equal((fwd + bias.float() + prev.float()).to(dtype), full.to(dtype))
    assert torch.equal(full.to(dtype).double(), round16(full, dtype))      # torch's one rounding is the nearest


@FORMATS
@pytest.mark.parametrize("layout", [NT, TN])
def test_one_hot_probe(dtype, layout):
    Mo, No, K = 96, 80, 320
    a, b, want = one_hot_probe(Mo, No, K, dtype, layout)
    assert a.dtype == dtype and b.dtype == dtype
    assert a.shape == ((Mo, K) if layout == NT else (K, Mo)) and b.shape == ((No, K) if layout == NT else (K, No))
    amk = a if layout == NT else a.t()
    bnk = b if layout == NT else b.t()
    assert torch.equal(amk.double().sum(1), torch.ones(Mo, dtype=F64))                 # exactly one 1 per row
    assert torch.equal(amk.double().argmax(1), one_hot_k(Mo, K))
    prod, _ = product64(a, b, layout)
    assert torch.equal(prod, want.double())
    assert torch.equal(want.double(), bnk.double()[:, one_hot_k(Mo, K)].t())
    assert int(bnk.double().abs().max()) <= 125
    for k0 in range(0, K - 50, 17):                                                    # distinct within 50
        win = bnk[:, k0:k0 + 50].double()
        assert all(len(set(row.tolist())) == 50 for row in win[:8])
    # a product read from the neighbouring k is named
    wrong = want.clone().double()
    km = int(one_hot_k(Mo, K)[3])
    wrong[3, 5] = float(bnk[5, km + 1])
    msg = one_hot_blame(wrong, want, K)
    assert "out[3, 5]" in msg and f"k = {km}]" in msg and str(km + 1) in msg
    assert one_hot_blame(want.double(), want, K) == "exact"


@FORMATS
def test_poisoned_view(dtype):
    vals = torch.arange(3 * 40 * 24).reshape(3, 40, 24).remainder(7).to(dtype)
    for v in (vals[0], vals):
        for rows in (16, (0, 8)):
            view, buf = poisoned_view(v, rows, 64)
            assert torch.equal(view, v) and view.data_ptr() % 16 == 0 and view.stride(-2) % 8 == 0
            assert view.stride(-2) >= 24 + 128
            assert int(torch.isnan(buf).sum()) == buf.numel() - v.numel()
            if v.dim() == 3:
                assert view.stride(0) != view.shape[1] * view.stride(1)
