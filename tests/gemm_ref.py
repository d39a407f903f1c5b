"""Shared helpers of the exact and float64-bounded GEMM tests (tests/test_gemm_rs_exact_gpu.py,
tests/test_gemm_tn_exact_gpu.py; checked themselves in tests/test_gemm_ref_cpu.py).  Plain torch on whatever
device the inputs live on: no extension, no dltb import.

    product64       the float64 product of 16-bit operands and the float64 sum of its terms' magnitudes
    bound           per-element error bound of an fp32-accumulated product rounded once to 16 bits
    ints            small-integer operands (every fp32 sum exact in any order)
    poisoned_view   an operand inside a larger NaN-filled buffer: a read outside the view shows in the result
    one_hot_probe   operands whose product names, per output element, the k that was read
    report          every element inside its bound; prints the worst error / bound ratio

The bound is

    half_ulp(want)  +  MARGIN * (K + 2) * U * (abs_sum + extra_abs)         U = 2^-24, MARGIN = 2

The first term is the one final rounding to the 16-bit format.  The second is the standard bound of an fp32
sum of K exact products (a 16-bit x 16-bit product is exact in fp32) plus up to two more fp32 operations of the
epilogue (bias, accumulate onto the old value, or the multiply by aux), taken on the magnitudes that are added:
it holds for ANY summation order, so it needs no knowledge of how the MFMA and the k-loop order the terms.
It is an ASSUMPTION that each accumulation step inside an MFMA instruction rounds no worse than one fp32
round-to-nearest: nothing in this tree or its toolchain's documents states how v_mfma_f32_*_bf16 / _f16 round
their internal sums.  MARGIN = 2 is the one allowance on it, the same as tests/test_rowwise_gpu.py.  The
exact-integer tests do not depend on the assumption (no sum rounds).

The bound is useful up to K of about a thousand.  tests/test_gemm_ref_cpu.py shows that at K <= 1152 it
accepts fp32 products in two summation orders and rejects a dropped k-step, a dropped single term, a bias
on the wrong column group and a double rounding; at K = 4096 it is ten or more half-ulps wide and would pass
a dropped term in most elements, so the GPU tests that use it stay at K <= 1152.
"""
import torch

from rowwise_ref import half_ulp, round16  # noqa: F401  (re-exported)

F64 = torch.float64
U = 2.0 ** -24          # one fp32 rounding, relative
MARGIN = 2.0            # on the fp32 part (see the module docstring)
EXACT_LIMIT = 2 ** 24   # integers below it are exact in fp32

NT, TN = "nt", "tn"


def product64(a, b, layout):
    """(want, abs_sum) in float64.  ``nt``: a [M, K], b [N, K] -> a b^T.  ``tn``: a [(batch,) K, M],
    b [(batch,) K, N] -> a^T b per batch.  abs_sum = |a| |b| in the same layout: the sum of the magnitudes
    of the K terms of each output element."""
    a, b = a.double(), b.double()
    if layout == NT:
        assert a.dim() == 2 and b.dim() == 2 and a.shape[1] == b.shape[1]
        return a @ b.t(), a.abs() @ b.abs().t()
    assert layout == TN and a.dim() == b.dim() and a.shape[-2] == b.shape[-2]
    at = a.transpose(-1, -2)
    return at @ b, at.abs() @ b.abs()


def bound(want, abs_sum, K, dtype, extra_abs=0.0):
    """Largest accepted |got - want| per element: see the module docstring.  ``extra_abs``: the magnitudes the
    epilogue adds (|bias|, |prev|), broadcastable to ``want``."""
    extra = torch.as_tensor(extra_abs, dtype=F64, device=want.device)
    return half_ulp(want, dtype) + MARGIN * (K + 2) * U * (abs_sum.double() + extra)


def ints(gen, shape, dtype, lo=-2, hi=2):
    """Uniform integers in [lo, hi] as ``dtype`` on the generator's device.  The caller asserts that
    K * max(|lo|, |hi|)^2 plus what its epilogue adds stays below EXACT_LIMIT: then every fp32 sum is exact
    in any order and the only rounding is the final one to 16 bits."""
    t = torch.randint(lo, hi + 1, tuple(shape), generator=gen, device=gen.device)
    out = t.to(dtype)
    assert torch.equal(out.to(torch.int64), t), "integers not exact in the format"
    return out


def poisoned_view(values, pad_rows, pad_cols):
    """(view, buffer): ``values`` [(batch,) R, C] copied into the middle of a NaN-filled buffer
    [(batch,) before + R + after, pad_cols + C + pad_cols (rounded up to 8 elements)]; ``pad_rows`` is one
    number for both sides or (before, after).  The view's row stride is a multiple of 8 elements and its
    base 16-byte aligned, and a batched view's batch stride differs from rows x row stride, so a kernel
    reading a row, a column or a batch outside its operand multiplies NaNs."""
    before, after = (pad_rows, pad_rows) if isinstance(pad_rows, int) else pad_rows
    assert pad_cols % 8 == 0 and values.dim() in (2, 3) and values.element_size() == 2
    R, C = values.shape[-2:]
    width = (C + 2 * pad_cols + 7) // 8 * 8
    buf = torch.full(tuple(values.shape[:-2]) + (before + R + after, width), float("nan"),
                     dtype=values.dtype, device=values.device)
    view = buf[..., before:before + R, pad_cols:pad_cols + C]
    view.copy_(values)
    assert view.stride(-1) == 1 and view.stride(-2) % 8 == 0 and view.data_ptr() % 16 == 0
    assert values.dim() == 2 or (view.stride(0) % 8 == 0 and (before + after == 0 or view.stride(0) != R * view.stride(1)))
    return view, buf


def one_hot_k(M, K, device=None):
    """k(m) = (37 m + 11) % K: the one k at which row m of the probe's A is 1."""
    return (37 * torch.arange(M, device=device) + 11) % K


def one_hot_probe(M, N, K, dtype, layout, device=None):
    """(a, b, want): A has exactly one 1 per output row m, at k(m); B[n, k] = ((3 n + 5 k) % 251) - 125, exact
    in both formats and distinct along k within any window of 50.  The product is want[m, n] = B[n, k(m)]
    exactly (int64): an element that differs was formed from another k, see ``one_hot_blame``."""
    km = one_hot_k(M, K, device)
    n = torch.arange(N, device=device)
    k = torch.arange(K, device=device)
    bnk = (3 * n[:, None] + 5 * k[None, :]) % 251 - 125                     # [N, K]
    amk = torch.zeros(M, K, dtype=dtype, device=device)
    amk[torch.arange(M, device=device), km] = 1
    want = bnk[:, km].t().contiguous()                                      # [M, N]
    b16 = bnk.to(dtype)
    assert torch.equal(b16.to(torch.int64), bnk)
    if layout == NT:
        return amk, b16, want
    assert layout == TN
    return amk.t().contiguous(), b16.t().contiguous(), want


def one_hot_blame(got, want, K):
    """Failure message of a one-hot probe: the first wrong element, the k it should have read and the k (or
    ks) near it whose B value it holds instead."""
    bad = (got.double() != want.double()).nonzero()
    if bad.numel() == 0:
        return "exact"
    m, n = (int(v) for v in bad[0])
    km = int((37 * m + 11) % K)
    g = float(got[m, n])
    ks = [k for k in range(K) if ((3 * n + 5 * k) % 251) - 125 == g]
    near = sorted(ks, key=lambda k: abs(k - km))[:4]
    return (f"{bad.shape[0]} of {got.numel()} elements wrong; first out[{m}, {n}] = {g} instead of "
            f"{float(want[m, n])} = B[n, k = {km}]; that value is B[n, k] at k = {near if near else 'no k (a sum?)'}")


def report(what, got, want, bnd):
    """Every element of ``got`` within ``bnd`` of the float64 ``want``; prints and returns the worst
    error / bound ratio."""
    got, want = got.double(), want.double()
    bnd = torch.as_tensor(bnd, dtype=F64, device=got.device).expand_as(want)
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} against {tuple(want.shape)}"
    err = (got - want).abs()
    ok = (err <= bnd) | (torch.isinf(bnd) & ~torch.isnan(got))             # want rounds to inf: any non-nan
    fin = torch.isfinite(bnd) & (bnd > 0)
    ratio = torch.where(fin, err / bnd, torch.zeros_like(err))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax()) if ratio.numel() else 0
    worst = float(ratio.flatten()[i]) if ratio.numel() else 0.0
    print(f"{what}: worst error/bound {worst:.3f} (error {float(err.flatten()[i]):.3e}, "
          f"bound {float(bnd.flatten()[i]):.3e}, {got.numel()} elements)")
    nbad = int((~ok).sum())
    assert nbad == 0, f"{what}: {nbad} of {got.numel()} elements outside their bound, worst error/bound {worst:.3f}"
    return worst


def flagged(got, want, bnd):
    """Share of elements of ``got`` outside ``bnd`` of ``want`` (what ``report`` would reject)."""
    bad = ~((got.double() - want.double()).abs() <= bnd)
    return float(bad.double().mean())
