"""The row-wise and elementwise kernels (csrc/norm.hip, csrc/elementwise.hip, csrc/embedding.hip,
csrc/xent.hip), kernel by kernel and in both 16-bit formats, against the float64 references of
tests/rowwise_ref.py (themselves checked against torch in tests/test_rowwise_ref_cpu.py).

No tolerance is taken from what a kernel returns.  Every bound is derived where it is used, from the
kernel's source text, as

    half_ulp(want)                         the final rounding to the 16-bit format (absent for fp32 outputs)
  + MARGIN * c * U * sum|terms|            the fp32 evaluation: c roundings of U = 2^-24 relative each on the
                                           magnitudes that are added (not on the result, which may cancel)
  + H * |value|                            per hardware approximation (__expf, __logf, rsqrtf, v_rcp_f32)

MARGIN = 2 is the one allowance on the fp32 part.  H = 2^-20 is an ASSUMPTION: no accuracy figure for these
instructions is documented in this tree or its toolchain's documents, and nobody here has measured one.  It
is 256 times below fp16's half ulp (2^-12 relative), so wherever an approximated value feeds a 16-bit output
the bound does not depend on it; it matters for the fp32 outputs (rstd, loss, lse) only.  The erf polynomial
gets the 1.5e-7 absolute error csrc/common.h claims for it.  Every element must be inside its bound, and
every test prints its worst error / bound ratio."""
import math

import pytest
import torch

import dltb  # noqa: F401
from dltb.ops._ext import ext
from dltb.ops.rng import StepSeed, keep_mask_2d, site_seed          # the specification of the dropout hash

from rowwise_ref import (embed64, embed_dwpe64, embed_dwte64, gelu64, gelu_grad64, half_ulp, layernorm64,
                         norm_bwd64, rmsnorm64, rope64, silu_mul64, silu_mul_grad64, xent64)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
FORMATS = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])

U = 2.0 ** -24          # one fp32 rounding, relative
H = 2.0 ** -20          # one hardware approximation, relative (assumed, see the module docstring)
MARGIN = 2.0            # on the fp32 part
ERF_ABS = 1.5e-7        # csrc/common.h: Abramowitz & Stegun 7.1.26
# elementwise grids stop at 2048 blocks of 256 lanes: this many 16-byte vectors wrap the grid-stride loop
# and leave 3 vectors for the last pass
WRAP_VECS = 256 * 2048 + 3


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def gen(seed):
    return torch.Generator(DEV).manual_seed(seed)


def randn(g, *shape, dtype=F32, scale=1.0, shift=0.0):
    return (torch.randn(*shape, device=DEV, generator=g) * scale + shift).to(dtype)


def report(what, got, want, bound):
    """Every element of ``got`` within ``bound`` of the float64 ``want``; prints the worst error / bound."""
    got, want = got.double(), want.double()
    bound = torch.as_tensor(bound, dtype=F64, device=got.device).expand_as(want)
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} against {tuple(want.shape)}"
    err = (got - want).abs()
    ok = (err <= bound) | (torch.isinf(bound) & ~torch.isnan(got))        # want rounds to inf: any non-nan
    fin = torch.isfinite(bound) & (bound > 0)
    ratio = torch.where(fin, err / bound, torch.zeros_like(err))
    i = int(ratio.argmax()) if ratio.numel() else 0
    worst = float(ratio.flatten()[i]) if ratio.numel() else 0.0
    print(f"{what}: worst error/bound {worst:.3f} (error {float(err.flatten()[i]):.3e}, "
          f"bound {float(bound.flatten()[i]):.3e}, {got.numel()} elements)")
    nbad = int((~ok).sum())
    assert nbad == 0, f"{what}: {nbad} of {got.numel()} elements outside their bound, worst error/bound {worst:.3f}"
    return worst


def step_seed(v):
    s = StepSeed(v, 0, device=DEV)
    s.next()
    return s


def keep_of(sd, site, rows, cols, p):
    return keep_mask_2d(site_seed(int(sd.value), site), rows, cols, p, device=DEV)


def all_finite(dtype):
    """Every finite bit pattern of the format, padded with zeros to a multiple of 8 (65 280 / 63 488)."""
    v = torch.arange(-32768, 32768, dtype=torch.int32, device=DEV).to(torch.int16).view(dtype)
    v = v[torch.isfinite(v)]
    assert v.numel() == {BF16: 65280, F16: 63488}[dtype] and v.numel() % 8 == 0
    return v.contiguous()


# ============================================================================ norm_fwd / norm_apply
NORM_WIDTHS = [8, 520, 768, 2560, 3584, 4096]     # 1, 2 (one lane in the second), 2, 5 -> 6, 7 -> 8, 8 register passes


def lane_terms(d):
    """Elements one lane adds up in a row reduction: 8 per register pass."""
    return 8 * ((d // 8 + 63) // 64)


def norm_rows(dtype, rms, N, d, seed):
    """Row 0 (and every row past 4) zero-mean randn; 1: 30 + 0.5 randn (a one-pass E[x^2] - mean^2 variance loses
    it); 2: constant (rstd = 1 / sqrt(eps)); 3: all zero for RMSNorm; 4: scaled to 2^14 in fp16 (the squares
    reach 2^28: they must be formed and summed in fp32).  A single row is the offset family."""
    g = gen(seed)
    x = torch.randn(N, d, device=DEV, generator=g)
    if N == 1:
        x = 30.0 + 0.5 * x
    if N > 4:
        x[1] = 30.0 + 0.5 * x[1]
        x[2] = 3.0
        if rms:
            x[3] = 0.0
        if dtype == F16:
            x[4] = x[4] * (2.0 ** 14 / float(x[4].abs().max()))
    w = randn(g, d, scale=0.5, shift=1.0).to(dtype)
    b = randn(g, d, scale=0.1).to(dtype)
    r = randn(g, N, d, scale=0.5).to(dtype)
    return x.to(dtype), w, b, r


def check_norm_fwd(what, dtype, rms, s_k, w, b, eps, y, mean, rstd):
    """y, mean, rstd of the kernel against the reference on the stored stream ``s_k`` (a 16-bit tensor)."""
    N, d = s_k.shape
    n = lane_terms(d)
    if rms:
        want_y, _, want_rstd, s = rmsnorm64(s_k, w, eps)
        dmean = torch.zeros(N, dtype=F64, device=DEV)
        var = (s * s).mean(-1)
        c = s
    else:
        want_y, want_mean, want_rstd, s = layernorm64(s_k, w, b, eps)
        # mean = wave_sum(sum) / d: n sequential adds per lane, 6 butterfly rounds, 1 divide on sum|s| / d
        dmean = (n + 7) * U * s.abs().mean(-1)
        report(f"{what} mean", mean, want_mean, MARGIN * dmean)
        c = s - want_mean[:, None]
        var = (c * c).mean(-1)
    # var = wave_sum(sum (v - mean)^2) / d.  The kernel's mean error enters as exactly dmean^2 (sum (v - m')^2 / d
    # = var + (m' - m)^2); per term 1 rounding of v - mean (2 on the square) and 1 of the square itself (an fma
    # with the running sum at best), then n + 6 adds and the divide: (n + 10) U var.  var + eps: 1 rounding.
    # rstd = rsqrtf(.) halves the relative error and adds H.
    dvar = dmean ** 2 * MARGIN ** 2 + MARGIN * ((n + 10) * U * var + U * (var + eps))
    rho32 = 0.5 * dvar / (var + eps)                               # relative, margin included
    report(f"{what} rstd", rstd, want_rstd, want_rstd * (rho32 + H))
    # y = (v - mean) * rstd * w + b: the first factor carries dmean + U |c|, the second rho; 2 multiplies and
    # the add (U on |t| + |b|, the magnitudes added).  RMSNorm: no mean, no add.
    t = (c * want_rstd[:, None] * w.double()).abs()
    e32 = (want_rstd[:, None] * w.double().abs()) * (MARGIN * dmean[:, None]) + t * rho32[:, None] + MARGIN * U * (
        3 * t + (0 if rms else t + b.double().abs()))
    report(f"{what} y", y, want_y, half_ulp(want_y, dtype) + e32 + t * H)


@FORMATS
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("N", [1, 5, 301])
@pytest.mark.parametrize("d", NORM_WIDTHS)
def test_norm_fwd_and_apply(dtype, rms, N, d):
    """norm_fwd's y, s, mean and rstd against float64 without a residual, with one (p = 0) and with a dropped
    one (p = 0.1), at eps = 1e-5 and 1e-2 (where a missing eps shows on ordinary rows); norm_apply bitwise its y."""
    C = ext()
    x, w, b, r = norm_rows(dtype, rms, N, d, 1000 * d + N)
    bb = None if rms else b
    sd = step_seed(d + N)
    for eps in (1e-5, 1e-2):
        for p in (None, 0.0, 0.1):
            what = f"norm_fwd {'rms' if rms else 'ln'} {dtype} N={N} d={d} eps={eps} p={p}"
            s, y, mean, rstd = C.norm_fwd(x, None if p is None else r, w, bb, eps, rms, p or 0.0, sd.device_tensor, 3)
            if p is None:
                s_k = x
            else:
                keep = keep_of(sd, 3, N, d, p) if p else None
                want_s = x.double() + (torch.where(keep, r.double() / (1 - p), 0.0) if p else r.double())
                # s = x + r * scale: the fp32 scale 1 / (1 - p) (U), the multiply (U), the add (U on |x| + |r'|)
                rr = (want_s - x.double()).abs()
                report(f"{what} s", s, want_s, half_ulp(want_s, dtype) + MARGIN * U * (2 * rr + x.double().abs() + rr))
                if p:
                    assert same_bits(s[~keep], x[~keep]), "a dropped residual element leaves x as it is"
                s_k = s
            check_norm_fwd(what, dtype, rms, s_k, w, bb, eps, y, None if rms else mean, rstd)
            again = C.norm_fwd(x, None if p is None else r, w, bb, eps, rms, p or 0.0, sd.device_tensor, 3)
            assert same_bits(again[1], y) and same_bits(again[3], rstd), f"{what}: repeated call"
            y2 = C.norm_apply(s_k, w, bb, None if rms else mean, rstd, rms)
            assert same_bits(y2, y), f"{what}: norm_apply is bitwise norm_fwd's y"


@FORMATS
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
def test_norm_apply_strided_and_wrapped(dtype, rms):
    C = ext()
    # into a column block of a wider buffer: the other columns keep their bits
    N, d, wide, off = 37, 520, 1600, 528
    x, w, b, _ = norm_rows(dtype, rms, N, d, 5)
    bb = None if rms else b
    _, y, mean, rstd = C.norm_fwd(x, None, w, bb, 1e-5, rms, 0.0, None, 0)
    buf = randn(gen(6), N, wide).to(dtype)
    before = buf.clone()
    view = buf[:, off:off + d]
    assert not view.is_contiguous()
    C.norm_apply(x, w, bb, None if rms else mean, rstd, rms, view)
    assert same_bits(view.contiguous(), y)
    inside = torch.zeros(wide, dtype=torch.bool, device=DEV)
    inside[off:off + d] = True
    assert same_bits(buf[:, ~inside], before[:, ~inside]), "columns outside the block were written"
    # past the grid-stride wrap: N d / 8 = 256 * 2048 + 3 vectors
    N, d = WRAP_VECS, 8
    x = randn(gen(7), N, d).to(dtype)
    w, b = randn(gen(8), d, shift=1.0).to(dtype), randn(gen(9), d).to(dtype)
    bb = None if rms else b
    _, y, mean, rstd = C.norm_fwd(x, None, w, bb, 1e-5, rms, 0.0, None, 0)
    assert same_bits(C.norm_apply(x, w, bb, None if rms else mean, rstd, rms), y)
    check_norm_fwd(f"norm_fwd wrap {dtype} rms={rms}", dtype, rms, x[-1024:], w, bb, 1e-5, y[-1024:],
                   None if rms else mean[-1024:], rstd[-1024:])


# =========================================================================================== norm backward
def bwd_inputs(dtype, rms, N, d, seed):
    g = gen(seed)
    s = randn(g, N, d, shift=0.25).to(dtype)
    dy, dres = randn(g, N, d).to(dtype), randn(g, N, d).to(dtype)
    w = randn(g, d, scale=0.5, shift=1.0).to(dtype)
    if rms:
        _, mean, rstd, _ = rmsnorm64(s, w, 1e-5)
    else:
        _, mean, rstd, _ = layernorm64(s, w, w, 1e-5)
    # the statistics as the forward hands them over: fp32
    return dy, s, w, dres, (None if rms else mean.float()), rstd.float()


def dx_bound(dtype, dy, s, w, mean, rstd, dres, want_dx):
    """dx = rstd * (g - s1 - xh * s2) + dres with g = dy * w, xh = (s - mean) * rstd, s1 = wave_sum(g) / d,
    s2 = wave_sum(g * xh) / d (both kernels):
      s1: n adds per lane, 6 butterfly rounds, the divide, 1 rounding in g: (n + 8) U mean|g|
      s2: as s1 plus 2 roundings in xh and 1 in the product:              (n + 11) U mean|g xh|
      inner sum, T = |g| + |s1| + |xh s2| the magnitudes added: 1 (g) + 3 (xh, xh * s2) + 2 subtractions -> 6 U T,
      plus |xh| ds2 + ds1; times rstd (U); + dres (U on the magnitudes added)."""
    d = dy.shape[-1]
    n = lane_terms(d)
    rs = rstd.double()[:, None]
    xh = ((s.double() - (0.0 if mean is None else mean.double()[:, None])) * rs)
    g = dy.double() * w.double()
    s1 = torch.zeros_like(rs) if mean is None else g.mean(-1, keepdim=True)
    s2 = (g * xh).mean(-1, keepdim=True)
    ds1 = (n + 8) * U * g.abs().mean(-1, keepdim=True) * (mean is not None)
    ds2 = (n + 11) * U * (g * xh).abs().mean(-1, keepdim=True)
    T = g.abs() + s1.abs() + (xh * s2).abs()
    e32 = rs * (ds1 + xh.abs() * ds2 + 6 * U * T) + U * (rs * T + dres.double().abs())
    return half_ulp(want_dx, dtype) + MARGIN * e32


def colsum_bound(dtype, want, mags, chain):
    """A column sum stored in 16 bits: ``chain`` fp32 roundings on the magnitudes summed, then the final rounding."""
    return half_ulp(want, dtype) + MARGIN * chain * U * mags


@FORMATS
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("N", [5, 301])
@pytest.mark.parametrize("d", NORM_WIDTHS)
def test_norm_bwd_split(dtype, rms, N, d):
    """norm_bwd (= norm_bwd_dx + norm_bwd_dgamma): dx, and dgamma / dbeta overwriting and accumulating."""
    C = ext()
    dy, s, w, dres, mean, rstd = bwd_inputs(dtype, rms, N, d, 77 * d + N)
    want_dx, want_gw, want_gb, _ = norm_bwd64(dy, s, w, mean, rstd, dres)
    xh = (s.double() - (0.0 if rms else mean.double()[:, None])) * rstd.double()[:, None]
    # norm_dgamma_kernel: P = clamp(N / 32, 1, 128) row slices of rps rows, a lane takes every 4th row of its slice,
    # 3 adds over the 4 phases; norm_colreduce_kernel: every 16th partial, 16 adds, 1 more to accumulate.
    # Each dgamma term dy * (s - mean) * rstd carries 3 roundings.
    P = min(max(N // 32, 1), 128)
    rps = -(-N // P)
    chain = -(-rps // 4) + 3 + -(-P // 16) + 16 + 1 + 3
    for accumulate in (False, True):
        what = f"norm_bwd split {'rms' if rms else 'ln'} {dtype} N={N} d={d} acc={accumulate}"
        gw = randn(gen(1), d).to(dtype)
        gb = randn(gen(2), d).to(dtype)
        prev_w, prev_b = (gw.double(), gb.double()) if accumulate else (torch.zeros(d, dtype=F64, device=DEV),) * 2
        dx = C.norm_bwd(dy, s, w, mean, rstd, dres, gw, None if rms else gb, accumulate, rms)
        report(f"{what} dx", dx, want_dx, dx_bound(dtype, dy, s, w, mean, rstd, dres, want_dx))
        report(f"{what} dgamma", gw, want_gw + prev_w,
               colsum_bound(dtype, want_gw + prev_w, (dy.double() * xh).abs().sum(0) + prev_w.abs(), chain))
        if not rms:
            report(f"{what} dbeta", gb, want_gb + prev_b,
                   colsum_bound(dtype, want_gb + prev_b, dy.double().abs().sum(0) + prev_b.abs(), chain))
    # the two halves on their own give the same bits
    dx2 = C.norm_bwd_dx(dy, s, w, mean, rstd, dres, rms)
    assert same_bits(dx2, dx)
    gw2, gb2 = randn(gen(1), d).to(dtype), randn(gen(2), d).to(dtype)
    C.norm_bwd_dgamma(dy, s, mean, rstd, gw2, None if rms else gb2, True, rms)
    assert same_bits(gw2, gw) and (rms or same_bits(gb2, gb))


# LayerNorm's fold of the K x 8 x d fp32 images (launch_bwd_fused): one barrier while K * 8 * d * 4 <= 128 KiB, with
# hipFuncSetAttribute above 64 KiB, else one image at a time:
#   K = 2 (no dx sum): d = 2048 is exactly 128 KiB, one barrier + attribute;  d = 1024: 64 KiB, one barrier
#   K = 3 (dx sum):    d = 1024 is 96 KiB, one barrier + attribute;            d = 2048: 192 KiB, the serial fold
# RMSNorm has K = 1 / 2: d = 2048 with the dx sum is 128 KiB again.
@FORMATS
@pytest.mark.parametrize("dx_sum", [False, True], ids=["", "dxsum"])
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("N", [7, 64, 4099])
@pytest.mark.parametrize("d", [64, 520, 1024, 2048])
def test_norm_bwd_fused(dtype, rms, N, d, dx_sum):
    """norm_bwd_fused: dx, its fp32 column partials (dgamma, dbeta, the stored dx), and those partials summed
    into 16-bit slots (overwrite / accumulate onto a non-zero slot).  N = 4099: two rows per wave, an odd rest,
    and waves whose first row is past the end."""
    C = ext()
    dy, s, w, dres, mean, rstd = bwd_inputs(dtype, rms, N, d, 31 * d + N)
    want_dx, want_gw, want_gb, _ = norm_bwd64(dy, s, w, mean, rstd, dres)
    xh = (s.double() - (0.0 if rms else mean.double()[:, None])) * rstd.double()[:, None]
    what = f"norm_bwd_fused {'rms' if rms else 'ln'} {dtype} N={N} d={d} dxsum={dx_sum}"
    dx, part = C.norm_bwd_fused(dy, s, w, mean, rstd, dres, rms, dx_sum)
    report(f"{what} dx", dx, want_dx, dx_bound(dtype, dy, s, w, mean, rstd, dres, want_dx))
    rpw = max(N // (8 * 256), 1)
    nblk = -(-N // (8 * rpw))
    K = (1 if rms else 2) + int(dx_sum)
    assert tuple(part.shape) == (K, nblk, d) and part.dtype == F32
    # a wave adds its rpw rows (rpw roundings, 2 more in the dgamma term dy * xh with xh 2 roundings itself -> 3),
    # the fold adds 8 waves; summing the blocks in float64 here adds nothing
    wants = [(want_gw, (dy.double() * xh).abs().sum(0), 3, "dgamma")]
    if not rms:
        wants.append((want_gb, dy.double().abs().sum(0), 0, "dbeta"))
    if dx_sum:
        wants.append((dx.double().sum(0), dx.double().abs().sum(0), 0, "dx column sum"))       # of the stored dx
    outs0 = [randn(gen(3 + k), d).to(dtype) for k in range(K)]
    for accumulate in (False, True):
        outs = [o.clone() for o in outs0]
        C.colreduce_multi([part[k] for k in range(K)], outs, [accumulate] * K)
        for k, (want, mags, extra, name) in enumerate(wants):
            if not accumulate:
                report(f"{what} {name} partials", part[k].double().sum(0), want, MARGIN * (rpw + 8 + extra) * U * mags)
            # the reduction to the slot: at most one add per block partial in whatever order, 1 for the old value
            prev = outs0[k].double() if accumulate else torch.zeros_like(want)
            report(f"{what} {name} slot acc={accumulate}", outs[k], want + prev,
                   colsum_bound(dtype, want + prev, mags + prev.abs(), rpw + 8 + extra + nblk + 1))
    dx2, part2 = C.norm_bwd_fused(dy, s, w, mean, rstd, dres, rms, dx_sum)
    assert same_bits(dx2, dx) and same_bits(part2, part), "repeated call"


@FORMATS
@pytest.mark.parametrize("N,d", [(301, 768), (64, 1024)])
@pytest.mark.parametrize("p", [0.1, 0.0])
def test_norm_bwd_fused_dropout_backward(dtype, N, d, p):
    """XS == 2 in both formats: dm is documented as bitwise the dropout kernel's on the stored dx, and is held to
    that.  dx is NOT bitwise the XS == 0 instantiation's: the two are compiled apart and contract their fp32
    expressions differently, which flips a rounding tie of the 16-bit store in about one element of 65 000 in
    fp16 (tests/test_kernels_gpu.py::test_norm_bwd_fused_dropout compares them in bf16, where its shapes happen
    to agree).  So dx, and the dgamma / dbeta partials, are held to the float64 bounds of the other variants."""
    C = ext()
    dy, s, w, dres, mean, rstd = bwd_inputs(dtype, False, N, d, 13 * d + N)
    sd = step_seed(9)
    dm = torch.empty_like(s)
    dx, part = C.norm_bwd_fused(dy, s, w, mean, rstd, dres, False, False, None, dm, p, sd.device_tensor if p else None, 7)
    what = f"norm_bwd_fused dm {dtype} N={N} d={d} p={p}"
    want_dx, want_gw, want_gb, _ = norm_bwd64(dy, s, w, mean, rstd, dres)
    report(f"{what} dx", dx, want_dx, dx_bound(dtype, dy, s, w, mean, rstd, dres, want_dx))
    xh = (s.double() - mean.double()[:, None]) * rstd.double()[:, None]
    rpw = max(N // (8 * 256), 1)
    report(f"{what} dgamma partials", part[0].double().sum(0), want_gw, MARGIN * (rpw + 11) * U * (dy.double() * xh).abs().sum(0))
    report(f"{what} dbeta partials", part[1].double().sum(0), want_gb, MARGIN * (rpw + 8) * U * dy.double().abs().sum(0))
    assert same_bits(dm, C.dropout(None, dx, p, sd.device_tensor if p else None, 7))
    if p:
        keep = keep_of(sd, 7, N, d, p)
        assert not bool(bits(dm[~keep]).any()) and bool((dm[keep] != 0).any())
    dx2, part2 = C.norm_bwd_fused(dy, s, w, mean, rstd, dres, False, False, None, torch.empty_like(s), p,
                                  sd.device_tensor if p else None, 7)
    assert same_bits(dx2, dx) and same_bits(part2, part), "repeated call"
    report(f"norm_bwd_fused dm column sum {dtype} N={N} d={d} p={p}", part[2].double().sum(0), dm.double().sum(0),
           MARGIN * (rpw + 8) * U * dm.double().abs().sum(0))


@FORMATS
@pytest.mark.parametrize("d", [12, 4104])
def test_norm_backward_rejects_widths_its_kernels_cannot_take(dtype, d):
    """The row-in-registers kernels hold 8 x 64 vectors of 8 elements: every binding that reaches one refuses
    d % 8 != 0 and d > 4096 with norm_fwd's message, before any launch.  norm_bwd_dgamma walks column blocks of
    512 over any width and needs only whole 16-byte vectors: it refuses 12 and takes 4104."""
    C = ext()
    N = 4
    g = gen(d)
    dy, s =randn(g, N, d).to(dtype), randn(g, N, d).to(dtype)
    w, gw, gb = randn(g, d).to(dtype), randn(g, d).to(dtype), randn(g, d).to(dtype)
    mean, rstd = torch.zeros(N, device=DEV), torch.ones(N, device=DEV)
    msg = "norm: d must be a multiple of 8 and <= 4096"
    with pytest.raises(RuntimeError, match=msg):
        C.norm_fwd(s, None, w, gb, 1e-5, False, 0.0, None, 0)
    with pytest.raises(RuntimeError, match=msg):
        C.norm_bwd(dy, s, w, mean, rstd, None, gw, gb, False, False)
    with pytest.raises(RuntimeError, match=msg):
        C.norm_bwd_dx(dy, s, w, mean, rstd, None, False)
    with pytest.raises(RuntimeError, match=msg):
        C.norm_bwd_fused(dy, s, w, mean, rstd, None, False, False)
    gw0, gb0 = gw.clone(), gb.clone()
    if d % 8:
        with pytest.raises(RuntimeError, match="norm: d must be a multiple of 8"):
            C.norm_bwd_dgamma(dy, s, mean, rstd, gw, gb, False, False)
        assert same_bits(gw, gw0) and same_bits(gb, gb0)
    else:
        C.norm_bwd_dgamma(dy, s, mean, rstd, gw, gb, False, False)
        _, want_gw, want_gb, _ = norm_bwd64(dy, s, w, mean, rstd)
        chain = 1 + 3 + 1 + 16 + 3                               # P = 1, 4 rows: see test_norm_bwd_split
        report(f"norm_bwd_dgamma d={d} dgamma", gw, want_gw, colsum_bound(dtype, want_gw, (dy.double() * s.double()).abs().sum(0), chain))
        report(f"norm_bwd_dgamma d={d} dbeta", gb, want_gb, colsum_bound(dtype, want_gb, dy.double().abs().sum(0), chain))


# =================================================================================================== GELU
A_S = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)


def erf_fast_bound(ax):
    """Allowed absolute error of erf_fast (csrc/common.h) at |argument| ``ax`` (float64), the argument's own
    rounding included.  q = p(t) t e is what the kernel subtracts from 1:
       t = rcp(fma(c, ax, 1)): U + H relative, which moves p(t) t by |sum k a_k t^k| (first order)
       e = __expf(-ax * ax):   U ax^2 (the square's rounding, amplified by the exponent) + H
       p: 4 fma, each U on a partial sum below sum |a_k| t^k / t;  p * t * e: 2 U
       y = 1 - q: U (half an ulp of a value below 1)
       the argument x * 0.70710678f: 1 rounding and the constant's own (U / 2), through erf' = 2 / sqrt(pi) e."""
    t = 1.0 / (1.0 + 0.3275911 * ax)
    e = torch.exp(-ax * ax)
    pw = [t ** (k + 1) for k in range(5)]
    pt = sum(a * p for a, p in zip(A_S, pw))
    pabs = sum(abs(a) * p for a, p in zip(A_S, pw))
    sens = sum((k + 1) * a * p for k, (a, p) in enumerate(zip(A_S, pw))).abs()
    e32 = e * (sens * U + 4 * U * pabs + 2 * U * pt + pt * ax * ax * U) + U + 1.5 * U * ax * e * 2.0 / math.sqrt(math.pi)
    eh = e * (sens + pt) * H
    return ERF_ABS + MARGIN * e32 + eh


def gelu_bound(x, want, dtype):
    """g = 0.5 x (1 + erf_fast(x / sqrt 2)): 0.5 x is exact, 1 + erf exact or one rounding (U), the product U."""
    ax = x.double().abs()
    return half_ulp(want, dtype) + 0.5 * ax * erf_fast_bound(ax * math.sqrt(0.5)) + MARGIN * 2 * U * want.abs()


def gelu_grad_bound(x, want, dtype):
    """g' = cdf + x * 0.39894228f * e with erf_fast's own e = exp(-x^2 / 2): the cdf as above; the second term
    2 multiplies (2 U) and e's error (H + U x^2 / 2 + the argument's 1.5 U x^2); the add U on both magnitudes."""
    x = x.double()
    ax = x.abs()
    cdf = 0.5 * torch.special.erfc(-x * math.sqrt(0.5))
    term = ax * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    e32 = term * (2 * U + 2 * U * x * x) + U * (cdf + term)
    return half_ulp(want, dtype) + 0.5 * erf_fast_bound(ax * math.sqrt(0.5)) + term * H + MARGIN * e32


@FORMATS
def test_gelu_every_finite_input(dtype):
    """gelu_fwd, gelu_bwd with dg = 1 (and gelu_fwd_grad's g and g' in bf16) at every finite value of the format."""
    C = ext()
    x = all_finite(dtype)
    want, want_g = gelu64(x), gelu_grad64(x)
    g = C.gelu_fwd(x)
    report(f"gelu_fwd {dtype} exhaustive", g, want, gelu_bound(x, want, dtype))
    df = C.gelu_bwd(torch.ones_like(x).view(-1, 8), x.view(-1, 8), None, False).view(-1)
    report(f"gelu_bwd dg=1 {dtype} exhaustive", df, want_g, gelu_grad_bound(x, want_g, dtype))
    if dtype == BF16:
        g2, gp = C.gelu_fwd_grad(x)
        report("gelu_fwd_grad g bf16 exhaustive", g2, want, gelu_bound(x, want, dtype))
        report("gelu_fwd_grad g' bf16 exhaustive", gp, want_g, gelu_grad_bound(x, want_g, dtype))
        assert same_bits(gp, df), "g' of gelu_fwd_grad and gelu_bwd with dg = 1: the same expression"
    else:
        with pytest.raises(RuntimeError, match="bf16 only"):
            C.gelu_fwd_grad(x)
    assert same_bits(C.gelu_fwd(x), g)


@FORMATS
def test_gelu_past_the_grid_wrap(dtype):
    C = ext()
    x = randn(gen(21), WRAP_VECS * 8, scale=2.0).to(dtype)
    want = gelu64(x)
    report(f"gelu_fwd {dtype} wrap", C.gelu_fwd(x), want, gelu_bound(x, want, dtype))
    if dtype == BF16:
        g2, gp = C.gelu_fwd_grad(x)
        want_g = gelu_grad64(x)
        report("gelu_fwd_grad g bf16 wrap", g2, want, gelu_bound(x, want, dtype))
        report("gelu_fwd_grad g' bf16 wrap", gp, want_g, gelu_grad_bound(x, want_g, dtype))


# colsum_kernel: P = clamp(N / 32, 1, 128) slices of rps = ceil(N / P) rows, a lane adds every 4th row of its
# slice, 3 adds over the phases; colreduce_kernel: every 16th partial, 16 adds, 1 to accumulate.
# (4100, 24): 128 partials of rps = 33 rows, the last slice 4100 - 127 * 33 = -91 rows short -> empty slices too.
def colsum_chain(N):
    P = min(max(N // 32, 1), 128)
    rps = -(-N // P)
    return -(-rps // 4) + 3 + -(-P // 16) + 16 + 1


@FORMATS
@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("N,k", [(5, 8), (301, 520), (4100, 24)])
def test_gelu_bwd_bias_gradient_and_colsum(dtype, N, k, accumulate):
    C = ext()
    g = gen(N + k)
    f, dg = randn(g, N, k, scale=1.5).to(dtype), randn(g, N, k).to(dtype)
    db0 = randn(g, k).to(dtype)
    db = db0.clone()
    df = C.gelu_bwd(dg, f, db, accumulate)
    # df = dg * gelu'(f): gelu' to gelu_grad_bound's error terms (without its final rounding), the product U
    want_df = dg.double() * gelu_grad64(f)
    gb = gelu_grad_bound(f, gelu_grad64(f), dtype) - half_ulp(gelu_grad64(f), dtype)
    report(f"gelu_bwd df {dtype} N={N} k={k}", df, want_df,
           half_ulp(want_df, dtype) + dg.double().abs() * gb + MARGIN * U * want_df.abs())
    prev = db0.double() if accumulate else torch.zeros(k, dtype=F64, device=DEV)
    want = df.double().sum(0) + prev                                     # of the rounded df
    report(f"gelu_bwd db {dtype} N={N} k={k} acc={accumulate}", db, want,
           colsum_bound(dtype, want, df.double().abs().sum(0) + prev.abs(), colsum_chain(N)))
    out = db0.clone()
    C.colsum_into(dg, out, accumulate)
    want = dg.double().sum(0) + prev
    report(f"colsum_into {dtype} N={N} k={k} acc={accumulate}", out, want,
           colsum_bound(dtype, want, dg.double().abs().sum(0) + prev.abs(), colsum_chain(N)))


# ================================================================================================= SwiGLU
def swiglu_bounds(dtype, g, u, d):
    """s = 1 / (1 + __expf(-g)): the exponential H + U |g| relative (its argument is scaled in fp32), damped by
    1 - s in s; the add and the divide U each -> rho = (1 - s) (H + U |g|) + 2 U.  Below fp32's normal range
    (s < 2^-126: denormal, or 0 once __expf(-g) is inf at g < -88.7, where s < 2^-128) s is off by up to 2^-126.
       h  = g * s * u:  rho + 2 U                            du = d * (g * s): rho + 2 U
       dg = (d * u * s) * (1 + g * (1 - s)) = A * B:  A rho + 2 U;  1 - s is off by s rho + U (1 - s) absolute,
            g (1 - s) one more U, the add U on 1 + |g| (1 - s) (B crosses zero near g = -1.278);  A * B: U."""
    g, u, d = g.double(), u.double(), d.double()
    s, oms = torch.sigmoid(g), torch.sigmoid(-g)
    floor = 2.0 ** -126
    out = []

    def both(f):
        return f((1 - s) * H, 0.0) + MARGIN * f((1 - s) * U * g.abs() + 2 * U, U)

    wh, wdu = g * s * u, d * g * s
    out.append(half_ulp(wh, dtype) + both(lambda rho, uu: wh.abs() * (rho + 2 * uu)) + (g * u).abs() * floor)
    A, B = d * u * s, 1 + g * oms
    wdg = A * B

    def fdg(rho, uu):
        dB = g.abs() * (s * rho + uu * oms) + uu * (g * oms).abs() + uu * (1 + (g * oms).abs())
        return A.abs() * dB + wdg.abs() * (rho + 3 * uu)

    out.append(half_ulp(wdg, dtype) + both(fdg) + (d * u).abs() * (1 + g.abs()) * floor)
    out.append(half_ulp(wdu, dtype) + both(lambda rho, uu: wdu.abs() * (rho + 2 * uu)) + (d * g).abs() * floor)
    return (wh, wdg, wdu), out


def check_swiglu(what, dtype, gate, up, dh):
    C = ext()
    F = gate.shape[1]
    gu = torch.cat([gate, up], 1).contiguous()
    (wh, wdg, wdu), (bh, bdg, bdu) = swiglu_bounds(dtype, gate, up, dh)
    h = C.swiglu_fwd(gu)
    dgu = C.swiglu_bwd(dh, gu)
    report(f"swiglu_fwd {what}", h, wh, bh)
    report(f"swiglu_bwd dgate {what}", dgu[:, :F], wdg, bdg)
    report(f"swiglu_bwd dup {what}", dgu[:, F:], wdu, bdu)
    dgu2, h2 = C.swiglu_bwd_h(dh, gu)
    assert same_bits(h2, h), "swiglu_bwd_h's h is bitwise swiglu_fwd's"
    assert same_bits(dgu2, dgu), "swiglu_bwd_h's dgu is bitwise swiglu_bwd's"


@FORMATS
def test_swiglu_every_finite_gate(dtype):
    """The gate over every finite value of the format, against three up values of magnitude <= 1."""
    gate = all_finite(dtype)[None, :].expand(3, -1).contiguous()
    up = torch.tensor([1.0, -0.625, 2.0 ** -7], device=DEV)[:, None].expand_as(gate).to(dtype).contiguous()
    dh = randn(gen(31), *gate.shape).to(dtype)
    check_swiglu(f"{dtype} exhaustive", dtype, gate, up, dh)


@FORMATS
@pytest.mark.parametrize("N,F", [(5, 8), (WRAP_VECS, 8)], ids=["5x8", "wrap"])
def test_swiglu_shapes(dtype, N, F):
    g = gen(N)
    check_swiglu(f"{dtype} N={N} F={F}", dtype, randn(g, N, F, scale=3.0).to(dtype), randn(g, N, F).to(dtype),
                 randn(g, N, F).to(dtype))


# =================================================================================================== RoPE
def rope_tables(T, D):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D // 2, dtype=F64) * 2.0 / D))
    ang = torch.arange(T, dtype=F64)[:, None] * inv[None, :]
    return ang.cos().float().to(DEV), ang.sin().float().to(DEV)


def check_rope(what, dtype, T, N, Hq, Hkv, D, pad):
    """Hq + Hkv rotated heads, then Hkv value heads, in rows ``pad`` elements wider than that."""
    C = ext()
    heads = Hq + Hkv
    wide = (heads + Hkv) * D + pad
    buf = randn(gen(T + D), N, wide).to(dtype)
    view = buf[:, :wide - pad]
    assert pad == 0 or not view.is_contiguous()
    cos, sin = rope_tables(T, D)
    x0 = buf.clone()
    for inverse in (False, True):
        before = buf.clone()
        C.rope_(view, cos, sin, T, heads, D, inverse)
        src = before[:, :heads * D].reshape(N, heads, D)
        want = rope64(src, cos, sin, T, inverse)
        # o1 = x1 c - x2 s, o2 = x2 c + x1 s: a multiply and an fma, 2 roundings on the magnitudes added
        half = D // 2
        t = torch.arange(N, device=DEV) % T
        c, s = cos.double()[t][:, None, :].abs(), sin.double()[t][:, None, :].abs()
        x1, x2 = src[..., :half].double().abs(), src[..., half:].double().abs()
        mags = torch.cat([x1 * c + x2 * s, x2 * c + x1 * s], -1)
        report(f"rope {what} inverse={inverse}", buf[:, :heads * D].reshape(N, heads, D), want,
               half_ulp(want, dtype) + MARGIN * 2 * U * mags)
        assert same_bits(buf[:, heads * D:], x0[:, heads * D:]), "value and padding columns keep their bits"


@FORMATS
@pytest.mark.parametrize("D", [16, 64, 128])
def test_rope(dtype, D):
    check_rope(f"{dtype} D={D}", dtype, T=5, N=10, Hq=3, Hkv=2, D=D, pad=24)


@FORMATS
def test_rope_past_the_grid_wrap(dtype):
    # N * heads * D / 16 = 174 764 * 3 = 524 292 lane items: past 256 * 2048
    check_rope(f"{dtype} wrap", dtype, T=43691, N=174764, Hq=2, Hkv=1, D=16, pad=8)


# ================================================================================================ dropout
@FORMATS
@pytest.mark.parametrize("p", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("rows,cols", [(WRAP_VECS, 8), (301, 24), (37, 1024)])
def test_dropout(dtype, rows, cols, p):
    """out = x + dropout(r) and out = dropout(r): dropped elements are x's bits (or +0), kept ones
    x + r / (1 - p): the fp32 scale (U), the multiply (U), the add (U on |x| + |r'|)."""
    C = ext()
    g = gen(rows + cols)
    x, r = randn(g, rows, cols).to(dtype), randn(g, rows, cols).to(dtype)
    sd = step_seed(99)
    seed = sd.device_tensor if p > 0 else None
    keep = keep_of(sd, 7, rows, cols, p) if p > 0 else torch.ones(rows, cols, dtype=torch.bool, device=DEV)
    if p == 1.0:
        assert not bool(keep.any())
    elif p == 0.1:
        assert abs(float(keep.float().mean()) - 0.9) < 0.01
    rs = torch.where(keep, r.double() / (1 - p), 0.0) if p < 1 else torch.zeros_like(r, dtype=F64)
    for xin in (x, None):
        what = f"dropout{'_add' if xin is not None else ''} {dtype} {rows}x{cols} p={p}"
        out = C.dropout(xin, r, p, seed, 7)
        assert not bool(torch.isnan(out).any())
        xs = xin.double() if xin is not None else torch.zeros_like(rs)
        want = xs + rs
        report(what, out, want, half_ulp(want, dtype) + MARGIN * U * (2 * rs.abs() + xs.abs() + rs.abs()))
        dropped = ~keep
        assert same_bits(out[dropped], (xin if xin is not None else torch.zeros_like(r))[dropped])
        assert same_bits(C.dropout(xin, r, p, seed, 7), out)
    if p == 0.1:       # the mask is the specification's: the same seed and site in another kernel's decisions
        ones = torch.ones_like(r)
        assert torch.equal(C.dropout(None, ones, p, seed, 7) != 0, keep)
        assert not torch.equal(C.dropout(None, ones, p, seed, 8) != 0, keep)


# ============================================================================================== embedding
def id_mix(g, B, T, V):
    """Heavy repeats (20 distinct ids), some -1 and some V: both kernels skip those; nothing else out of range."""
    idx = torch.randint(0, 20, (B, T), device=DEV, generator=g)
    flat = idx.view(-1)
    flat[::9] = -1
    flat[4::31] = V
    flat[1] = V - 1
    return idx


@FORMATS
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("d", [8, 520, 768])
def test_embed_fwd_and_position_gradient(dtype, d, p):
    C = ext()
    B, T, V, P = 3, 7, 50, 10                                  # B T = 21 rows: no multiple of 4; wpe longer than T
    g = gen(d)
    wte, wpe = randn(g, V, d).to(dtype), randn(g, P, d).to(dtype)
    idx = torch.randint(0, V, (B, T), device=DEV, generator=g)
    sd = step_seed(5)
    seed = sd.device_tensor if p else None
    keep = keep_of(sd, 2, B * T, d, p).view(B, T, d) if p else None
    x = C.embed_fwd(idx, wte, wpe, p, seed, 2)
    want = embed64(idx, wte, wpe, keep, p)
    # (a + b) * scale: the add, the fp32 scale, the multiply
    report(f"embed_fwd {dtype} d={d} p={p}", x, want, half_ulp(want, dtype) + MARGIN * 3 * U * want.abs())
    if p:
        assert not bool(x[~keep].float().abs().any())
    dx = randn(g, B, T, d).to(dtype)
    want = embed_dwpe64(dx, P, keep, p)
    mags = embed_dwpe64(dx.double().abs(), P, keep, p)
    for accumulate in (False, True):
        dwpe0 = randn(gen(1), P, d).to(dtype)
        dwpe = dwpe0.clone()
        C.embed_bwd(dx, idx, None, dwpe, accumulate, p, seed, 2)
        prev = dwpe0.double() if accumulate else torch.zeros_like(want)
        # per element: the scale (2 U), B adds from 0, 1 to accumulate
        report(f"embed_bwd dwpe {dtype} d={d} p={p} acc={accumulate}", dwpe, want + prev,
               half_ulp(want + prev, dtype) + MARGIN * (B + 3) * U * (mags + prev.abs()))
        if accumulate:
            assert same_bits(dwpe[T:], dwpe0[T:]), "rows past T keep their bits when accumulating"
        else:
            assert not bool(bits(dwpe[T:]).any()), "rows past T become +0"


def check_embed_dwte(what, dtype, B, T, V, d, p):
    C = ext()
    g = gen(B * T + d)
    idx = id_mix(g, B, T, V)
    dx = randn(g, B, T, d).to(dtype)
    sd = step_seed(6)
    seed = sd.device_tensor if p else None
    keep = keep_of(sd, 4, B * T, d, p).view(B, T, d) if p else None
    dwte0 = randn(g, V, d).to(dtype)                           # accumulates onto a non-zero table
    outs = []
    for _ in range(2):
        dwte = dwte0.clone()
        C.embed_bwd(dx, idx, dwte, None, False, p, seed, 4)
        outs.append(dwte)
    assert same_bits(outs[0], outs[1]), f"{what}: repeated call"
    want = embed_dwte64(dx, idx, V, keep, p) + dwte0.double()
    mags = embed_dwte64(dx.double().abs(), idx, V, keep, p) + dwte0.double().abs()
    flat = idx.view(-1)
    ok = (flat >= 0) & (flat < V)
    cnt = torch.bincount(flat[ok], minlength=V).double()[:, None]
    # a row's sum: from the old value, one add per position of that id in a fixed order; the scale 2 U per term
    report(f"embed_bwd dwte {what}", outs[0], want, half_ulp(want, dtype) + MARGIN * (cnt + 2) * U * mags)
    untouched = cnt[:, 0] == 0
    assert same_bits(outs[0][untouched], dwte0[untouched]), f"{what}: rows of absent ids keep their bits"


@FORMATS
@pytest.mark.parametrize("N", [300, 4096])
def test_embed_token_gradient_scan_path(dtype, N):
    check_embed_dwte(f"scan {dtype} N={N}", dtype, 2, N // 2, 40, 64, 0.1 if N == 300 else 0.0)


@FORMATS
@pytest.mark.parametrize("B,T,d", [(2, 2050, 64), (2, 6, 4104)], ids=["N=4100", "d=4104"])
def test_embed_token_gradient_sort_path(dtype, B, T, d):
    """embed_bwd_tok_kernel behind torch's sort: more than 4096 rows, or a row wider than the scan kernel's 8 x 512."""
    check_embed_dwte(f"sort {dtype} N={B * T} d={d}", dtype, B, T, 40, d, 0.1)


# =================================================================================================== loss
XENT_V = [(8, 1), (4096, 1), (4104, 2), (32000, 8), (131072, 32)]


def xent_inputs(dtype, V):
    """randn * 2; row 1 one dominant logit; row 2 equal logits; row 3 ignored; in fp16 row 4 offset by 30000."""
    g = gen(V)
    z = torch.randn(5, V, device=DEV, generator=g) * 2
    z[1, V // 3] = 45.0
    z[2] = -1.5
    if dtype == F16:
        z[4] += 30000.0
    t = torch.randint(0, V, (5,), device=DEV, generator=g)
    t[1] = V // 3
    t[3] = -1
    return z.to(dtype), t


def xent_stat_bounds(z, vpt):
    """S = sum exp(z - m_thread), merged as (m, S) pairs.  Each exponential: its argument's rounding and the scaling
    inside __expf, 2 U |a| with |a| <= R = max z - min z, and H.  A thread adds 8 vpt terms; 6 butterfly rounds of
    2 multiplies, 1 add and 1 __expf (H + U R) each; the 8 waves: 1 multiply, 1 __expf, 8 adds:
        dS / S <= 8 H + U (2 R + 7 R + 8 vpt + 6 * 3 + 9) = 8 H + U (9 R + 8 vpt + 27)
    lse = M + __logf(S): dS / S, the logarithm's H |log S| + U |log S|, the add U |lse|.  Returns (fp32 part, H part)."""
    z = z.double()
    R = z.max(-1).values - z.min(-1).values
    lse = torch.logsumexp(z, -1)
    logS = (lse - z.max(-1).values).abs()
    return U * (9 * R + 8 * vpt + 27 + logS + lse.abs()), H * (8 + logS), R


@FORMATS
@pytest.mark.parametrize("V,vpt", XENT_V)
def test_xent(dtype, V, vpt):
    C = ext()
    z, t = xent_inputs(dtype, V)
    want_loss, want_lse, want_d = xent64(z, t)
    e32, eh, R = xent_stat_bounds(z, vpt)
    what = f"xent {dtype} V={V}"
    a = z.clone()
    loss = C.xent_fwd_bwd_(a, t, -1)
    # loss = lse - z[t]: one more rounding, on the magnitudes subtracted
    zt = z.double().gather(1, t.clamp(min=0)[:, None])[:, 0].abs()
    lb = MARGIN * (e32 + U * (want_lse.abs() + zt)) + eh
    report(f"{what} loss", loss, want_loss, lb)
    assert float(loss[3]) == 0.0 and not bool(bits(a[3]).any()), "an ignored row: loss 0, dlogits +0"
    # dlogits = e_i * (__expf(m_t - M) / S) (- 1 at the target): e_i H + 2 U R, the thread's factor H + U R, S as
    # above, the divide and the multiply 2 U; the target's subtraction U on 1 + p
    p = torch.exp(z.double() - want_lse[:, None])
    onehot = torch.zeros_like(p).scatter_(1, t.clamp(min=0)[:, None], 1.0) * (t >= 0)[:, None]
    db = half_ulp(want_d, dtype) + p * (10 * H + MARGIN * U * (12 * R[:, None] + 8 * vpt + 29)) + MARGIN * U * onehot * (1 + p)
    db[3] = 0.0
    report(f"{what} dlogits", a, want_d, db)
    # the split pair: loss rows bitwise the fused kernel's, lse to its bound, dlogits from the kernel's own lse
    loss2, lse = C.xent_lse(z, t, -1)
    assert same_bits(loss2, loss), "xent_lse's loss rows carry xent_fwd_bwd_'s bits"
    report(f"{what} lse", lse, want_lse, MARGIN * e32 + eh)
    b = z.clone()
    C.xent_bwd_lse_(b, t, lse, -1)
    # exp(z - lse) - onehot: the subtraction and __expf's scaling 2 U |z - lse|, H; the target's subtraction U
    arg = (z.double() - lse.double()[:, None])
    p2 = torch.exp(arg)
    want2 = (p2 - onehot) * (t >= 0)[:, None]
    b2 = half_ulp(want2, dtype) + p2 * (H + MARGIN * 2 * U * arg.abs()) + MARGIN * U * onehot * (1 + p2)
    b2[3] = 0.0
    report(f"{what} xent_bwd_lse_", b, want2, b2)
    c = z.clone()
    assert same_bits(C.xent_fwd_bwd_(c, t, -1), loss) and same_bits(c, a), "repeated call"


@pytest.mark.parametrize("N", [1, 1025, 3000])
def test_xent_mean(N):
    """out = (sum(loss) / max(count, 1), max(count, 1)): a lane adds ceil(N / 1024) rows, block_sum 6 + 16 adds, the
    divide; the count is a small integer, exact."""
    C = ext()
    g = gen(N)
    t = torch.randint(0, 100, (N,), device=DEV, generator=g)
    if N > 1:
        t[::5] = -1
    loss = torch.rand(N, device=DEV, generator=g) * 10 * (t != -1)
    out = C.xent_mean(loss, t, -1)
    cnt = max(int((t != -1).sum()), 1)
    chain = -(-N // 1024) + 22 + 1
    assert float(out[1]) == cnt
    report(f"xent_mean N={N}", out[:1], loss.double().sum()[None] / cnt, MARGIN * chain * U * loss.double().sum() / cnt)
    none = torch.full((N,), -1, device=DEV)
    out = C.xent_mean(torch.zeros(N, device=DEV), none, -1)
    assert out.tolist() == [0.0, 1.0], "every row ignored: the count clamps to 1"


@FORMATS
@pytest.mark.parametrize("with_den", [False, True])
def test_scale_by_past_the_grid_wrap(dtype, with_den):
    """y = x * (num / den): the divide (U) and the multiply (U); the stored scale: the divide."""
    C = ext()
    x = randn(gen(41), WRAP_VECS * 8).to(dtype)
    num = torch.tensor([3.0], device=DEV)
    den = torch.tensor([7.0], device=DEV) if with_den else None
    gout = torch.zeros(1, device=DEV)
    y = C.scale_by(x, num, den, gout)
    sc = 3.0 / 7.0 if with_den else 3.0
    report(f"scale_by {dtype} den={with_den} scale", gout, torch.tensor([sc], dtype=F64, device=DEV), MARGIN * U * sc)
    want = x.double() * sc
    report(f"scale_by {dtype} den={with_den}", y, want, half_ulp(want, dtype) + MARGIN * 2 * U * want.abs())
    assert same_bits(C.scale_by(x, num, den, None), y)
