"""csrc/gemm_rs.hip, every production config (0 - 14), bit-exactly on small integers and inside the float64
bounds of tests/gemm_ref.py on N(0,1) data -- at the k-loop's edges (one round of the register pipeline,
the two-step minimum, several wraps of the three LDS buffers), at tile counts that are no multiple of 8 and
of gm, through operand views surrounded by NaN and row-strided outputs, and through the fused GELU / dGELU
epilogues.  bf16 only: the binding refuses fp16.

The table below is copied from kRsCfgs; ``step = 64 * d * kg`` is the K granule rs_fits demands (one round of
the d-deep register pipeline in each of the kg k-groups).  Every case asserts gemm_rs_supported first: none
is skipped."""
import pytest
import torch

import dltb  # noqa: F401
from dltb.ops._ext import ext

from gemm_ref import (EXACT_LIMIT, MARGIN, NT, U, bound, ints, one_hot_blame, one_hot_probe, poisoned_view,
                      product64, report)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
BM = 128
# cfg -> (bn, d, kg, nw): tile width, stages in flight, k-groups, waves per k-group (csrc/gemm_rs.hip kRsCfgs)
CFGS = {0: (64, 4, 1, 4), 1: (256, 2, 1, 4), 2: (192, 2, 1, 4), 3: (128, 2, 1, 4), 4: (64, 2, 1, 4),
        5: (64, 4, 1, 4), 6: (256, 2, 1, 8), 7: (192, 2, 1, 8), 8: (64, 4, 1, 8), 9: (64, 2, 2, 4),
        10: (64, 4, 2, 4), 11: (64, 2, 2, 4), 12: (64, 4, 2, 4), 13: (64, 2, 2, 4), 14: (64, 2, 2, 4)}
ALL = pytest.mark.parametrize("cfg", sorted(CFGS))
SENTINEL = -7.0


def gen(seed):
    return torch.Generator(DEV).manual_seed(seed)


def step_of(cfg):
    bn, d, kg, _ = CFGS[cfg]
    return 64 * d * kg


def bits(t):
    return t.contiguous().view(torch.int16)


def nan_out(M, N):
    return torch.full((M, N), float("nan"), device=DEV, dtype=BF16)


def supported(M, N, K, cfg):
    assert ext().gemm_rs_supported(M, N, K, cfg), f"cfg {cfg} refuses {M} x {N} x {K}"


def to16(x64):
    """The one rounding of an exact float64 result (an integer or a multiple of 0.5 below 2^24: exact in fp32,
    so torch's conversion through fp32 rounds once)."""
    assert float(x64.abs().max()) < EXACT_LIMIT
    return x64.to(BF16)


def exact_case(cfg, tm, tn, K, gm, mode, seed):
    """One launch on integers in [-2, 2] (bias / prev in [-8, 8]); out pre-filled with NaN unless accumulating."""
    bn = CFGS[cfg][0]
    M, N = tm * BM, tn * bn
    supported(M, N, K, cfg)
    g = gen(seed)
    a, b = ints(g, (M, K), BF16), ints(g, (N, K), BF16)
    bias = ints(g, (N,), BF16, -8, 8) if mode == "bias" else None
    prev = ints(g, (M, N), BF16, -8, 8) if mode == "acc" else None
    assert K * 2 * 2 + 8 < EXACT_LIMIT
    want, _ = product64(a, b, NT)
    if bias is not None:
        want = want + bias.double()
    if prev is not None:
        want = want + prev.double()
    out = prev.clone() if prev is not None else nan_out(M, N)
    y = ext().gemm_rs(a, b, out, bias, prev is not None, cfg, gm)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    ref = to16(want)
    if not torch.equal(out, ref):
        bad = (out != ref) | torch.isnan(out)
        rows, cols = bad.any(1).nonzero().flatten(), bad.any(0).nonzero().flatten()
        raise AssertionError(
            f"cfg {cfg} {M} x {N} x {K} gm {gm} {mode}: {int(bad.sum())} of {bad.numel()} elements differ "
            f"({int(torch.isnan(out).sum())} NaN = never written), rows {int(rows[0])}..{int(rows[-1])}, "
            f"cols {int(cols[0])}..{int(cols[-1])}, largest difference "
            f"{float((out.double() - ref.double()).nan_to_num(0).abs().max())}")


# ================================================================================ exact small integers
@ALL
def test_exact_k_edges(cfg):
    """K = 1, 2, 3, 5 granules: one round of the register pipeline (nkg == d; nkg == 2, the kernel's minimum, for
    the d = 2 configs) up to several wraps of the three LDS buffers; 2 x 2 tiles, gm 1 and 2; bias / accumulate
    / neither."""
    s = step_of(cfg)
    seed = 100 * cfg
    for mult in (1, 2, 3, 5):
        for gm in (1, 2):
            for mode in ("none", "bias", "acc"):
                seed += 1
                exact_case(cfg, 2, 2, mult * s, gm, mode, seed)


@ALL
@pytest.mark.parametrize("tm,tn", [(4, 2), (3, 2), (3, 3), (5, 1)], ids=["4x2", "3x2", "3x3", "5x1"])
def test_exact_tile_walks(cfg, tm, tn):
    """8, 6, 9 and 5 tiles (tiles & 7 != 0 in xcd_grouped) at gm 1, 2, 4 (the fallback walk when tiles_m % gm != 0):
    every tile written, each with its own product."""
    for gm in (1, 2, 4):
        exact_case(cfg, tm, tn, step_of(cfg), gm, "none", 1000 * cfg + 10 * tm + tn + gm)


@ALL
def test_one_hot(cfg):
    """Each output element is one B value picked by a one-hot row of A: a k-step read twice, skipped, or taken
    from the wrong LDS buffer or k-group names the k it read."""
    bn = CFGS[cfg][0]
    M, N, K = 2 * BM, 2 * bn, 3 * step_of(cfg)
    supported(M, N, K, cfg)
    a, b, want = one_hot_probe(M, N, K, BF16, NT, DEV)
    out = ext().gemm_rs(a, b, nan_out(M, N), None, False, cfg, 1)
    torch.cuda.synchronize()
    assert torch.equal(out.double(), want.double()), f"cfg {cfg}: " + one_hot_blame(out, want, K)


# ==================================================================================== poisoned views
def strided_out(M, N, fill):
    """(view [M, N] with row stride N + 8, its buffer): the 8 gap columns hold SENTINEL."""
    buf = torch.full((M, N + 8), SENTINEL, device=DEV, dtype=BF16)
    view = buf[:, :N]
    view.copy_(fill) if torch.is_tensor(fill) else view.fill_(fill)
    assert view.stride(0) == N + 8 and view.data_ptr() % 16 == 0
    return view, buf


def gap_untouched(buf, N):
    return torch.equal(bits(buf[:, N:]), bits(torch.full_like(buf[:, N:], SENTINEL)))


@ALL
@pytest.mark.parametrize("mode", ["none", "bias", "acc", "gelu", "aux"])
def test_poisoned_views(cfg, mode):
    """a and b lie inside NaN-filled buffers (128 rows above and below, 64 columns left and right), out (and
    gelu_out / aux) is a row-strided view with ldc = N + 8: lda / ldb / ldc are honoured, nothing outside an
    operand reaches the result, nothing is written into the gap."""
    C = ext()
    bn = CFGS[cfg][0]
    M, N, K = 2 * BM, 2 * bn, 2 * step_of(cfg)
    supported(M, N, K, cfg)
    if mode == "aux" and not C.gemm_rs_aux_supported(M, N, K, cfg):
        assert not aux_rule(cfg)                       # refused by design: test_aux_supported_rule pins the list
        return
    g = gen(50 * cfg + len(mode))
    a, abuf = poisoned_view(ints(g, (M, K), BF16), 128, 64)
    b, bbuf = poisoned_view(ints(g, (N, K), BF16), 128, 64)
    a_bits, b_bits = bits(abuf).clone(), bits(bbuf).clone()
    want, _ = product64(a, b, NT)
    assert a.stride(0) == K + 128 and b.stride(0) == K + 128
    if mode == "acc":
        prev = ints(g, (M, N), BF16, -8, 8)
        out, obuf = strided_out(M, N, prev)
        C.gemm_rs(a, b, out, None, True, cfg, 2)
        want = want + prev.double()
    elif mode == "gelu":
        bias = ints(g, (N,), BF16, -2, 2) * 0.5
        out, obuf = strided_out(M, N, float("nan"))
        gout, gbuf = strided_out(M, N, float("nan"))
        assert C.gemm_rs_gelu_supported(M, N, K, cfg)
        C.gemm_rs(a, b, out, bias, False, cfg, 2, gelu_out=gout)
        want = want + bias.double()
    elif mode == "aux":
        aux, xbuf = strided_out(M, N, ints(g, (M, N), BF16, -2, 2))
        out, obuf = strided_out(M, N, float("nan"))
        x_bits = bits(xbuf).clone()
        _, part = C.gemm_rs_aux(a, b, out, aux, cfg, 2)
        want = want * aux.double()
    else:
        bias = ints(g, (N,), BF16, -8, 8) if mode == "bias" else None
        out, obuf = strided_out(M, N, float("nan"))
        C.gemm_rs(a, b, out, bias, False, cfg, 2)
        if bias is not None:
            want = want + bias.double()
    torch.cuda.synchronize()
    assert not torch.isnan(out).any(), f"cfg {cfg} {mode}: {int(torch.isnan(out).sum())} NaN in out"
    assert torch.equal(out, to16(want)), f"cfg {cfg} {mode}: result through strided views differs"
    assert gap_untouched(obuf, N), f"cfg {cfg} {mode}: out's gap columns were written"
    assert torch.equal(bits(abuf), a_bits) and torch.equal(bits(bbuf), b_bits)
    if mode == "gelu":
        assert gap_untouched(gbuf, N), f"cfg {cfg}: gelu_out's gap columns were written"
        assert torch.equal(bits(gout), bits(C.gelu_fwd(out.contiguous(), None)))
    if mode == "aux":
        assert torch.equal(bits(xbuf), x_bits)
        assert torch.equal(part, out.double().view(M // BM, BM, N).sum(1).to(F32))


# ====================================================================== many co-resident workgroups
_big = {}


def big_operands(K):
    """4096 x K and 2048 x K integers, the bias and the rounded reference: once per K, never modified."""
    if K not in _big:
        g = gen(4096 + K)
        a, b, bias = ints(g, (4096, K), BF16), ints(g, (2048, K), BF16), ints(g, (2048,), BF16, -8, 8)
        _big[K] = (a, b, bias, to16(product64(a, b, NT)[0] + bias.double()))
    return _big[K]


@pytest.mark.parametrize("cfg", [0, 4, 9, 11])
def test_exact_coresident_workgroups(cfg):
    """4096 x 2048 on 128 x 64 tiles: 1024 workgroups, several per CU at once (the case that exposed the LDS race
    fixed by rs_barrier), exact and twice."""
    K = step_of(cfg)
    supported(4096, 2048, K, cfg)
    a, b, bias, ref = big_operands(K)
    for rep in range(2):
        out = ext().gemm_rs(a, b, nan_out(4096, 2048), bias, False, cfg, 4)
        torch.cuda.synchronize()
        nbad = int(((out != ref) | torch.isnan(out)).sum())
        assert nbad == 0, f"cfg {cfg} run {rep}: {nbad} elements differ"


# ============================================================================================ gelu_out
@ALL
def test_gelu_out_exact(cfg):
    """f = a b^T + bias exact (integers plus a bias from {-1, -0.5, 0, 0.5, 1}), g bitwise gelu_fwd(f)."""
    C = ext()
    bn = CFGS[cfg][0]
    M, N, K = 2 * BM, 2 * bn, step_of(cfg)
    supported(M, N, K, cfg)
    assert C.gemm_rs_gelu_supported(M, N, K, cfg), f"cfg {cfg}: GELU epilogue refused"
    g = gen(300 + cfg)
    a, b = ints(g, (M, K), BF16), ints(g, (N, K), BF16)
    bias = ints(g, (N,), BF16, -2, 2) * 0.5
    assert bias.dtype == BF16 and set(bias.unique().tolist()) <= {-1.0, -0.5, 0.0, 0.5, 1.0}
    gout = nan_out(M, N)
    f = C.gemm_rs(a, b, nan_out(M, N), bias, False, cfg, 2, gelu_out=gout)
    torch.cuda.synchronize()
    assert torch.equal(f, to16(product64(a, b, NT)[0] + bias.double())), f"cfg {cfg}: f differs"
    assert torch.equal(bits(gout), bits(C.gelu_fwd(f, None))), f"cfg {cfg}: g is not gelu_fwd(f) bitwise"


# ========================================================================================= gemm_rs_aux
def aux_rule(cfg):
    """RsEpiF::FIXED and AUX_PF: a thread keeps its 4 columns in every row, at most 16 aux chunks per thread."""
    bn, _, kg, nw = CFGS[cfg]
    nt, cpr = 64 * nw * kg, bn // 4
    return nt % cpr == 0 and BM * cpr // nt <= 16


def aux_shape(cfg):
    return 2 * BM, 2 * CFGS[cfg][0], step_of(cfg)           # two m-tiles of partials


def test_aux_supported_rule():
    C = ext()
    admitted = [c for c in sorted(CFGS) if C.gemm_rs_aux_supported(*aux_shape(c), c)]
    assert admitted == [c for c in sorted(CFGS) if aux_rule(c)]
    assert admitted == [0, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14]
    for c in sorted(set(CFGS) - set(admitted)):
        M, N, K = aux_shape(c)
        supported(M, N, K, c)
        z = torch.zeros(M, K, device=DEV, dtype=BF16)
        with pytest.raises(RuntimeError):
            C.gemm_rs_aux(z, torch.zeros(N, K, device=DEV, dtype=BF16), None,
                          torch.zeros(M, N, device=DEV, dtype=BF16), c, 1)


AUX = pytest.mark.parametrize("cfg", [c for c in sorted(CFGS) if aux_rule(c)])


@AUX
def test_aux_exact(cfg):
    """out = (a b^T) * aux rounded once with aux from {0, +-0.5, +-1, +-2}; part = the fp32 column sums of the
    rounded out per 128-row tile: multiples of 0.5 far below 2^24, so exact in any order."""
    C = ext()
    M, N, K = aux_shape(cfg)
    assert C.gemm_rs_aux_supported(M, N, K, cfg)
    g = gen(400 + cfg)
    a, b = ints(g, (M, K), BF16), ints(g, (N, K), BF16)
    vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], device=DEV, dtype=BF16)
    aux = vals[torch.randint(0, 7, (M, N), generator=g, device=DEV)]
    out, part = C.gemm_rs_aux(a, b, nan_out(M, N), aux, cfg, 2)
    torch.cuda.synchronize()
    assert torch.equal(out, to16(product64(a, b, NT)[0] * aux.double())), f"cfg {cfg}: out differs"
    sums = out.double().view(M // BM, BM, N).sum(1)
    assert float(out.double().abs().view(M // BM, BM, N).sum(1).max()) * 2 < EXACT_LIMIT
    assert part.dtype == F32 and part.shape == (M // BM, N)
    assert torch.equal(part, sums.to(F32)), f"cfg {cfg}: column partials differ"


@AUX
def test_aux_bounded(cfg):
    """aux = GELU'(f) of N(0,1) f (gelu_fwd_grad), N(0,1) operands: out inside the bound of the product scaled
    by |aux| (K products + the multiply: K + 2 covers it); part within 130 fp32 roundings (128 sequential adds
    and the fold) of the float64 sums of the kernel's own rounded out."""
    C = ext()
    M, N, K = aux_shape(cfg)
    g = gen(500 + cfg)
    a = torch.randn(M, K, device=DEV, generator=g).to(BF16)
    b = torch.randn(N, K, device=DEV, generator=g).to(BF16)
    f = torch.randn(M, N, device=DEV, generator=g).to(BF16)
    aux = C.gelu_fwd_grad(f)[1]
    out, part = C.gemm_rs_aux(a, b, nan_out(M, N), aux, cfg, 2)
    torch.cuda.synchronize()
    want, abs_sum = product64(a, b, NT)
    x = aux.double()
    report(f"gemm_rs_aux cfg {cfg} K {K} out", out, want * x, bound(want * x, abs_sum * x.abs(), K, BF16))
    tiles = out.double().view(M // BM, BM, N)
    report(f"gemm_rs_aux cfg {cfg} K {K} part", part, tiles.sum(1), MARGIN * 130 * U * tiles.abs().sum(1))


# ========================================================================= float64-bounded random data
@ALL
def test_bounded_random(cfg):
    """N(0,1) operands at one granule and at the largest K <= 1152; bias ~ N(0,1), then bias and accumulate onto
    prev ~ N(0,1): every element inside the order-free bound."""
    C = ext()
    bn = CFGS[cfg][0]
    s = step_of(cfg)
    M, N = 2 * BM, 2 * bn
    for K in sorted({s, 1152 // s * s}):
        supported(M, N, K, cfg)
        g = gen(600 + cfg + K)
        a = torch.randn(M, K, device=DEV, generator=g).to(BF16)
        b = torch.randn(N, K, device=DEV, generator=g).to(BF16)
        bias = torch.randn(N, device=DEV, generator=g).to(BF16)
        prev = torch.randn(M, N, device=DEV, generator=g).to(BF16)
        want, abs_sum = product64(a, b, NT)
        out = C.gemm_rs(a, b, nan_out(M, N), bias, False, cfg, 2)
        torch.cuda.synchronize()
        wb = want + bias.double()
        report(f"gemm_rs cfg {cfg} K {K} bias", out, wb, bound(wb, abs_sum, K, BF16, bias.double().abs()))
        out = prev.clone()
        C.gemm_rs(a, b, out, bias, True, cfg, 2)
        torch.cuda.synchronize()
        wp = wb + prev.double()
        report(f"gemm_rs cfg {cfg} K {K} bias + prev", out, wp,
               bound(wp, abs_sum, K, BF16, bias.double().abs() + prev.double().abs()))


# ======================================================================================== gemm_rs_pick
def pick_rule(M, N, K):
    """dltb_gemm_rs_pick: the admissible production config whose tile count is closest to 256 (a count above it
    weighs double), ties to the earlier."""
    best, bestd = -1, 1 << 30
    for c in sorted(CFGS):
        bn, d, kg, _ = CFGS[c]
        if M <= 0 or N <= 0 or K <= 0 or M % BM or N % bn or K % (64 * d * kg) or K // 64 < 2 * kg:
            continue
        tiles = (M // BM) * (N // bn)
        dist = (tiles - 256) * 2 if tiles > 256 else 256 - tiles
        if dist < bestd:
            best, bestd = c, dist
    return best


PICKS = [(2048, 1024, 1024), (2048, 4096, 512), (2048, 3072, 256), (1024, 2048, 128), (256, 192, 128),
         (384, 320, 256), (4096, 2048, 512), (128, 64, 128)]


@pytest.mark.parametrize("M,N,K", PICKS, ids=lambda v: str(v))
def test_pick(M, N, K):
    C = ext()
    cfg = C.gemm_rs_pick(M, N, K)
    assert 0 <= cfg <= 14, f"pick {cfg} is no production config"
    assert cfg == pick_rule(M, N, K)
    assert C.gemm_rs_supported(M, N, K, -1) and C.gemm_rs_supported(M, N, K, cfg)
    g = gen(M + N + K)
    a = torch.randn(M, K, device=DEV, generator=g).to(BF16)
    b = torch.randn(N, K, device=DEV, generator=g).to(BF16)
    auto = C.gemm_rs(a, b, nan_out(M, N), None, False, -1, 1)
    named = C.gemm_rs(a, b, nan_out(M, N), None, False, cfg, 1)
    torch.cuda.synchronize()
    assert torch.equal(bits(auto), bits(named))


def test_pick_refuses_what_nothing_fits():
    C = ext()
    for M, N, K in [(2048, 1024, 64), (2048, 1000, 1024), (100, 1024, 1024), (2048, 1024, 192 + 32)]:
        assert pick_rule(M, N, K) == -1 and C.gemm_rs_pick(M, N, K) == -1
        assert not C.gemm_rs_supported(M, N, K, -1)
