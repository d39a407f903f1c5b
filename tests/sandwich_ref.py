"""Float64 references and error bounds of the sandwich-norm kernels (csrc/sandwich_norm.hip) and the GeGLU
instantiations of the gated-FFN kernels (csrc/elementwise.hip), written from the kernels' header comments with plain
torch float64 on whatever device the inputs live on: no extension, no dltb import.

    sandwich64          (s before its rounding, s = round16(.), rstd_a, y | None, rstd_s | None)
    sandwich_bwd64      (ds before its rounding, dx = round16(ds), da, dgamma of w_next, dgamma of w_out)
    sandwich_autograd64 the same gradients from torch autograd of the unrounded float64 composition
    gelu_tanh64, gelu_tanh_grad64, geglu64, geglu_grad64
    fwd_bounds, norm_y_bounds, rms_dx_bound, geglu_bounds     the bounds, derived in their docstrings

Bounds are built as in tests/test_rowwise_gpu.py: U = 2^-24 per fp32 rounding on the magnitudes that are added,
MARGIN = 2 on the fp32 part, H = 2^-20 (assumed) per hardware rsqrt / rcp / exp2, ``half_ulp`` per rounding to 16 bits.
"""
import math

import torch

from rowwise_ref import half_ulp, norm_bwd64, rmsnorm64, round16

F64 = torch.float64
U = 2.0 ** -24
H = 2.0 ** -20
MARGIN = 2.0
GELU_K, GELU_C = math.sqrt(2.0 / math.pi), 0.044715


def lane_terms(d):
    """Elements one lane adds up in a row reduction: 8 per register slice."""
    return 8 * ((d // 8 + 63) // 64)


# ------------------------------------------------------------------------------------------------ sandwich norm
def sandwich64(x, a, w_out, w_next, eps, dtype):
    """rstd_a = 1 / sqrt(mean(a^2) + eps); s = round16(x + a rstd_a w_out); with ``w_next`` y = s rstd_s w_next and
    rstd_s from the rounded s.  Returns (s before its rounding, s, rstd_a, y | None, rstd_s | None)."""
    n, _, rstd_a, _ = rmsnorm64(a, w_out, eps)
    s_exact = x.double() + n
    s = round16(s_exact, dtype)
    if w_next is None:
        return s_exact, s, rstd_a, None, None
    y, _, rstd_s, _ = rmsnorm64(s, w_next, eps)
    return s_exact, s, rstd_a, y, rstd_s


def sandwich_bwd64(dy, s, w_next, rstd_s, dres, a, w_out, rstd_a, dtype, dx_stored=None):
    """ds = dres + RMSNormBwd(dy; s, w_next, rstd_s); dx = round16(ds); da = RMSNormBwd(dx; a, w_out, rstd_a).
    ``dx_stored``: the dx the second half reads instead of round16(ds) (a kernel's own stored dx).  Returns
    (ds, dx, da, sum_rows dy s rstd_s, sum_rows dx a rstd_a)."""
    ds, g_next, _, _ = norm_bwd64(dy, s, w_next, None, rstd_s, dres)
    dx = round16(ds, dtype) if dx_stored is None else dx_stored.double()
    da, g_out, _, _ = norm_bwd64(dx, a, w_out, None, rstd_a)
    return ds, dx, da, g_next, g_out


def sandwich_autograd64(x, a, w_out, w_next, eps, dy, dres):
    """(dx, da, dw_next, dw_out) of L = sum(y dy) + sum(s dres) with s = x + RMSNorm(a; w_out), y = RMSNorm(s; w_next)
    (None: no y), by torch autograd in float64 without any rounding."""
    x, a, w_out = (t.detach().double().requires_grad_() for t in (x, a, w_out))

    def rms(v, w):
        return v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps) * w

    s = x + rms(a, w_out)
    loss = (s * dres.double()).sum()
    if w_next is not None:
        w_next = w_next.detach().double().requires_grad_()
        loss = loss + (rms(s, w_next) * dy.double()).sum()
    loss.backward()
    return x.grad, a.grad, (None if w_next is None else w_next.grad), w_out.grad


def rstd_bound(v, eps):
    """(relative fp32 error of rstd = rsqrtf(wave_sum(sum v^2) / d + eps) with MARGIN, without the rsqrt's H).
    A lane squares and adds its n = ``lane_terms(d)`` elements (2 n roundings), 6 butterfly rounds and the divide:
    (2 n + 7) U var; the eps add: U (var + eps); rsqrt halves the relative error."""
    v = v.double()
    n = lane_terms(v.shape[-1])
    var = (v * v).mean(-1)
    return 0.5 * MARGIN * ((2 * n + 7) * U * var + U * (var + eps)) / (var + eps)


def fwd_bounds(dtype, x, a, w_out, eps, want_s_exact, want_rstd_a):
    """(bound of rstd_a, bound of s).  s = x + (a * rstd_a) * w_out: the normalised value t carries rstd_a's error
    (``rstd_bound`` + H) and 2 multiplies; the add rounds on |x| + |t| (a fused multiply-add rounds less); then the one
    rounding to 16 bits."""
    rho = rstd_bound(a, eps)
    t = (a.double() * want_rstd_a[:, None] * w_out.double()).abs()
    e32 = t * (rho[:, None] + H) + MARGIN * U * (2 * t + x.double().abs() + t)
    return want_rstd_a * (rho + H), half_ulp(want_s_exact, dtype) + e32


def norm_y_bounds(dtype, s_stored, w, eps, want_y, want_rstd):
    """(bound of rstd_s, bound of y) for y = s * rstd_s * w of the STORED s: rstd's error and 2 multiplies."""
    rho = rstd_bound(s_stored, eps)
    t = (s_stored.double() * want_rstd[:, None] * w.double()).abs()
    return want_rstd * (rho + H), half_ulp(want_y, dtype) + t * (rho[:, None] + H) + MARGIN * U * 2 * t


def rms_dx_bound(dtype, dy, s, w, rstd, dres, want_dx):
    """dx = rstd * (g - xh * s2) (+ dres) with g = dy * w, xh = s * rstd, s2 = wave_sum(sum g xh) / d and rstd an
    fp32 input:  s2: n adds per lane, 6 butterfly rounds, the divide, 3 roundings in a term (g, xh, their product):
    (n + 10) U mean|g xh|;  inner difference on T = |g| + |xh s2|: g 1, xh and xh * s2 2, the subtraction 1 -> 4 U T,
    plus |xh| ds2;  times rstd: U;  + dres: U on the magnitudes added."""
    n = lane_terms(dy.shape[-1])
    rs = rstd.double()[:, None]
    xh = s.double() * rs
    g = dy.double() * w.double()
    s2 = (g * xh).mean(-1, keepdim=True)
    ds2 = (n + 10) * U * (g * xh).abs().mean(-1, keepdim=True)
    T = g.abs() + (xh * s2).abs()
    e32 = rs * (xh.abs() * ds2 + 4 * U * T) + U * rs * T
    if dres is not None:
        e32 = e32 + U * (rs * T + dres.double().abs())
    return half_ulp(want_dx, dtype) + MARGIN * e32


# ------------------------------------------------------------------------------------------------------- GeGLU
def _gelu_u(g):
    return GELU_K * (g + GELU_C * g * g * g)


def gelu_tanh64(g):
    """0.5 g (1 + tanh(u)), u = k (g + c g^3), as g sigmoid(2 u): 0.5 (1 + tanh u) without its cancellation."""
    g = g.double()
    return g * torch.sigmoid(2.0 * _gelu_u(g))


def gelu_tanh_grad64(g):
    """0.5 (1 + t) + 0.5 g (1 - t^2) k (1 + 3 c g^2) with 0.5 (1 - t^2) = 2 sigmoid(2 u) sigmoid(-2 u)."""
    g = g.double()
    u = _gelu_u(g)
    sp, sm = torch.sigmoid(2.0 * u), torch.sigmoid(-2.0 * u)
    return sp + g * (2.0 * sp * sm) * (GELU_K * (1.0 + 3.0 * GELU_C * g * g))


def geglu64(gate, up):
    return gelu_tanh64(gate) * up.double()


def geglu_grad64(dh, gate, up):
    """(dgate, dup) of h = gelu_tanh(gate) * up."""
    return dh.double() * gelu_tanh_grad64(gate) * up.double(), dh.double() * gelu_tanh64(gate)


SAT_Z = 160.0       # |2 log2(e) u| from which exp2 is inf / 0 in fp32 whatever the few-ulp error of its argument


def geglu_bounds(dtype, gate, up, dh):
    """Bounds of (h, dgate, dup) for the kernels' evaluation (csrc/elementwise.hip ``gelu_tanh_half``):

       z = 2 log2(e) k (g (1 + c g^2)): 6 roundings -> exp2's result carries rho_e = H + ln2 |z| 6 U relative
       r = rcp(1 + e): with sg = e / (1 + e) = 0.5 (1 + t) the true value, dr = r (sg rho_e + U + H)
       t = fma(-2, r, 1): dt = 2 dr + U;   hp = 0.5 (1 + t): dhp = dr + U / 2 + U hp   (an ABSOLUTE U / 2: the
           form cancels for negative gates, where hp is small)
       act = g hp: |g| dhp + U |act|;   h = act up, dup = dh act: one more U
       q = fma(-t, t, 1): dq = 2 |t| dt + U;  A = 0.5 g q: 0.5 |g| dq + U |A|;  B = k fma(3 c, g^2, 1): 3 U relative
       grad = fma(A, B, hp): dhp + B dA + 3 U |A B| + U |grad|;   dgate = (dh grad) up: 2 more U

    Where |z| >= SAT_Z the exp2 is exactly inf or 0, so r, t, hp are exactly their limits and the derivative's second
    term is exactly 0: there the bound on hp and grad is the true value's own distance from the limit (about
    exp(-|z|), nothing) -- the kernel must return the saturated values exactly, however large g is."""
    g, u_, d = gate.double(), up.double(), dh.double()
    Um = MARGIN * U
    uu = _gelu_u(g)
    z = 2.0 * math.log2(math.e) * uu
    sg, r = torch.sigmoid(2.0 * uu), torch.sigmoid(-2.0 * uu)
    t = sg - r                                                    # tanh(u)
    rho_e = H + math.log(2.0) * z.abs() * 6 * Um
    dr = r * (sg * rho_e + Um + H)
    dt = 2 * dr + Um
    dhp = dr + Um / 2 + Um * sg
    B = GELU_K * (1.0 + 3.0 * GELU_C * g * g)
    q = 4.0 * sg * r
    A = 0.5 * g * q
    grad = gelu_tanh_grad64(gate)
    dq = 2 * t.abs() * dt + Um
    dA = 0.5 * g.abs() * dq + Um * A.abs()
    dgrad = dhp + B * dA + 3 * Um * (A * B).abs() + Um * grad.abs()
    sat = z.abs() >= SAT_Z
    lim = (g > 0).double()
    dhp = torch.where(sat, (sg - lim).abs(), dhp)
    dgrad = torch.where(sat, (grad - lim).abs(), dgrad)
    act = g * sg
    dact = g.abs() * dhp + Um * act.abs()
    wh, wdg, wdu = act * u_, d * grad * u_, d * act
    bh = half_ulp(wh, dtype) + u_.abs() * dact + Um * wh.abs()
    bdu = half_ulp(wdu, dtype) + d.abs() * dact + Um * wdu.abs()
    bdg = half_ulp(wdg, dtype) + (d * u_).abs() * dgrad + 2 * Um * wdg.abs()
    return (wh, wdg, wdu), (bh, bdg, bdu)
