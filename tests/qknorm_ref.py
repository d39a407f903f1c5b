"""Float64 references of the fused QK-norm + RoPE kernels (csrc/qknorm.hip), written from the kernels' header
comment with plain torch float64 on whatever device the inputs live on: no extension, no dltb import.

    qk_weight64            [Hq + Hkv, D]: the q weight for the q heads, the k weight for the k heads
    qknorm_rope64          y = RoPE(x rstd w), rstd = 1 / sqrt(mean_D(x^2) + eps); returns (y, rstd)
    qknorm_rope_bwd64      (dx, dwq, dwk) of it, by the hand-written formulas (g = R(-theta) dy, ...)
    qknorm_rope_autograd64 the same three by torch autograd of "RMSNorm per head, then rotate-half RoPE"
    fwd_bound, bwd_bounds  the error bounds of a 16-bit result computed in fp32 (derivation: tests/test_qknorm_cpu.py)

x / dy: [N, Hq + Hkv, D]; cos / sin: the kernel's own fp32 [>= T, D/2] tables; row r takes position r % T.
"""
import torch

from rowwise_ref import half_ulp, rope64

F64 = torch.float64
U = 2.0 ** -24          # one fp32 rounding, relative
MARGIN = 2.0            # on the fp32 part (tests/test_rowwise_gpu.py)


def qk_weight64(wq, wk, Hq, Hkv):
    D = wq.numel()
    return torch.cat([wq.double().reshape(1, D).expand(Hq, D), wk.double().reshape(1, D).expand(Hkv, D)], 0)


def qknorm_rope64(x, wq, wk, cos, sin, T, Hq, eps):
    x = x.double()
    rstd = 1.0 / ((x * x).mean(-1) + eps).sqrt()
    y = x * rstd[..., None] * qk_weight64(wq, wk, Hq, x.shape[1] - Hq)
    return rope64(y, cos, sin, T), rstd


def qknorm_rope_bwd64(dy, x, wq, wk, cos, sin, T, Hq, eps):
    x = x.double()
    g = rope64(dy.double(), cos, sin, T, inverse=True)
    rstd = (1.0 / ((x * x).mean(-1) + eps).sqrt())[..., None]
    xh = x * rstd
    gw = g * qk_weight64(wq, wk, Hq, x.shape[1] - Hq)
    dx = rstd * (gw - xh * (gw * xh).mean(-1, keepdim=True))
    t = g * xh
    return dx, t[:, :Hq].sum((0, 1)), t[:, Hq:].sum((0, 1))


def qknorm_rope_autograd64(dy, x, wq, wk, cos, sin, T, Hq, eps):
    """(y, dx, dwq, dwk) by autograd: RMSNorm over D per head with the q / k weight, then rotate-half RoPE."""
    x = x.double().clone().requires_grad_(True)
    wq = wq.double().clone().requires_grad_(True)
    wk = wk.double().clone().requires_grad_(True)
    N, heads, D = x.shape
    half = D // 2
    var = x.pow(2).mean(-1, keepdim=True)
    xn = x * torch.rsqrt(var + eps)
    y = torch.cat([xn[:, :Hq] * wq, xn[:, Hq:] * wk], 1)
    t = torch.arange(N, device=x.device) % T
    c = cos.double().reshape(-1, half)[t][:, None, :]
    s = sin.double().reshape(-1, half)[t][:, None, :]
    y1, y2 = y[..., :half], y[..., half:]
    out = torch.cat([y1 * c - y2 * s, y2 * c + y1 * s], -1)
    out.backward(dy.double())
    return out.detach(), x.grad, wq.grad, wk.grad


def _tables(cos, sin, N, T, half, device):
    t = torch.arange(N, device=device) % T
    return cos.double().reshape(-1, half)[t][:, None, :], sin.double().reshape(-1, half)[t][:, None, :]


def fwd_bound(dtype, x, wq, wk, cos, sin, T, Hq, eps, want, n_var, H=0.0):
    """Per-element bound of the forward's 16-bit output.  ``n_var``: fp32 roundings on var = mean(x^2) (squares, adds,
    the eps add); ``H``: relative error of a hardware rsqrt (0: none)."""
    x = x.double()
    N, heads, D = x.shape
    half = D // 2
    rstd = 1.0 / ((x * x).mean(-1, keepdim=True) + eps).sqrt()
    rho = (0.5 * (n_var + 1) + 1) * U
    y = (x * rstd * qk_weight64(wq, wk, Hq, heads - Hq)).abs()
    c, s = _tables(cos, sin, N, T, half, x.device)
    c, s = c.abs(), s.abs()
    Tm = torch.cat([y[..., :half] * c + y[..., half:] * s, y[..., half:] * c + y[..., :half] * s], -1)
    return half_ulp(want, dtype) + MARGIN * Tm * (rho + 4 * U) + Tm * H


def bwd_bounds(dtype, dy, x, wq, wk, cos, sin, T, Hq, eps, want_dx, n_var, n_dot, H=0.0):
    """(per-element bound of the 16-bit dx; per-term fp32 error of the weight-gradient terms g xh; their magnitudes
    |g xh|), the last two [N, heads, D] for the caller to sum over the rows and heads of a weight.  ``n_dot``: fp32
    roundings of the sum in mean(gw xh)."""
    x, dy = x.double(), dy.double()
    N, heads, D = x.shape
    half = D // 2
    w = qk_weight64(wq, wk, Hq, heads - Hq)
    rs = 1.0 / ((x * x).mean(-1, keepdim=True) + eps).sqrt()
    rho = (0.5 * (n_var + 1) + 1) * U
    c, s = _tables(cos, sin, N, T, half, x.device)
    d1, d2 = dy[..., :half], dy[..., half:]
    g = torch.cat([d1 * c + d2 * s, d2 * c - d1 * s], -1)
    Tg = torch.cat([(d1 * c).abs() + (d2 * s).abs(), (d2 * c).abs() + (d1 * s).abs()], -1)
    xh = x * rs
    gw = g * w
    dgw = 3 * U * Tg * w.abs() + U * gw.abs()
    m = (gw * xh).mean(-1, keepdim=True)
    dm = (3 * U * Tg * (w * xh).abs()).mean(-1, keepdim=True) \
        + (rho + (n_dot + 3) * U) * (gw * xh).abs().mean(-1, keepdim=True)
    Tin = gw.abs() + (xh * m).abs()
    e32 = rs * (dgw + xh.abs() * dm + (xh * m).abs() * (rho + 2 * U) + U * Tin) + rs * Tin * (rho + U)
    term = 3 * U * Tg * xh.abs() + (g * xh).abs() * (rho + 2 * U)
    return (half_ulp(want_dx, dtype) + MARGIN * e32 + 3 * H * rs * Tin, MARGIN * term + H * (g * xh).abs(),
            (g * xh).abs())
