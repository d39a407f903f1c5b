"""Float64 references of the optimizer update path (csrc/adamw.hip), written from the kernels' own
header comments with plain torch / Python arithmetic: no extension, no dltb import.

    adamw64  one AdamW step on float64 tensors (returns new tensors, the inputs are left alone)
    amp64    one dynamic-loss-scaling decision (the comment above amp_step_kernel), with the AdamW
             hyper-parameter tensor hp = [lr, lr/bc1, 1/sqrt(bc2), skip] it maintains
    clip64   the gradient-clipping coefficient and norm
"""
import math

import torch


def adamw64(master, m, v, g, lr, b1, b2, eps, wd, t, gscale=None):
    """p *= 1 - lr*wd;  m = lerp(m, g, 1-b1);  v = b2 v + (1-b2) g^2;
    p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps), with g multiplied by ``gscale`` first."""
    assert master.dtype == m.dtype == v.dtype == torch.float64
    g = g.double()
    if gscale is not None:
        g = g * float(gscale)
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    p = master * (1.0 - lr * wd)
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    denom = v.sqrt() / math.sqrt(bc2) + eps
    p = p - (lr / bc1) * m / denom
    return p, m, v


def clip64(norm_sq, max_norm, extra_scale):
    """(coef, norm): norm = sqrt(norm_sq) * extra, coef = extra * min(1, max_norm / (norm + 1e-6))
    (no clipping with max_norm <= 0)."""
    nrm = math.sqrt(norm_sq) * extra_scale
    c = min(1.0, max_norm / (nrm + 1e-6)) if max_norm > 0 else 1.0
    return c * extra_scale, nrm


def amp64(state, norm_sq, hp, max_norm, extra_scale, b1, b2, growth, backoff, interval):
    """state = [scale S, growth tracker, optimizer steps taken, steps skipped]; norm_sq the sum of
    squares of the S-scaled gradients.  Returns (state, coef, norm_out, hp), all new.

    found inf / nan -> hp[3] = 1, coef = 0, norm_out = norm_sq, S *= backoff, tracker = 0, skipped += 1
                       (hp[0..2] and the step count stay);
    otherwise       -> norm = sqrt(norm_sq) / S * extra, coef = extra * clip(norm) / S, t = taken + 1,
                       hp[1] = hp[0] / (1 - b1^t), hp[2] = 1 / sqrt(1 - b2^t), hp[3] = 0,
                       tracker += 1 and S *= growth when it reaches ``interval``.
    ``b1`` / ``b2`` are used as given: pass the float32-rounded betas to compare with the kernel."""
    S, tracker, taken, skipped = (float(x) for x in state)
    hp = [float(x) for x in hp]
    norm_sq = float(norm_sq)
    if not math.isfinite(norm_sq):
        hp[3] = 1.0
        return [S * backoff, 0.0, taken, skipped + 1.0], 0.0, norm_sq, hp
    c, nrm = clip64(norm_sq, max_norm, extra_scale / S)       # norm and clip of the unscaled gradient
    t = taken + 1.0
    hp[1] = hp[0] / (1.0 - b1 ** t)
    hp[2] = 1.0 / math.sqrt(1.0 - b2 ** t)
    hp[3] = 0.0
    tracker += 1.0
    if tracker >= interval:
        S *= growth
        tracker = 0.0
    return [S, tracker, t, skipped], c, nrm, hp


# The loss-scaling sequence driven through amp64, the CPU branch of DynamicLossScaler.step and the
# amp_step kernel: sums of squares of the scaled gradients, call by call.  With S = 1024,
# extra_scale = 1/8 and max_norm = 1 the unscaled norms are 0.37, 5.3 (clip active), inf (S -> 512),
# 0.37, nan (S -> 256), then 0.43, 8.9 (clip active) and 0.51: three clean calls in a row, so with
# growth_interval = 3 the scale doubles on the last of them.
AMP_NORM_SQ = (9.1e6, 1.9e9, float("inf"), 2.3e6, float("nan"), 7.7e5, 3.3e8, 1.1e6)
AMP_INIT_SCALE = 1024.0
AMP_INTERVAL = 3
AMP_EXTRA = 0.125


def bias_correction_bound(beta, t):
    """Relative error allowed on lr / (1 - beta^t) and 1 / sqrt(1 - beta^t) evaluated in float32: a
    two-ulp powf (2 * 2^-24 relative on beta^t <= 1) amplified by the cancellation in 1 - beta^t,
    plus one ulp each for the subtraction, the divide and the sqrt."""
    return 2.0 ** -23 / (1.0 - beta ** t) + 2.0 ** -22
