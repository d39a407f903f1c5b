"""Float64 references of the row-wise and elementwise kernels (csrc/norm.hip, csrc/elementwise.hip,
csrc/embedding.hip, csrc/xent.hip), written from the kernels' header comments with plain torch float64
on whatever device the inputs live on: no extension, no dltb import.

    half_ulp, round16           the 16-bit storage formats (bf16, fp16): spacing and round-to-nearest-even
    layernorm64, rmsnorm64      (y, mean | None, rstd, s) with s = round16(x + dropout(r)) the normalised row
    norm_bwd64                  (dx, dgamma, dbeta | None, column sum of round16(dx) | None)
    gelu64, gelu_grad64         x Phi(x) and Phi(x) + x phi(x), the erf form
    silu_mul64, silu_mul_grad64 silu(gate) * up and its (dgate, dup)
    rope64                      rotate-half RoPE on the kernel's own fp32 tables, forward and inverse
    embed64, embed_dwpe64, embed_dwte64
    xent64                      (loss rows, log-sum-exp rows, softmax - onehot)

Dropout keep decisions are an input (a boolean mask), never computed here.
"""
import math

import torch

F64 = torch.float64
# stored mantissa bits, smallest normal exponent, largest finite exponent
_FMT = {torch.float16: (10, -14, 15), torch.bfloat16: (7, -126, 127)}


def half_ulp(x, dtype):
    """Half the spacing of ``dtype`` at the float64 value(s) ``x``: the largest error of rounding x to the
    format.  Below the smallest normal the spacing is the subnormal one (2^-24 for fp16, 2^-133 for bf16);
    from the point where the format rounds to +-inf (the largest finite value plus half its spacing) the
    result is inf, as it is for a non-finite x."""
    mant, emin, emax = _FMT[dtype]
    a = torch.as_tensor(x, dtype=F64).abs()
    _, ex = torch.frexp(a)                                   # a = m 2^ex, m in [0.5, 1): a in [2^(ex-1), 2^ex)
    e = torch.where(a == 0, torch.full_like(ex, emin), ex - 1).clamp(min=emin)
    h = torch.ldexp(torch.ones_like(a), e - mant - 1)
    top = (2.0 - 2.0 ** -mant) * 2.0 ** emax                 # largest finite
    over = top + 2.0 ** (emax - mant - 1)                    # ties to even: the tie itself goes to inf
    return torch.where((a >= over) | ~torch.isfinite(a), torch.full_like(a, math.inf), h)


def round16(x, dtype):
    """float64 -> the nearest value of ``dtype`` (ties to even), returned as float64.  torch converts
    float64 through float32, which rounds twice; this picks among that candidate and its two neighbours."""
    mant, emin, emax = _FMT[dtype]
    x = torch.as_tensor(x, dtype=F64)
    a = x.abs()
    inf_key = ((1 << (15 - mant)) - 1) << mant               # bit pattern of +inf: 0x7C00 / 0x7F80
    key0 = a.to(dtype).view(torch.int16).to(torch.int64) & 0x7FFF
    key0 = key0.clamp(max=inf_key)

    def val(k):                                              # +inf stands for the next power of two
        v = k.to(torch.int16).view(dtype).to(F64)
        return torch.where(k >= inf_key, torch.full_like(v, 2.0 ** (emax + 1)), v)

    best_k, best_d = None, None
    for dk in (0, -1, 1):
        k = (key0 + dk).clamp(0, inf_key)
        d = (val(k) - a).abs()
        if best_k is None:
            best_k, best_d = k, d
        else:
            take = (d < best_d) | ((d == best_d) & (k % 2 == 0) & (best_k % 2 == 1))
            best_k, best_d = torch.where(take, k, best_k), torch.where(take, d, best_d)
    out = best_k.to(torch.int16).view(dtype).to(F64)          # the inf key reads back as inf
    out = torch.where(x < 0, -out, out)
    return torch.where(torch.isnan(x), x, out)


def dropped64(r, keep, p):
    """dropout(r) in float64: r / (1 - p) where ``keep``, else 0 (r itself without a mask)."""
    r = r.double()
    if keep is None:
        return r
    return torch.where(keep, r / (1.0 - p), torch.zeros_like(r)) if p < 1.0 else torch.zeros_like(r)


# ------------------------------------------------------------------------------------------ norms
def _stream64(x, residual, keep, p, dtype):
    s = x.double()
    if residual is not None:
        s = round16(s + dropped64(residual, keep, p), dtype or x.dtype)      # the kernel stores s and reads it back
    return s


def layernorm64(x, w, b, eps, residual=None, keep=None, p=0.0, dtype=None):
    """s = x + dropout(r) (rounded to the storage format);  y = (s - mean) * rstd * w + b with the biased
    variance.  Returns (y, mean, rstd, s)."""
    s = _stream64(x, residual, keep, p, dtype)
    mean = s.mean(-1)
    c = s - mean[..., None]
    rstd = 1.0 / ((c * c).mean(-1) + eps).sqrt()
    return c * rstd[..., None] * w.double() + b.double(), mean, rstd, s


def rmsnorm64(x, w, eps, residual=None, keep=None, p=0.0, dtype=None):
    """y = s * rstd * w, rstd = 1 / sqrt(mean(s^2) + eps).  Returns (y, None, rstd, s)."""
    s = _stream64(x, residual, keep, p, dtype)
    rstd = 1.0 / ((s * s).mean(-1) + eps).sqrt()
    return s * rstd[..., None] * w.double(), None, rstd, s


def norm_bwd64(dy, s, w, mean, rstd, dres=None, dxsum_dtype=None):
    """xhat = (s - mean) rstd, g = dy w;  dx = rstd (g - mean(g) - xhat mean(g xhat)) (+ dres);
    dgamma = sum_rows dy xhat, dbeta = sum_rows dy.  ``mean`` None: RMSNorm (no mean(g) term, no dbeta).
    ``dxsum_dtype``: also the column sum of dx rounded to that format."""
    dy, s, w, rstd = dy.double(), s.double(), w.double(), rstd.double()[:, None]
    rms = mean is None
    xh = (s if rms else s - mean.double()[:, None]) * rstd
    g = dy * w
    s1 = 0.0 if rms else g.mean(-1, keepdim=True)
    s2 = (g * xh).mean(-1, keepdim=True)
    dx = rstd * (g - s1 - xh * s2)
    if dres is not None:
        dx = dx + dres.double()
    dxs = round16(dx, dxsum_dtype).sum(0) if dxsum_dtype is not None else None
    return dx, (dy * xh).sum(0), (None if rms else dy.sum(0)), dxs


# ------------------------------------------------------------------------------------ elementwise
def _phi_cdf(x):
    return 0.5 * torch.special.erfc(-x * math.sqrt(0.5))    # (1 + erf(x / sqrt 2)) / 2 without its cancellation


def gelu64(x):
    x = x.double()
    return x * _phi_cdf(x)


def gelu_grad64(x):
    x = x.double()
    return _phi_cdf(x) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def silu_mul64(gate, up):
    g = gate.double()
    return g * torch.sigmoid(g) * up.double()


def silu_mul_grad64(dh, gate, up):
    """(dgate, dup) of h = silu(gate) * up."""
    g, u, d = gate.double(), up.double(), dh.double()
    s = torch.sigmoid(g)
    one_minus_s = torch.sigmoid(-g)
    return d * u * s * (1.0 + g * one_minus_s), d * g * s


def rope64(x, cos, sin, T, inverse=False):
    """x: [N, heads, D]; cos / sin: [>= T, D/2] tables; row r takes position r % T.  Pairs (i, i + D/2):
    o1 = x1 c - x2 s, o2 = x2 c + x1 s (s negated for the inverse)."""
    N, _, D = x.shape
    half = D // 2
    t = torch.arange(N, device=x.device) % T
    c = cos.double().reshape(-1, half)[t][:, None, :]
    s = sin.double().reshape(-1, half)[t][:, None, :]
    if inverse:
        s = -s
    x1, x2 = x[..., :half].double(), x[..., half:].double()
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


# -------------------------------------------------------------------------------------- embedding
def embed64(idx, wte, wpe, keep=None, p=0.0):
    """x[b, t] = dropout(wte[idx[b, t]] + wpe[t])."""
    T = idx.shape[1]
    return dropped64(wte.double()[idx] + wpe.double()[:T][None], keep, p)


def embed_dwpe64(dx, P, keep=None, p=0.0):
    """[P, d]: row t < T is sum_b g[b, t] with g = dropout_mask(dx) / (1 - p); rows >= T are zero."""
    g = dropped64(dx, keep, p)
    out = torch.zeros(P, g.shape[-1], dtype=F64, device=dx.device)
    out[:g.shape[1]] = g.sum(0)
    return out


def embed_dwte64(dx, idx, V, keep=None, p=0.0):
    """[V, d]: row v is the sum of g[r] over the positions with idx[r] = v; ids outside [0, V) are skipped."""
    g = dropped64(dx, keep, p).reshape(-1, dx.shape[-1])
    flat = idx.reshape(-1)
    ok = (flat >= 0) & (flat < V)
    out = torch.zeros(V, g.shape[-1], dtype=F64, device=dx.device)
    out.index_add_(0, flat[ok], g[ok])
    return out


# ------------------------------------------------------------------------------------------- loss
def xent64(logits, targets, ignore_index=-1):
    """(loss, lse, dlogits): lse = logsumexp(z), loss = lse - z[t], dlogits = softmax(z) - onehot(t); loss and
    dlogits are 0 on rows whose target is ``ignore_index`` or outside [0, V).  lse is given for every row."""
    z = logits.double()
    V = z.shape[-1]
    valid = (targets != ignore_index) & (targets >= 0) & (targets < V)
    t = targets.clamp(0, V - 1)
    lse = torch.logsumexp(z, -1)
    loss = torch.where(valid, lse - z.gather(-1, t[:, None])[:, 0], torch.zeros_like(lse))
    d = torch.exp(z - lse[:, None])
    d.scatter_add_(-1, t[:, None], -torch.ones_like(lse)[:, None])
    return loss, lse, torch.where(valid[:, None], d, torch.zeros_like(d))
