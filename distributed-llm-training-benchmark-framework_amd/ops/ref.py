"""Pure-torch reference implementations of every dltb kernel.

They reproduce the HIP kernels' semantics — same dropout masks (counter hash of
:mod:`dltb.ops.rng`), same rounding points (the residual stream ``s`` is rounded to the storage
dtype before normalisation, softmax-xent writes unscaled dlogits, ...) — computed in fp32.  They
are the CPU execution path of the model (unit tests, gloo multi-process tests) and the oracle the
GPU kernel tests compare against.
"""
import math

import torch
import torch.nn.functional as F

from .rng import C_COL, C_ROW, MASK32, _fmix32, _mul32, attn_keep_mask, keep_mask, keep_mask_2d, site_seed


def _f(t):
    """fp32 compute copy (fp64 inputs stay fp64 for precision tests)."""
    return t if t.dtype == torch.float64 else t.float()


def _seed(seed, site):
    return site_seed(int(seed.value), site)


def _drop(x32, p, seed, site, row_offset=0):
    if p <= 0.0:
        return x32
    s = _seed(seed, site)
    n_cols = x32.shape[-1]
    keep = keep_mask_2d(s, x32.numel() // n_cols, n_cols, p, device=x32.device,
                        row_offset=row_offset).view(x32.shape)
    return torch.where(keep, x32 * (1.0 / (1.0 - p)), torch.zeros((), device=x32.device))


# ------------------------------------------------------------------------------ norms
def norm_fwd(x, r, w, b, eps, rms, p, seed, site):
    dt = x.dtype
    x32 = _f(x)
    s = None
    if r is not None:
        s = (x32 + _drop(_f(r), p, seed, site)).to(dt)
        x32 = _f(s)
    if rms:
        var = x32.pow(2).mean(-1, keepdim=True)
        rstd = torch.rsqrt(var + eps)
        y = x32 * rstd * _f(w)
        mean = None
    else:
        mean = x32.mean(-1, keepdim=True)
        var = (x32 - mean).pow(2).mean(-1, keepdim=True)
        rstd = torch.rsqrt(var + eps)
        y = (x32 - mean) * rstd * _f(w) + _f(b)
        mean = mean.reshape(-1)
    return s, y.to(dt), mean, rstd.reshape(-1)


def norm_apply(s, w, b, mean, rstd, rms):
    """y of :func:`norm_fwd` rebuilt from the stored residual stream ``s`` and the statistics it returned."""
    x32 = _f(s)
    rstd = rstd.reshape(x32.shape[:-1] + (1,))
    if rms:
        y = x32 * rstd * _f(w)
    else:
        y = (x32 - mean.reshape(x32.shape[:-1] + (1,))) * rstd * _f(w) + _f(b)
    return y.to(s.dtype)


def _write_slot(slot, val, accumulate):
    if slot is None:
        return
    v = val.reshape(slot.shape).float()
    if accumulate:
        v = v + _f(slot)
    slot.copy_(v)


def norm_bwd(dy, s, w, mean, rstd, dres, gw, gb, accumulate, rms):
    d = dy.shape[-1]
    dy32 = _f(dy).reshape(-1, d)
    x32 = _f(s).reshape(-1, d)
    rstd = rstd.reshape(-1, 1)
    mu = 0.0 if rms else mean.reshape(-1, 1)
    xh = (x32 - mu) * rstd
    g = dy32 * _f(w)
    s2 = (g * xh).mean(-1, keepdim=True)
    if rms:
        dx = rstd * (g - xh * s2)
    else:
        s1 = g.mean(-1, keepdim=True)
        dx = rstd * (g - s1 - xh * s2)
    if dres is not None:
        dx = dx + _f(dres).reshape(-1, d)
    _write_slot(gw, (dy32 * xh).sum(0), accumulate)
    if not rms:
        _write_slot(gb, dy32.sum(0), accumulate)
    return dx.to(dy.dtype).view_as(dy)


def sandwich_fwd(x, a, w_out, w_next, eps):
    """Sandwich norm, "normalise, then add": rstd_a = rsqrt(mean(a^2) + eps), s = round16(x + a rstd_a w_out) -- the
    normalised value is never rounded on its own -- and, with ``w_next``, rstd_s and y = round16(s rstd_s w_next) from
    the STORED s, as :func:`norm_fwd` forms them.  Returns (s, y | None, rstd_a, rstd_s | None)."""
    dt = x.dtype
    a32 = _f(a)
    rstd_a = torch.rsqrt(a32.pow(2).mean(-1, keepdim=True) + eps)
    s = (_f(x) + a32 * rstd_a * _f(w_out)).to(dt)
    if w_next is None:
        return s, None, rstd_a.reshape(-1), None
    s32 = _f(s)
    rstd_s = torch.rsqrt(s32.pow(2).mean(-1, keepdim=True) + eps)
    return s, (s32 * rstd_s * _f(w_next)).to(dt), rstd_a.reshape(-1), rstd_s.reshape(-1)


def sandwich_bwd(dy, s, w_next, rstd_s, dres, a, w_out, rstd_a):
    """The backward of :func:`sandwich_fwd` with ``w_next``: ds = dres + RMSNormBwd(dy; s, w_next, rstd_s),
    dx = round16(ds), da = round16(RMSNormBwd(dx; a, w_out, rstd_a)) from the STORED dx -- two :func:`norm_bwd` in a
    row.  Returns (dx, da, part) with part fp32 [2, 1, d]: the sums over the rows of dy s rstd_s (gradient of
    ``w_next``) and of dx a rstd_a (gradient of ``w_out``); the GPU kernel returns one row per workgroup."""
    d = dy.shape[-1]
    part = torch.zeros(2, 1, d, dtype=torch.float32, device=dy.device)
    dx = norm_bwd(dy, s, w_next, None, rstd_s, dres, part[0, 0], None, False, True)
    da = norm_bwd(dx, a, w_out, None, rstd_a, None, part[1, 0], None, False, True)
    return dx, da, part


# ------------------------------------------------------------------------------ elementwise
def gelu_fwd(f):
    return F.gelu(_f(f)).to(f.dtype)


def gelu_bwd(dg, f, db, accumulate):
    x = _f(f)
    cdf = 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    df = (_f(dg) * (cdf + x * pdf)).to(dg.dtype)
    if db is not None:
        _write_slot(db, _f(df).reshape(-1, df.shape[-1]).sum(0), accumulate)
    return df


def colsum_into(src, out, accumulate):
    _write_slot(out, _f(src).reshape(-1, src.shape[-1]).sum(0), accumulate)


def dropout(x, r, p, seed, site):
    out = _drop(_f(r), p, seed, site)
    if x is not None:
        out = out + _f(x)
    return out.to(r.dtype)


GLU_ACTS = {"silu": False, "swiglu": False, "geglu": True}      # name -> the gate's activation is gelu_tanh


def glu_is_geglu(act):
    """True for the GeGLU FFN (``"geglu"``), False for SwiGLU (``"silu"`` or the config's ``"swiglu"``)."""
    if act not in GLU_ACTS:
        raise ValueError(f"the gated FFN's activation must be one of {', '.join(GLU_ACTS)}, got {act!r}")
    return GLU_ACTS[act]


_GELU_K, _GELU_C = math.sqrt(2.0 / math.pi), 0.044715


def _gelu_tanh_parts(g):
    """(hp, grad) with gelu_tanh(g) = g hp: hp = 0.5 (1 + t), t = tanh(k (g + c g^3)); grad = d gelu_tanh / dg =
    hp + 0.5 g (1 - t^2) k (1 + 3 c g^2), the second term exactly 0 where t = +-1 (0 * inf once g^2 overflows)."""
    g2 = g * g
    t = torch.tanh(_GELU_K * (g * (1.0 + _GELU_C * g2)))
    hp = 0.5 * (1.0 + t)
    q = 1.0 - t * t
    second = torch.where(q == 0, torch.zeros_like(g), 0.5 * g * q * (_GELU_K * (1.0 + 3.0 * _GELU_C * g2)))
    return hp, hp + second


def swiglu_fwd(gu, act="silu"):
    """h = silu(gate) * up; ``act="geglu"``: h = gelu_tanh(gate) * up (the Gemma FFN)."""
    F2 = gu.shape[-1] // 2
    g, u = _f(gu)[..., :F2], _f(gu)[..., F2:]
    if glu_is_geglu(act):
        return (g * _gelu_tanh_parts(g)[0] * u).to(gu.dtype)
    return (F.silu(g) * u).to(gu.dtype)


def swiglu_bwd(dh, gu, act="silu"):
    F2 = gu.shape[-1] // 2
    g, u = _f(gu)[..., :F2], _f(gu)[..., F2:]
    d = _f(dh)
    if glu_is_geglu(act):
        hp, grad = _gelu_tanh_parts(g)
        return torch.cat([d * grad * u, d * (g * hp)], -1).to(gu.dtype)
    s = torch.sigmoid(g)
    dg = d * u * s * (1 + g * (1 - s))
    du = d * g * s
    return torch.cat([dg, du], -1).to(gu.dtype)


def swiglu_bwd_h(dh, gu, act="silu"):
    """(dgu, h): :func:`swiglu_bwd` and the forward's h = :func:`swiglu_fwd` (gu), which the forward did not keep."""
    return swiglu_bwd(dh, gu, act), swiglu_fwd(gu, act)


def rope_tables(T, D, theta, device=None):
    half = D // 2
    inv = 1.0 / (theta ** (torch.arange(0, half, dtype=torch.float64) * 2.0 / D))
    ang = torch.arange(T, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().float().to(device), ang.sin().float().to(device)


def rope_(qkv2d, cos, sin, T, heads, D, inverse=False):
    N = qkv2d.shape[0]
    half = D // 2
    x = _f(qkv2d[:, :heads * D]).view(N // T, T, heads, D)
    x1, x2 = x[..., :half], x[..., half:]
    c = cos[:T].view(1, T, 1, half)
    s = sin[:T].view(1, T, 1, half)
    if inverse:
        s = -s
    o1 = x1 * c - x2 * s
    o2 = x2 * c + x1 * s
    qkv2d[:, :heads * D] = torch.cat([o1, o2], -1).reshape(N, heads * D).to(qkv2d.dtype)


def _qk_weight(wq, wk, Hq, Hkv, D):
    """[Hq + Hkv, D]: the q weight for the q heads, the k weight for the k heads."""
    return torch.cat([_f(wq).reshape(1, D).expand(Hq, D), _f(wk).reshape(1, D).expand(Hkv, D)], 0)


def qknorm_rope_fwd(qkv2d, wq, wk, cos, sin, T, Hq, Hkv, D, eps):
    """QK-norm fused with RoPE, in place on the q|k columns: per row and head x -> RMSNorm over D with the q (k)
    weight, then the rotate-half rotation of :func:`rope_` at position ``row mod T``, all in fp32 with ONE rounding.
    The V columns are not touched.  Returns ``raw``, a contiguous copy of the q|k columns as they were (the backward
    recomputes rstd from it; the in-place result cannot be inverted bit-safely)."""
    N = qkv2d.shape[0]
    heads, half = Hq + Hkv, D // 2
    raw = qkv2d[:, :heads * D].clone().contiguous()
    x = _f(raw).view(N // T, T, heads, D)
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    y = x * rstd * _qk_weight(wq, wk, Hq, Hkv, D)
    y1, y2 = y[..., :half], y[..., half:]
    c = cos[:T].view(1, T, 1, half)
    s = sin[:T].view(1, T, 1, half)
    o1 = y1 * c - y2 * s
    o2 = y2 * c + y1 * s
    qkv2d[:, :heads * D] = torch.cat([o1, o2], -1).reshape(N, heads * D).to(qkv2d.dtype)
    return raw


def qknorm_rope_bwd_(dqkv2d, raw, wq, wk, cos, sin, T, Hq, Hkv, D, eps):
    """The backward of :func:`qknorm_rope_fwd`, in place on the q|k columns of ``dqkv2d``: g = R(-theta) dy in fp32,
    rstd recomputed from ``raw`` by the forward's expression, xh = x rstd, dx = rstd (g w - xh mean(g w xh)) rounded
    once.  Returns the weight-gradient partials (dwq_part, dwk_part), fp32 [1, D] each here (the GPU kernel returns
    one row per workgroup): g xh summed over the rows and the q (k) heads."""
    N = dqkv2d.shape[0]
    heads, half = Hq + Hkv, D // 2
    dy = _f(dqkv2d[:, :heads * D]).view(N // T, T, heads, D)
    d1, d2 = dy[..., :half], dy[..., half:]
    c = cos[:T].view(1, T, 1, half)
    s = sin[:T].view(1, T, 1, half)
    g = torch.cat([d1 * c + d2 * s, d2 * c - d1 * s], -1)
    x = _f(raw).view(N // T, T, heads, D)
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    xh = x * rstd
    gw = g * _qk_weight(wq, wk, Hq, Hkv, D)
    dx = rstd * (gw - xh * (gw * xh).mean(-1, keepdim=True))
    dqkv2d[:, :heads * D] = dx.reshape(N, heads * D).to(dqkv2d.dtype)
    t = (g * xh).reshape(N, heads, D)
    return t[:, :Hq].sum((0, 1)).reshape(1, D), t[:, Hq:].sum((0, 1)).reshape(1, D)


# ------------------------------------------------------------------------------ embedding
def embed_fwd(idx, wte, wpe, p, seed, site):
    B, T = idx.shape
    x = _f(wte)[idx] + _f(wpe)[:T][None]
    return _drop(x.reshape(B * T, -1), p, seed, site).reshape(B, T, -1).to(wte.dtype)


def embed_bwd(dx, idx, dwte, dwpe, accumulate_wpe, p, seed, site):
    B, T = idx.shape
    d = dx.shape[-1]
    g = _drop(_f(dx).reshape(B * T, d), p, seed, site)
    if dwpe is not None:
        full = torch.zeros(dwpe.shape, dtype=torch.float32, device=dx.device)
        full[:T] = g.view(B, T, d).sum(0)
        _write_slot(dwpe, full, accumulate_wpe)
    if dwte is not None:
        acc = _f(dwte)
        acc.index_add_(0, idx.reshape(-1), g)
        dwte.copy_(acc)


# ------------------------------------------------------------------------------ xent
def check_xent_opts(softcap, z_coef):
    """The head-loss options: ``softcap`` = C (the loss is formed from ``C * tanh(z / C)``) and ``z_coef`` = B (the
    loss gains ``B * logsumexp^2``); both finite numbers >= 0, 0 = off."""
    for name, v in (("softcap", softcap), ("z_coef", z_coef)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"xent: {name} must be a finite number >= 0 (0 = off), got {v!r}")


def _xent_capped(logits, softcap):
    """(c, 1 - tanh^2) in fp32: ``c = softcap * tanh(z / softcap)`` and the cap's derivative; (z, None) when off."""
    z = _f(logits)
    if not softcap:
        return z, None
    t = torch.tanh(z / softcap)
    return softcap * t, 1.0 - t * t


def _xent_grad(pr, dcap, t, valid, lse, z_coef):
    """``(pr (1 + 2 B lse) - onehot) (1 - tanh^2)``, 0 for ignored rows."""
    if z_coef:
        pr = pr * (1.0 + 2.0 * z_coef * lse)[:, None]
    pr.scatter_add_(-1, t[:, None], -torch.ones_like(pr[:, :1]))
    if dcap is not None:
        pr = pr * dcap
    return torch.where(valid[:, None], pr, torch.zeros_like(pr))


def xent_fwd_bwd_(logits, targets, ignore_index, softcap=0.0, z_coef=0.0):
    """Returns per-row loss; overwrites logits with unscaled (softmax - onehot).  With ``softcap`` = C / ``z_coef`` =
    B (:func:`check_xent_opts`): c = C tanh(z / C), ``loss = lse(c) - c_t + B lse^2`` and
    ``dz = (softmax(c) (1 + 2 B lse) - onehot) (1 - (c / C)^2)``."""
    check_xent_opts(softcap, z_coef)
    z, dcap = _xent_capped(logits, softcap)
    valid = targets != ignore_index
    lse = torch.logsumexp(z, -1)
    t = targets.clamp(min=0)
    tl = z.gather(-1, t[:, None])[:, 0]
    row = lse - tl
    if z_coef:
        row = row + z_coef * lse * lse
    loss = torch.where(valid, row, torch.zeros_like(lse))
    pr = _xent_grad(torch.softmax(z, -1), dcap, t, valid, lse, z_coef)
    logits.copy_(pr.to(logits.dtype))
    return loss


def xent_lse(logits, targets, ignore_index, softcap=0.0, z_coef=0.0):
    """(per-row loss, per-row log-sum-exp) in fp32; the logits are only read.  The loss is
    :func:`xent_fwd_bwd_`'s, the same expressions on the same values; under ``softcap`` the log-sum-exp is that of
    the capped logits."""
    check_xent_opts(softcap, z_coef)
    z, _ = _xent_capped(logits, softcap)
    valid = targets != ignore_index
    lse = torch.logsumexp(z, -1)
    tl = z.gather(-1, targets.clamp(min=0)[:, None])[:, 0]
    row = lse - tl
    if z_coef:
        row = row + z_coef * lse * lse
    return torch.where(valid, row, torch.zeros_like(lse)), lse


def xent_bwd_lse_(logits, targets, lse, ignore_index, softcap=0.0, z_coef=0.0):
    """Overwrites logits with unscaled ``exp(z - lse) - onehot`` (0 for ignored rows) from the kept
    log-sum-exp: :func:`xent_fwd_bwd_`'s gradient without its reduction, options included.  Returns logits."""
    check_xent_opts(softcap, z_coef)
    z, dcap = _xent_capped(logits, softcap)
    valid = targets != ignore_index
    t = targets.clamp(min=0)
    l = lse.to(torch.float32)
    pr = _xent_grad(torch.exp(z - l[:, None]), dcap, t, valid, l, z_coef)
    logits.copy_(pr.to(logits.dtype))
    return logits


# ------------------------------------------------------------------------------ attention
def check_window(window, causal):
    """Sliding window ``W >= 1``: query i sees key j iff ``i - W < j <= i`` (W keys including its own, the
    Hugging Face Mistral mask); 0 = no window.  Only defined together with the causal mask."""
    if window < 0:
        raise ValueError(f"attention: window must be >= 0 (0 = no window), got {window}")
    if window > 0 and not causal:
        raise ValueError("attention: a sliding window needs causal=True")


def check_bounds(bounds, causal, window, B, T):
    """Document bounds (:func:`doc_bounds`): an int32 ``[2, B, T]`` tensor, only together with the causal mask
    and instead of ``window`` (the window is folded into the bounds).  ``None`` = no document mask."""
    if bounds is None:
        return
    if not causal:
        raise ValueError("attention: document bounds need causal=True")
    if window:
        raise ValueError("attention: pass either bounds or window (doc_bounds folds the window in)")
    if bounds.dtype != torch.int32:
        raise ValueError(f"attention: bounds must be int32, got {bounds.dtype}")
    if tuple(bounds.shape) != (2, B, T):
        raise ValueError(f"attention: bounds must have shape [2, {B}, {T}], got {list(bounds.shape)}")


Q_RANGE_ALIGN = 128      # the attention kernels' query block (csrc/attention.hip, kBlockRows)


def check_q_range(q_range, T, causal, p):
    """Query range ``(q_begin, q_end)`` of a length-``T`` problem: the query-side tensors (q, o, do, dq, lse) hold
    only rows ``q_begin .. q_end - 1`` of every batch row, k / v / dk / dv all ``T`` rows, and every mask keeps
    meaning global positions (tensor row i is position ``q_begin + i``).  Both ends are multiples of 128 with
    ``0 <= q_begin < q_end <= T``; a range other than ``(0, T)`` is causal only and without attention dropout
    (the packed keep-mask is laid out for the square problem).  ``None`` = the whole row.  Returns
    ``(q_begin, q_end)``."""
    if q_range is None:
        return 0, T
    qb, qe = int(q_range[0]), int(q_range[1])
    if not 0 <= qb < qe <= T:
        raise ValueError(f"attention: q_range must satisfy 0 <= begin < end <= T, got ({qb}, {qe}) with T = {T}")
    if qb % Q_RANGE_ALIGN or qe % Q_RANGE_ALIGN:
        raise ValueError(f"attention: q_range bounds must be multiples of {Q_RANGE_ALIGN}, got ({qb}, {qe})")
    if (qb, qe) != (0, T):
        if not causal:
            raise ValueError("attention: a query range needs causal=True")
        if p > 0:
            raise ValueError("attention: a query range other than (0, T) needs dropout p = 0 (the packed keep-mask "
                             "is laid out for the square problem)")
    return qb, qe


def check_sink(sink, q, Hq, causal, p):
    """ValueError unless ``sink`` is None or [Hq] values of q's dtype under the causal mask without dropout."""
    if sink is None:
        return
    if not causal:
        raise ValueError("attention: a sink needs causal=True")
    if p != 0.0:
        raise ValueError(f"attention: a sink needs dropout p = 0, got {p}")
    if sink.numel() != Hq:
        raise ValueError(f"attention: sink must hold Hq = {Hq} values, got {sink.numel()}")
    if sink.dtype != q.dtype:
        raise ValueError(f"attention: sink must have q's dtype {q.dtype}, got {sink.dtype}")


def check_softcap(softcap, causal, p, sink):
    """Logit soft-capping ``cap``: every score x becomes ``cap * tanh(x / cap)`` before the masks and the softmax
    (Gemma-2 uses 50).  ValueError unless ``cap == 0`` (off), or ``cap`` is finite and > 0 under the causal mask,
    without dropout and without a sink."""
    if softcap == 0:
        return
    if not (isinstance(softcap, (int, float)) and math.isfinite(softcap) and softcap > 0):
        raise ValueError(f"attention: softcap must be 0 (off) or finite and > 0, got {softcap!r}")
    if not causal:
        raise ValueError("attention: softcap needs causal=True")
    if p != 0.0:
        raise ValueError(f"attention: softcap needs dropout p = 0, got {p}")
    if sink is not None:
        raise ValueError("attention: softcap together with a sink is not supported")


def doc_bounds(idx, eos_id, window=0):
    """Document mask of packed rows as two int32 planes ``[2, B, T]``.  A token equal to ``eos_id`` ends a
    document and belongs to it.  ``lo[b, i]`` is the first key query i sees (0 without an EOS in ``idx[b, :i]``,
    else 1 + the last one's position); ``hi[b, j]`` is one past the last query that sees key j (T without an
    EOS in ``idx[b, j:]``, else 1 + the first one's position).  A sliding window ``W > 0`` is folded in:
    ``lo[i] = max(lo[i], i - W + 1)``, ``hi[j] = min(hi[j], j + W)``.  Key j is visible to query i iff
    ``lo[i] <= j <= i`` (the same as ``j <= i < hi[j]``); both planes are non-decreasing along T and
    ``lo[i] <= i < hi[i]``.  The torch twin of the ``attn_doc_bounds`` kernel, and the CPU path."""
    if idx.dim() != 2 or idx.dtype != torch.int64:
        raise ValueError("doc_bounds: idx must be an int64 [B, T] tensor")
    if window < 0:
        raise ValueError(f"doc_bounds: window must be >= 0 (0 = no window), got {window}")
    B, T = idx.shape
    pos = torch.arange(T, device=idx.device, dtype=torch.int64).expand(B, T)
    eos = idx == eos_id
    last = torch.where(eos, pos, torch.full_like(pos, -1)).cummax(1).values       # last EOS at or before i
    lo = torch.cat([torch.zeros_like(pos[:, :1]), last[:, :-1] + 1], 1)           # ... strictly before i, + 1
    first = torch.where(eos, pos, torch.full_like(pos, T - 1)).flip(1).cummin(1).values.flip(1)
    hi = first + 1                                                                 # first EOS at or after j, + 1
    if window > 0:
        lo = torch.maximum(lo, pos - window + 1)
        hi = torch.minimum(hi, pos + window)
    return torch.stack([lo, hi]).to(torch.int32)


def _attn_probs(q, k, B, T, Hq, Hkv, D, scale, causal, window=0, bounds=None, qb=0, qe=None, softcap=0.0):
    """Scores [B, Hq, Tq, T] of the queries at positions ``qb .. qe - 1`` (default: all T) against all T keys.
    ``softcap`` = cap > 0: the raw scores x are capped to ``cap * tanh(x / cap)`` before the masks."""
    check_window(window, causal)
    check_bounds(bounds, causal, window, B, T)
    qe = T if qe is None else qe
    qh = _f(q).reshape(B, qe - qb, Hq, D).transpose(1, 2)        # [B,Hq,Tq,D]
    kh = _f(k).reshape(B, T, Hkv, D).transpose(1, 2)
    if Hq != Hkv:
        kh = kh.repeat_interleave(Hq // Hkv, dim=1)
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    if softcap:
        s = softcap * torch.tanh(s / softcap)
    if causal:
        m = torch.ones(T, T, dtype=torch.bool, device=q.device).triu(1)
        if 0 < window < T:                                            # keys j <= i - W are out of the band
            m |= torch.ones(T, T, dtype=torch.bool, device=q.device).tril(-window)
        s = s.masked_fill(m[qb:qe], float("-inf"))
        if bounds is not None:                                        # keys j < lo[b, i] are other documents
            j = torch.arange(T, device=q.device)
            lo = bounds[0].to(q.device)[:, qb:qe]                     # the lo plane is indexed by global query
            s = s.masked_fill((j[None, None, :] < lo[:, :, None])[:, None], float("-inf"))
    return s


def _attn_keep(B, Hq, T, p, seed, site, device):
    if p <= 0.0:
        return None
    s = _seed(seed, site)
    rows = torch.arange(B * Hq * T, dtype=torch.int64, device=device)[:, None]
    cols = torch.arange(T, dtype=torch.int64, device=device)[None, :]
    return attn_keep_mask(s, rows, cols, p).view(B, Hq, T, T)


def attn_fwd(q, k, v, B, T, Hq, Hkv, scale, causal, p, seed, site, window=0, bounds=None, q_range=None, sink=None,
             softcap=0.0):
    """``q_range`` (:func:`check_q_range`): q holds only the range's rows of each batch row; o [B * Tq, Hq * D]
    and lse [B, Hq, Tq] come back for those rows.  ``sink`` ([Hq], :func:`check_sink`): one raw logit per query head
    is appended to every row's scores as a column without a value: the log-sum-exp runs over [scores | sink], the
    probabilities of the real keys sum to less than 1.  ``softcap`` (:func:`check_softcap`): the scores are capped
    before the masks; lse is that of the capped scores."""
    D = q.shape[1] // Hq
    qb, qe = check_q_range(q_range, T, causal, p)
    check_sink(sink, q, Hq, causal, p)
    check_softcap(softcap, causal, p, sink)
    s = _attn_probs(q, k, B, T, Hq, Hkv, D, scale, causal, window, bounds, qb, qe, softcap)
    lse = torch.logsumexp(s, -1)                                      # [B,Hq,T]
    if sink is not None:
        # log-sum-exp over the row with the sink column appended, as log(exp(lse of the scores) + exp(sink)): a sink
        # whose exp underflows beside the row leaves lse as it was, to the bit
        lse = torch.logaddexp(lse, _f(sink).to(lse.dtype).view(1, Hq, 1))
    pr = torch.exp(s - lse[..., None])
    keep = _attn_keep(B, Hq, T, p, seed, site, q.device)
    if keep is not None:
        pr = torch.where(keep, pr / (1.0 - p), torch.zeros((), device=q.device))
    vh = _f(v).reshape(B, T, Hkv, D).transpose(1, 2)
    if Hq != Hkv:
        vh = vh.repeat_interleave(Hq // Hkv, dim=1)
    o = torch.matmul(pr, vh).transpose(1, 2).reshape(B * (qe - qb), Hq * D)
    return o.to(q.dtype), _f(lse).contiguous()


def attn_sink_bwd(lse, delta, sink):
    """The sink gradient as partials [1, Hq] (the GPU kernel returns one row per workgroup):
    ``ds_h = - sum_{b, t} exp(sink_h - lse[b, h, t]) * delta[b, h, t]`` with delta = rowsum(dO * O)."""
    Hq = lse.shape[1]
    sk = _f(sink).to(lse.dtype).view(1, Hq, 1)
    return -(torch.exp(sk - lse) * delta.to(lse.dtype)).sum((0, 2)).reshape(1, Hq)


def attn_bwd(q, k, v, o, do, lse, dq, dk, dv, B, T, Hq, Hkv, scale, causal, p, seed, site, window=0,
             bounds=None, q_range=None, sink=None, softcap=0.0):
    """``q_range``: q, o, do, lse, dq hold the range's rows; dk, dv all T rows -- the range's contribution, zero
    in every row no query of the range sees.  ``sink``: the forward's sinks; o and lse include them, so dq / dk / dv
    are formed as without (p = exp(s - lse), delta = rowsum(dO * O): the sink's value is the zero vector) and the
    sink gradient is returned as [1, Hq] partials (:func:`attn_sink_bwd`); None without a sink.  ``softcap``: the
    forward's cap; with z = cap tanh(x / cap), dz = p (dP - delta) as ever and dx = dz (1 - tanh(x / cap)^2), the
    tanh recomputed from the same product (a masked score has dz = 0)."""
    D = q.shape[1] // Hq
    G = Hq // Hkv
    qb, qe = check_q_range(q_range, T, causal, p)
    check_sink(sink, q, Hq, causal, p)
    check_softcap(softcap, causal, p, sink)
    Tq = qe - qb
    s = _attn_probs(q, k, B, T, Hq, Hkv, D, scale, causal, window, bounds, qb, qe, softcap)
    pr = torch.exp(s - lse.view(B, Hq, Tq)[..., None])
    keep = _attn_keep(B, Hq, T, p, seed, site, q.device)
    z = torch.ones_like(pr) if keep is None else keep.to(pr.dtype) / (1.0 - p)   # fp64 inputs stay fp64
    qh = _f(q).reshape(B, Tq, Hq, D).transpose(1, 2)
    kh = _f(k).reshape(B, T, Hkv, D).transpose(1, 2).repeat_interleave(G, dim=1)
    vh = _f(v).reshape(B, T, Hkv, D).transpose(1, 2).repeat_interleave(G, dim=1)
    doh = _f(do).reshape(B, Tq, Hq, D).transpose(1, 2)
    oh = _f(o).reshape(B, Tq, Hq, D).transpose(1, 2)
    delta = (doh * oh).sum(-1, keepdim=True)
    pd = pr * z
    dvh = torch.matmul(pd.transpose(-1, -2), doh)                     # [B,Hq,T,D]
    dp = torch.matmul(doh, vh.transpose(-1, -2))
    ds = pr * (dp * z - delta)
    if softcap:         # through the cap: 1 - tanh^2 from the capped scores (masked entries: ds = 0 already)
        ds = ds * (1.0 - torch.where(torch.isfinite(s), s / softcap, torch.zeros_like(s)) ** 2)
    dqh = torch.matmul(ds, kh) * scale
    dkh = torch.matmul(ds.transpose(-1, -2), qh) * scale
    if G > 1:
        dkh = dkh.view(B, Hkv, G, T, D).sum(2)
        dvh = dvh.view(B, Hkv, G, T, D).sum(2)
    dq.copy_(dqh.transpose(1, 2).reshape(B * Tq, Hq * D).to(dq.dtype))
    dk.copy_(dkh.transpose(1, 2).reshape(B * T, Hkv * D).to(dk.dtype))
    dv.copy_(dvh.transpose(1, 2).reshape(B * T, Hkv * D).to(dv.dtype))
    if sink is None:
        return None
    return attn_sink_bwd(_f(lse).view(B, Hq, Tq), delta.squeeze(-1), sink)


# ------------------------------------------------------------------------------ mixture of experts
# Top-k routing with a fixed capacity (csrc/moe.hip).  N token rows, E experts, K choices per token, C slots per
# expert.  Index tensors are int32: expert / slot [N, K], src / src_k [E * C], counts [E]; slot -1 = dropped
# assignment, src -1 = empty slot.  fp64 inputs stay fp64 (precision tests).
MOE_MAX_EXPERTS = 64
MOE_TOP_K = (1, 2, 4)


def moe_capacity(N, E, K, factor):
    """Slots per expert: min(ceil(factor N K / E), N), rounded up to a multiple of 16 (the GEMMs' row granularity)."""
    c = min(int(math.ceil(factor * N * K / E)), N)
    return -(-c // 16) * 16


def moe_route(h, wr, K):
    """(expert, gate, logits): logits = h Wr^T in fp32; the K largest per row, ordered by descending logit, ties by
    ascending expert index; gates = softmax over the K chosen logits."""
    logits = _f(h) @ _f(wr).t()
    vals, idx = torch.sort(logits, dim=-1, descending=True, stable=True)
    sel = vals[:, :K]
    ex = torch.exp(sel - sel[:, :1])
    return idx[:, :K].to(torch.int32).contiguous(), ex / ex.sum(-1, keepdim=True), logits


def moe_assign(expert, E, C):
    """(slot, src, src_k, counts).  Assignment (n, k) to expert e gets position p = the number of assignments to e
    among the earlier (n', k') in row-major order; its slot is e C + p, or -1 (dropped) when p >= C.  src / src_k:
    the token row and choice held by each slot.  counts: assignments per expert before dropping."""
    N, K = expert.shape
    flat = expert.reshape(-1).long()
    onehot = F.one_hot(flat, E)
    pos = (onehot.cumsum(0) - onehot).gather(1, flat[:, None]).squeeze(1)
    keep = pos < C
    slot = torch.where(keep, flat * C + pos, torch.full_like(pos, -1))
    src = torch.full((E * C,), -1, dtype=torch.int32, device=expert.device)
    src_k = torch.full((E * C,), -1, dtype=torch.int32, device=expert.device)
    i = torch.arange(N * K, device=expert.device)[keep]
    src[slot[keep]] = (i // K).to(torch.int32)
    src_k[slot[keep]] = (i % K).to(torch.int32)
    return slot.to(torch.int32).view(N, K), src, src_k, onehot.sum(0).to(torch.int32)


# Dropless routing: one packed row space [0, R) instead of E slabs of C rows.  Expert e owns the segment
# [offsets[e], offsets[e + 1]), offsets = the exclusive prefix sum of the counts rounded up to MOE_SEGMENT rows (the
# grouped GEMMs' tile, csrc/gemm_grouped.hip), and R is static: every assignment fits whatever the routing.
MOE_SEGMENT = 128


def moe_dropless_rows(N, E, K):
    """R = roundup(N K, 128) + 128 E: at least sum_e roundup(counts[e], 128) for any counts that sum to N K."""
    return -(-(N * K) // MOE_SEGMENT) * MOE_SEGMENT + MOE_SEGMENT * E


def moe_assign_dropless(expert, E):
    """(slot [N, K], src [R], src_k [R], counts [E], offsets [E + 1]), all int32.  Assignment (n, k) to expert e at
    position p (the row-major order of :func:`moe_assign`) gets slot offsets[e] + p; nothing is dropped.  Every row
    of [0, R) without an assignment -- the padding of a segment, the tail past offsets[E] -- has src = src_k = -1."""
    N, K = expert.shape
    R = moe_dropless_rows(N, E, K)
    flat = expert.reshape(-1).long()
    onehot = F.one_hot(flat, E)
    pos = (onehot.cumsum(0) - onehot).gather(1, flat[:, None]).squeeze(1)
    counts = onehot.sum(0)
    seg = -(-counts // MOE_SEGMENT) * MOE_SEGMENT
    offsets = torch.cat([torch.zeros(1, dtype=seg.dtype, device=seg.device), seg.cumsum(0)])
    slot = offsets[flat] + pos
    src = torch.full((R,), -1, dtype=torch.int32, device=expert.device)
    src_k = torch.full((R,), -1, dtype=torch.int32, device=expert.device)
    i = torch.arange(N * K, device=expert.device)
    src[slot] = (i // K).to(torch.int32)
    src_k[slot] = (i % K).to(torch.int32)
    return slot.to(torch.int32).view(N, K), src, src_k, counts.to(torch.int32), offsets.to(torch.int32)


def gemm_grouped_nt(a, offsets, bs, out=None):
    """c[r] = a[r] bs[e]^T for the rows r of segment e = [offsets[e], offsets[e + 1]); rows past offsets[E] are zero.
    A loop over the experts on the host-read offsets (the CPU definition of csrc/gemm_grouped.hip's NT kernel)."""
    off = offsets.tolist()
    c = torch.zeros(a.shape[0], bs[0].shape[0], dtype=a.dtype, device=a.device) if out is None else out.zero_()
    for e, b in enumerate(bs):
        if off[e + 1] > off[e]:
            c[off[e]:off[e + 1]] = (_f(a[off[e]:off[e + 1]]) @ _f(b).t()).to(a.dtype)
    return c


def gemm_grouped_tn(dy, x, offsets, dws, accumulate):
    """dws[e] (+)= dy[segment e]^T x[segment e] in place; an empty segment writes zeros, or nothing when
    ``accumulate[e]``."""
    off = offsets.tolist()
    for e, dw in enumerate(dws):
        rows = slice(off[e], off[e + 1])
        v = _f(dy[rows]).t() @ _f(x[rows])
        if accumulate[e]:
            if off[e + 1] == off[e]:
                continue
            v = v + _f(dw)
        dw.copy_(v)


def _moe_rows(t, index):
    """t[index] with zero rows where index < 0."""
    ok = (index >= 0)[:, None]
    return torch.where(ok, t[index.clamp(min=0).long()], torch.zeros((), dtype=t.dtype, device=t.device))


def moe_dispatch(h, src):
    """xe[s] = h[src[s]]; empty slots are exactly zero."""
    return _moe_rows(h, src)


def moe_combine(ye, slot, gate):
    """m[n] = sum_k gate[n, k] ye[slot[n, k]] over the kept k, in k order in fp32, rounded once."""
    y = _f(ye)
    acc = torch.zeros(slot.shape[0], y.shape[1], dtype=y.dtype, device=y.device)
    for k in range(slot.shape[1]):
        acc = acc + gate[:, k:k + 1].to(y.dtype) * _moe_rows(y, slot[:, k])
    return acc.to(ye.dtype)


def moe_combine_bwd(dm, ye, slot, src, expert, gate, E):
    """(dye, dgate, dlogits): dye[s] = gate(s) dm[src[s]] (zero rows for empty slots), dgate[n, k] =
    <dm[n], ye[slot[n, k]]> (0 when dropped), and the softmax backward dlogit_k = g_k (dgate_k - sum_j g_j dgate_j)
    scattered into a dense [N, E] row (0 for the experts not chosen)."""
    d32, y = _f(dm), _f(ye)
    g = gate.to(d32.dtype)
    N, K = slot.shape
    dgate = torch.zeros(N, K, dtype=d32.dtype, device=d32.device)
    dye = torch.zeros_like(y)
    for k in range(K):
        s = slot[:, k].long()
        ok = s >= 0
        dgate[:, k] = (d32 * _moe_rows(y, slot[:, k])).sum(-1)      # zero rows where dropped
        dye[s[ok]] = (g[:, k:k + 1] * d32)[ok]
    dl = g * (dgate - (g * dgate).sum(-1, keepdim=True))
    dlogits = torch.zeros(N, E, dtype=d32.dtype, device=d32.device).scatter_(1, expert.long(), dl)
    return dye.to(ye.dtype), dgate, dlogits


def moe_dispatch_bwd(dxe, slot, dlogits, wr):
    """dh[n] = sum_k dxe[slot[n, k]] + sum_e dlogits[n, e] Wr[e], in fp32, rounded once."""
    x = _f(dxe)
    acc = torch.zeros(slot.shape[0], x.shape[1], dtype=x.dtype, device=x.device)
    for k in range(slot.shape[1]):
        acc = acc + _moe_rows(x, slot[:, k])
    return (acc + dlogits.to(x.dtype) @ _f(wr).to(x.dtype)).to(dxe.dtype)


def moe_aux_fwd(logits, counts, K):
    """(lse [N], out [2] = (balance, z)) of the router's ``logits`` [N, E] and the assignment ``counts`` [E] (before
    drops) of K choices per token.  With p = softmax(logits) over all E experts and lse = logsumexp(logits) (row
    maximum subtracted): f[e] = counts[e] / (N K), a constant; P[e] = mean_n p[n, e];
    balance = E sum_e f[e] P[e] (1 for a uniform router, towards E as it collapses onto one expert);
    z = mean_n lse[n]^2."""
    N, E = logits.shape
    mx = logits.max(-1, keepdim=True).values
    ex = torch.exp(logits - mx)
    s = ex.sum(-1, keepdim=True)
    lse = (mx + torch.log(s)).squeeze(-1)
    f = counts.to(logits.dtype) / float(N * K)
    balance = E * (f * ((ex / s).sum(0) / N)).sum()
    z = (lse * lse).sum() / N
    return lse, torch.stack([balance, z])


def moe_aux_bwd_(dlogits, logits, lse, counts, g, K):
    """dlogits[n, e] += g_b (E / N) p[n, e] (f[e] - sum_j f[j] p[n, j]) + g_z (2 / N) lse[n] p[n, e] in place, with
    p = exp(logits - lse) and ``g`` = (g_b, g_z), the incoming gradients of :func:`moe_aux_fwd`'s (balance, z)."""
    N, E = logits.shape
    p = torch.exp(logits - lse[:, None])
    f = counts.to(logits.dtype) / float(N * K)
    g = g.to(logits.dtype)
    dot = (f * p).sum(-1, keepdim=True)
    dlogits += g[0] * (E / N) * (p * (f - dot)) + g[1] * (2.0 / N) * (lse[:, None] * p)
    return dlogits


def moe_router_wgrad(dlogits, h, dwr, accumulate, dense=False):
    """dWr (+)= dlogits^T h into the router's gradient slot.  ``dense``: which kernel the GPU runs (nothing here)."""
    h32 = _f(h)
    v = dlogits.to(h32.dtype).t() @ h32
    if accumulate:
        v = v + _f(dwr)
    dwr.copy_(v)


# ------------------------------------------------------------------------------ optimizer
def adamw_flat(master, exp_avg, exp_avg_sq, grad, lr, beta1, beta2, eps, wd, step, gscale=None):
    g = _f(grad)
    if gscale is not None:
        g = g * _f(gscale)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    master.mul_(1.0 - lr * wd)
    exp_avg.lerp_(g, 1.0 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
    denom = (exp_avg_sq.sqrt() / math.sqrt(bc2)).add_(eps)
    master.addcdiv_(exp_avg, denom, value=-(lr / bc1))


# ---- block-scaled FP8 moments (csrc/adamw.hip adamw_fp8_kernel; the contract, bit for bit) -------------------
# exp_avg and s = sqrt(exp_avg_sq) are stored as OCP E4M3 codes (uint8, torch.float8_e4m3fn bit patterns) with one
# fp32 power-of-two scale per 256 consecutive elements of a block-table row.  Rows are ADAM_CHUNK elements and start
# at a segment's first element, so a segment's blocks start at its first element too.
FP8_BLOCK = 256
ADAM_CHUNK = 4096                 # csrc/adamw.hip kAdamChunk (ext().adamw_chunk())
FP8_ROW_BLOCKS = ADAM_CHUNK // FP8_BLOCK
FP8_MAX = 448.0
FP8_NEAREST = 0x80000             # the random word that rounds to nearest (ties away from zero)
FP8_KIND_M, FP8_KIND_S = 0, 1


def fp8_scale_exp(a):
    """Exponent e of a block's scale 2^e for its absmax ``a`` (fp32 tensor): 0 where a == 0, else the smallest
    e >= -126 with a * 2^-e <= 448 (448 = 1.75 * 2^8, so a mantissa above 1.75 takes one more)."""
    bits = a.contiguous().view(torch.int32).to(torch.int64) & MASK32
    e = ((bits + 0x1FFFFF) >> 23) - 135
    return torch.where(a == 0, torch.zeros_like(e), e.clamp(min=-126))


def _pow2(e):
    return ((e + 127) << 23).to(torch.int32).view(torch.float32)


def fp8_key(seed: int, counter: int, kind: int) -> int:
    """Per-launch key of one moment: fmix32(fmix32(counter * C_ROW + seed_hi) ^ (seed_lo + (kind + 1) * C_COL))."""
    one = lambda v: int(_fmix32(torch.tensor(v & MASK32, dtype=torch.int64)))
    return one(one((counter & MASK32) * C_ROW + ((seed >> 32) & MASK32)) ^ (((seed & MASK32) + (kind + 1) * C_COL) & MASK32))


def fp8_rand20(seed: int, counter: int, kind: int, idx):
    """The 20 random bits of the owner indices ``idx`` (int64 tensor)."""
    x = (_mul32(idx & MASK32, C_COL) + _mul32((idx >> 32) & MASK32, C_ROW)) & MASK32
    return _fmix32(x ^ fp8_key(seed, counter, kind)) >> 12


def fp8_round(y, inv, r20, floor_pos):
    """``y * inv`` (fp32; ``inv`` a power of two) rounded to one of its two E4M3 neighbours by the 20-bit words
    ``r20`` (tensor or int): the word is added to the fp32 bit pattern and the low 20 mantissa bits are cleared.
    Values below 2^-6 are first moved into [2^-6, 2^-5), whose 3-bit grid is E4M3's subnormal grid 2^-9.
    ``floor_pos``: a positive y never becomes 0.  The result is exactly representable in E4M3."""
    t = y.abs() * inv
    sub = t < 2.0 ** -6
    w = torch.where(sub, t + 2.0 ** -6, t)
    bits = ((w.contiguous().view(torch.int32).to(torch.int64) & MASK32) + r20) & 0xFFF00000
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits)          # NaN / inf patterns of a poisoned input
    q = bits.to(torch.int32).view(torch.float32)
    q = torch.where(sub, q - 2.0 ** -6, q)
    if floor_pos:
        q = torch.where((y > 0) & (q == 0), torch.full_like(q, 2.0 ** -9), q)
    return torch.where(q == 0, torch.zeros_like(q), torch.copysign(q, y))


def fp8_quantize(y, kind, seed, counter, owner_off=0, rounding="stochastic"):
    """Flat fp32 ``y`` (blocks of 256 from its first element, the last one may be partial; element j has the owner
    index ``owner_off + j``) -> (codes uint8 [n], scales fp32 [ceil(n / 256)])."""
    assert rounding in ("stochastic", "nearest")
    y = y.detach().float().reshape(-1)
    n = y.numel()
    nb = (n + FP8_BLOCK - 1) // FP8_BLOCK
    yp = torch.zeros(nb * FP8_BLOCK, dtype=torch.float32, device=y.device)
    yp[:n] = y
    yp = yp.view(nb, FP8_BLOCK)
    e = fp8_scale_exp(yp.abs().amax(dim=1))
    if rounding == "nearest":
        r20 = FP8_NEAREST
    else:
        idx = torch.arange(owner_off, owner_off + nb * FP8_BLOCK, dtype=torch.int64, device=y.device)
        r20 = fp8_rand20(int(seed), int(counter), kind, idx).view(nb, FP8_BLOCK)
    q = fp8_round(yp, _pow2(-e)[:, None], r20, kind == FP8_KIND_S)
    codes = q.to(torch.float8_e4m3fn).view(torch.uint8).reshape(-1)[:n].clone()
    return codes, _pow2(e)


def fp8_dequantize(codes, scales):
    """codes uint8 [n], scales fp32 [ceil(n / 256)] -> fp32 [n]: the E4M3 value times its block's scale (exact)."""
    n = codes.numel()
    v = codes.reshape(-1).view(torch.float8_e4m3fn).float()
    return v * scales.repeat_interleave(FP8_BLOCK)[:n]


def adamw_flat_fp8(master, mq, sq, mscale, sscale, grad, lr, beta1, beta2, eps, wd, step, gscale=None, seed=0,
                   counter=0, owner_off=0, rounding="stochastic"):
    """:func:`adamw_flat` on ONE segment's views with FP8 moments: ``mq`` / ``sq`` uint8 codes, ``mscale`` /
    ``sscale`` the segment's ceil(len / 256) scales (views, updated in place).  v_old = (s_code * scale)^2; the
    update runs in fp32 with this step's v_new in the denominator; m_new and sqrt(v_new) are stored."""
    m = fp8_dequantize(mq, mscale)
    d = fp8_dequantize(sq, sscale)
    v = d * d
    adamw_flat(master, m, v, grad, lr, beta1, beta2, eps, wd, step, gscale)
    for kind, val, codes, scales in ((FP8_KIND_M, m, mq, mscale), (FP8_KIND_S, v.sqrt(), sq, sscale)):
        c, sc = fp8_quantize(val, kind, seed, counter, owner_off, rounding)
        codes.copy_(c)
        scales.copy_(sc)
