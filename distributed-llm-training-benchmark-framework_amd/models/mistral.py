"""Mistral-7B-shape decoder (BASELINE.json config #5: ZeRO-3 bf16 on 8x MI355X).

Not part of the reference (it only names a Mistral image, scripts/build.sh:4, and a 7B sizing note,
docs/ARCHITECTURE.md:452-460); built from the same fused per-unit Functions as TinyGPT so every
strategy engine handles it unchanged:

    x = embed_tokens[idx]
    per layer:  h1 = RMSNorm(x); qkv = h1 Wqkv^T (fused q|k|v, GQA: 32 q / 8 kv heads x 128);
                RoPE(q, k) in place; o = causal FlashAttn(qkv); x1 = x + o Wo^T;
                h2 = RMSNorm(x1) (fused with the residual add); gu = h2 Wgu^T (gate|up);
                x2 = x1 + SiLU(gate) * up Wd^T
    logits = RMSNorm(x) lm_head^T (untied), softmax-xent fused

Parameter names follow the common fused-projection layout:
``model.embed_tokens.weight``, ``model.layers.{i}.{input_layernorm,post_attention_layernorm}.weight``,
``model.layers.{i}.self_attn.{qkv_proj,o_proj}.weight``, ``model.layers.{i}.mlp.{gate_up_proj,down_proj}.weight``,
``model.norm.weight``, ``lm_head.weight``.  RMSNorm / RoPE / SwiGLU / causal-GQA attention / xent
run as dltb HIP kernels on the GPU.

With ``cfg.n_experts`` the FFN is a top-k mixture of experts with a fixed capacity per expert (``_moe_fwd`` /
``_moe_bwd``, csrc/moe.hip): ``mlp`` then holds ``router.weight`` and ``experts.{e}.{gate_up_proj,down_proj}.weight``.
With ``cfg.moe_aux_loss_coef`` / ``cfg.moe_z_loss_coef`` every layer also returns its (load-balancing, router-z) pair and
the loss is ``lm_loss + a sum_layers balance + b sum_layers z`` (ops/ref.py ``moe_aux_fwd``), on the rank's local rows.
With ``cfg.moe_dropless`` there is no capacity: the experts' rows are packed into 128-aligned segments and run as
grouped GEMMs that read the segment bounds on the device (``_moe_fwd_dropless``, csrc/gemm_grouped.hip).

With ``cfg.qk_norm`` every query head and every key head goes through an RMSNorm over ``head_dim`` before RoPE, with
one learned [head_dim] weight for q and one for k per layer: ``self_attn.{q_norm,k_norm}.weight``, the LAST two
entries of the layer's parameter list.  Norm and RoPE are one in-place pass (``qknorm_rope_fwd`` / ``_bwd_``,
csrc/qknorm.hip) where the flag-off path runs ``rope_``; the forward keeps ``raw``, the q|k columns before the norm.

With ``cfg.attn_sinks`` every query head has one learned sink logit per layer, ``self_attn.sinks`` [n_head], the LAST
entry of the layer's parameter list (after the QK-norm pair when both are on).  It joins the softmax denominator of
every query row and carries no value (``attn_fwd(..., sink=)``: the forward kernel's epilogue); o and lse include it,
so nothing more is kept for the backward, whose kernels run unchanged; ``attn_bwd(..., sink=)`` adds one small
reduction kernel whose fp32 partials reach the gradient slot with the layer's norm partials.

With ``cfg.attn_softcap`` = cap > 0 every attention score x becomes ``cap * tanh(x / cap)`` before the masks and the
softmax (``attn_fwd`` / ``attn_bwd(..., softcap=)``: the CAP kernels of csrc/attention.hip) on every attention path --
the whole row, the context-parallel ranges and both recompute modes.  It adds no parameter and keeps nothing more for
the backward: lse is that of the capped scores and the backward kernels recompute the tanh.

With ``cfg.final_softcap`` = C > 0 the head's loss is formed from ``c = C * tanh(logits / C)`` and with
``cfg.lm_z_loss_coef`` = B > 0 it gains ``B * logsumexp(c)^2`` per valid row (``xent_fwd_bwd_`` / ``xent_lse`` /
``xent_bwd_lse_(..., softcap=, z_coef=)``: the option kernels of csrc/xent.hip), unchunked and under ``head_chunk``.
c exists in fp32 registers only; the row mean, the 1 / count scale and what the backward keeps are unchanged (the
kept lse is that of c).  The logits handed back to a caller are the capped ones, rounded to the model's format.

With ``cfg.sandwich_norm`` every sublayer's output goes through its own RMSNorm before it joins the residual stream,
``x1 = x + RMSNorm(a; self_attn.out_norm)`` and ``x2 = x1 + RMSNorm(m; mlp.out_norm)`` (m: the dense FFN's output or the
MoE combine), on top of the two pre-norms.  The two [n_embd] weights sit in the layer's parameter list after the
QK-norm pair and before the sinks.  The attention site is one launch with the next pre-norm (``sandwich_fwd`` /
``sandwich_bwd``, csrc/sandwich_norm.hip); the FFN site's forward is the same kernel without the second norm and its
backward a plain ``norm_bwd``.  The layer keeps a, m and their two rstd rows in addition.

With ``cfg.ffn_act = "geglu"`` the gated FFN is ``gelu_tanh(gate) * up`` (``swiglu_fwd`` / ``_bwd`` / ``_bwd_h(...,
act=)``: the GEGLU instantiations of csrc/elementwise.hip) on the dense path, the recompute path and both MoE routings.
"""
import math

import torch
import torch.nn as nn

from ..ops import functional as F_
from ..ops import ref
from ..parallel.runtime import EAGER, Unit
from .config import ModelConfig


class _RMSNorm(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))


class _Attn(nn.Module):
    def __init__(self, d, kvd, qk_norm_dim=None, n_sinks=None):
        super().__init__()
        self.qkv_proj = nn.Linear(d, d + 2 * kvd, bias=False)
        self.o_proj = nn.Linear(d, d, bias=False)
        if qk_norm_dim:         # QK-norm: one [head_dim] weight for the query heads, one for the key heads
            self.q_norm = _RMSNorm(qk_norm_dim)
            self.k_norm = _RMSNorm(qk_norm_dim)
        if n_sinks:             # attention sinks: one raw logit per query head
            self.sinks = nn.Parameter(torch.zeros(n_sinks))


class _MLP(nn.Module):
    def __init__(self, d, f):
        super().__init__()
        self.gate_up_proj = nn.Linear(d, 2 * f, bias=False)
        self.down_proj = nn.Linear(f, d, bias=False)


class _MoE(nn.Module):
    """``cfg.n_experts`` SwiGLU FFNs behind a top-k router (the layer's ``mlp`` when ``n_experts`` is set)."""

    def __init__(self, d, f, n_experts):
        super().__init__()
        self.router = nn.Linear(d, n_experts, bias=False)
        self.experts = nn.ModuleList([_MLP(d, f) for _ in range(n_experts)])


class MistralLayer(nn.Module):
    def __init__(self, cfg: ModelConfig):
        super().__init__()
        d = cfg.n_embd
        self.input_layernorm = _RMSNorm(d)
        self.self_attn = _Attn(d, cfg.kv_heads * cfg.head_dim, cfg.head_dim if cfg.qk_norm else None,
                               cfg.n_head if cfg.attn_sinks else None)
        self.qk_norm = cfg.qk_norm
        self.attn_sinks = cfg.attn_sinks
        self.sandwich_norm = cfg.sandwich_norm
        self.post_attention_layernorm = _RMSNorm(d)
        self.mlp = _MoE(d, cfg.ffn_dim, cfg.n_experts) if cfg.n_experts else _MLP(d, cfg.ffn_dim)
        if cfg.sandwich_norm:   # sandwich norms: one RMSNorm on the attention sublayer's output, one on the FFN's
            self.self_attn.out_norm = _RMSNorm(d)
            self.mlp.out_norm = _RMSNorm(d)

    def param_list(self):
        # the QK-norm weights, then the sandwich norms' pair and then the sinks come last, so the dense (4, 5) and MoE
        # (4, 5 + 2e, 6 + 2e) indices hold with them
        tail = []
        if self.qk_norm:
            tail = [("self_attn.q_norm.weight", self.self_attn.q_norm.weight),
                    ("self_attn.k_norm.weight", self.self_attn.k_norm.weight)]
        if self.sandwich_norm:
            tail = tail + [("self_attn.out_norm.weight", self.self_attn.out_norm.weight),
                           ("mlp.out_norm.weight", self.mlp.out_norm.weight)]
        if self.attn_sinks:
            tail = tail + [("self_attn.sinks", self.self_attn.sinks)]
        head = [("input_layernorm.weight", self.input_layernorm.weight),
                ("self_attn.qkv_proj.weight", self.self_attn.qkv_proj.weight),
                ("self_attn.o_proj.weight", self.self_attn.o_proj.weight),
                ("post_attention_layernorm.weight", self.post_attention_layernorm.weight)]
        if isinstance(self.mlp, _MoE):      # the router, then every expert's pair: parameters 4, 5 + 2e, 6 + 2e
            moe = [("mlp.router.weight", self.mlp.router.weight)]
            for e, ex in enumerate(self.mlp.experts):
                moe += [(f"mlp.experts.{e}.gate_up_proj.weight", ex.gate_up_proj.weight),
                        (f"mlp.experts.{e}.down_proj.weight", ex.down_proj.weight)]
            return head + moe + tail
        return head + [("mlp.gate_up_proj.weight", self.mlp.gate_up_proj.weight),
                       ("mlp.down_proj.weight", self.mlp.down_proj.weight)] + tail


class _EmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, idx, model):
        rt, unit = model.rt, model.unit_embed
        (wte,) = rt.acquire(unit)
        x = wte.index_select(0, idx.reshape(-1))
        rt.release_forward(unit)
        ctx.model, ctx.idx = model, idx
        return x

    @staticmethod
    def backward(ctx, dx):
        model = ctx.model
        rt, unit = model.rt, model.unit_embed
        rt.acquire_backward(unit)
        rt.embedding_backward((unit, 0), None, dx.contiguous(), ctx.idx, 0.0, rt.seed, 0)
        rt.grads_ready(unit)
        rt.release_backward(unit)
        return None, None, None


def _n_block_weights(cfg, ws):
    """How many of a layer's parameters ``ws`` come before its tail -- the QK-norm pair, then the sandwich norms'
    pair, then the sinks -- that is the norms, projections and the FFN."""
    return len(ws) - (2 if cfg.qk_norm else 0) - (2 if cfg.sandwich_norm else 0) - (1 if cfg.attn_sinks else 0)


def _attn_tail(cfg, ws):
    """(nb, qkn, sink) of a layer's parameters ``ws``: :func:`_n_block_weights`, the QK-norm pair (q weight, k weight)
    at nb, nb + 1 or None, and the sinks (the last parameter) or None."""
    nb = _n_block_weights(cfg, ws)
    return nb, (tuple(ws[nb:nb + 2]) if cfg.qk_norm else None), (ws[-1] if cfg.attn_sinks else None)


def _out_norm_index(cfg, ws):
    """The index in ``ws`` of ``self_attn.out_norm.weight`` (``mlp.out_norm.weight`` follows it) under
    ``cfg.sandwich_norm`` -- after the QK-norm pair, before the sinks -- else None."""
    if not cfg.sandwich_norm:
        return None
    return _n_block_weights(cfg, ws) + (2 if cfg.qk_norm else 0)


def _ffn_out_fwd(cfg, x1, m, w_ffn_out, seed):
    """x2 and rstd_m: the FFN output ``m`` joins the residual stream, through its out-norm under ``cfg.sandwich_norm``
    (``w_ffn_out``; the kernel's form without a second norm), else by the plain add (rstd_m None)."""
    if w_ffn_out is None:
        return F_.dropout(x1, m, 0.0, seed, 0), None
    x2, _, rstd_m, _ = F_.sandwich_fwd(x1, m, w_ffn_out, None, cfg.norm_eps)
    return x2, rstd_m


def _rope_fwd(model, qkv, T, Hq, Hkv, D, qkn):
    """RoPE in place on the q|k columns of ``qkv`` (rows of T positions); with ``qkn`` = (wq, wk) the fused
    QK-norm + RoPE pass instead.  Returns ``raw`` (None without QK-norm)."""
    cos, sin = model.rope(qkv.device, T)
    if qkn is None:
        F_.rope_(qkv, cos, sin, T, Hq + Hkv, D, False)
        return None
    return F_.qknorm_rope_fwd(qkv, qkn[0], qkn[1], cos, sin, T, Hq, Hkv, D, model.cfg.norm_eps)


def _rope_bwd(model, dqkv, T, Hq, Hkv, D, qkn, raw, sq, sk, red):
    """The backward of :func:`_rope_fwd`, in place on the q|k columns of ``dqkv``: the inverse rotation (RoPE is
    orthogonal: grad = R(-theta) g), with QK-norm the fused backward, whose weight-gradient partials go to the
    gradient slots ``sq`` / ``sk`` ((tensor, accumulate) each) through ``red`` with the layer's norm partials."""
    cos, sin = model.rope(dqkv.device, T)
    if qkn is None:
        F_.rope_(dqkv, cos, sin, T, Hq + Hkv, D, True)
        return
    pq, pk = F_.qknorm_rope_bwd_(dqkv, raw, qkn[0], qkn[1], cos, sin, T, Hq, Hkv, D, model.cfg.norm_eps)
    F_.reduce_partials(red, pq, sq[0], sq[1])
    F_.reduce_partials(red, pk, sk[0], sk[1])


def _cp_rope_gather(model, qkv, Hq, Hkv, D, qkn=None):
    """The part of the context-parallel attention forward before its kernels: RoPE in place with each range's
    positions, then the all-gather of K | V into position order.  Returns (kv, raw).  Also the backward's
    re-gather under ``activation_recompute = "full"``, which does not keep kv.  With ``qkn`` = (wq, wk) each range
    runs the fused QK-norm + RoPE pass with its own cos / sin rows (the keys are normalised before the gather) and
    ``raw`` is the ranges' q|k columns before it, range-major like ``qkv``; else ``raw`` is None."""
    cp = model.cp
    B, T = model._cur_full_bt
    n = qkv.shape[0] // len(cp.ranges(T))
    cos, sin = model.rope(qkv.device, T)
    raws = []
    for j, (c, s_) in enumerate(cp.rope_rows(cos, sin, T)):
        if qkn is None:
            F_.rope_(qkv[j * n:(j + 1) * n], c, s_, n // B, Hq + Hkv, D, False)
        else:
            raws.append(F_.qknorm_rope_fwd(qkv[j * n:(j + 1) * n], qkn[0], qkn[1], c, s_, n // B, Hq, Hkv, D,
                                           model.cfg.norm_eps))
    # waits for the gather: the kernels read it
    return cp.gather_kv(qkv[:, Hq * D:], B, T), (raws if raws else None)


def _cp_attn_fwd(model, qkv, Hq, Hkv, D, window, bounds, seed, qkn=None, sink=None):
    """Context-parallel attention forward (parallel/context.py): RoPE with each range's positions, all-gather of
    K | V into position order, then the range kernels -- the local queries of each range against all T keys.
    ``qkv`` holds the local tokens range-major, so a range's rows are one block.  Returns (o, lse per range, kv,
    raw); ``qkn`` / ``raw``: :func:`_cp_rope_gather`; ``sink``: the layer's attention sinks for every range's call."""
    cp = model.cp
    B, T = model._cur_full_bt
    rngs = cp.ranges(T)
    n = qkv.shape[0] // len(rngs)
    qd, kd = Hq * D, Hkv * D
    kv, raw = _cp_rope_gather(model, qkv, Hq, Hkv, D, qkn)
    o = torch.empty(qkv.shape[0], qd, dtype=qkv.dtype, device=qkv.device)
    lses = []
    for j, rng in enumerate(rngs):
        _, lse, _ = F_.attn_fwd(qkv[j * n:(j + 1) * n, :qd], kv[:, :kd], kv[:, kd:], B, T, Hq, Hkv,
                                1.0 / math.sqrt(D), True, 0.0, seed, 0, o_out=o[j * n:(j + 1) * n],
                                window=window, bounds=bounds, q_range=rng, sink=sink,
                                softcap=model.cfg.attn_softcap)
        lses.append(lse)
    return o, lses, kv, raw


def _cp_attn_bwd(model, qkv, kv, o, do, lses, dqkv, Hq, Hkv, D, window, bounds, seed, qkn=None, raw=None, sq=None,
                 sk=None, red=None, sink=None, ss=None):
    """The backward of :func:`_cp_attn_fwd`: dQ of each range into its rows of ``dqkv``; each range's dK | dV
    over all T rows (zero where its queries see nothing), the zigzag pair summed by one add; reduce-scatter over
    the group into the local K | V columns of ``dqkv``; then the inverse RoPE of the local rows as without
    context parallelism.  With ``qkn`` = (wq, wk) the fused QK-norm + RoPE backward runs per range instead (``raw``:
    the forward's list); the ranges' weight-gradient partials fill one partial matrix per weight, so the later
    ranges' sums accumulate onto the first's in the one fixed-order reduction into the slot ``sq`` / ``sk``.  With
    ``sink`` each range's call writes its own rows of one sink-gradient partial matrix, reduced once into ``ss``."""
    cp = model.cp
    B, T = model._cur_full_bt
    rngs = cp.ranges(T)
    n = qkv.shape[0] // len(rngs)
    qd, kd = Hq * D, Hkv * D
    dkv = None
    spart, Gs = None, 0
    if sink is not None:
        Gs = F_.attn_sink_partials(dqkv, B, n // B)
        spart = torch.empty(len(rngs) * Gs, Hq, dtype=torch.float32, device=dqkv.device)
    for j, rng in enumerate(rngs):
        part = torch.empty_like(kv)
        blk = slice(j * n, (j + 1) * n)
        F_.attn_bwd(qkv[blk, :qd], kv[:, :kd], kv[:, kd:], o[blk], do[blk], lses[j], None, dqkv[blk, :qd],
                    part[:, :kd], part[:, kd:], B, T, Hq, Hkv, 1.0 / math.sqrt(D), True, 0.0, seed, 0,
                    window=window, bounds=bounds, q_range=rng, sink=sink, part_out=spart, g_off=j * Gs,
                    softcap=model.cfg.attn_softcap)
        dkv = part if dkv is None else dkv.add_(part)
    if sink is not None:
        F_.reduce_partials(red, spart, ss[0], ss[1])
    cp.scatter_dkv(dkv, dqkv[:, qd:], B, T)       # waits for the reduce-scatter: the inverse RoPE reads it
    cos, sin = model.rope(qkv.device, T)
    if qkn is not None:
        G = F_.qknorm_partials(dqkv, n)
        part = torch.empty(2, len(rngs) * G, D, dtype=torch.float32, device=dqkv.device)
    for j, (c, s_) in enumerate(cp.rope_rows(cos, sin, T)):
        if qkn is None:
            F_.rope_(dqkv[j * n:(j + 1) * n], c, s_, n // B, Hq + Hkv, D, True)
        else:
            F_.qknorm_rope_bwd_(dqkv[j * n:(j + 1) * n], raw[j], qkn[0], qkn[1], c, s_, n // B, Hq, Hkv, D,
                                model.cfg.norm_eps, part_out=part, g_off=j * G)
    if qkn is not None:
        F_.reduce_partials(red, part[0], sq[0], sq[1])
        F_.reduce_partials(red, part[1], sk[0], sk[1])


class _LayerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, model, i):
        rt, unit = model.rt, model.unit_blocks[i]
        cfg = model.cfg
        ctx.recompute = _check_recompute(model.activation_recompute)
        if cfg.n_experts and ctx.recompute != "off":
            raise ValueError("--activation-recompute is not supported together with --moe-experts "
                             f"(activation_recompute = {ctx.recompute!r}, n_experts = {cfg.n_experts})")
        ws = rt.acquire(unit)
        (w_in, wqkv, wo, w_post) = ws[:4]
        nb, qkn, sink = _attn_tail(cfg, ws)      # (q weight, k weight) of QK-norm; the attention sinks
        B, T = model._cur_bt
        Hq, Hkv, D = cfg.n_head, cfg.kv_heads, cfg.head_dim
        _, h1, _, rstd1 = F_.norm_fwd(x, None, w_in, None, cfg.norm_eps, True)
        qkv = F_.linear_fwd(h1, wqkv)
        qd, kd = Hq * D, Hkv * D
        # document mask: the forward's bounds (window folded in) replace the window, and stay for the backward
        bounds = model._cur_bounds
        window = 0 if bounds is not None else cfg.sliding_window or 0
        if model.cp is not None:      # context parallel: local queries against the group's gathered K | V
            o, lse, aux, raw = _cp_attn_fwd(model, qkv, Hq, Hkv, D, window, bounds, rt.seed, qkn, sink)
        else:
            raw = _rope_fwd(model, qkv, T, Hq, Hkv, D, qkn)
            o, lse, aux = F_.attn_fwd(qkv[:, :qd], qkv[:, qd:qd + kd], qkv[:, qd + kd:], B, T, Hq, Hkv,
                                      1.0 / math.sqrt(D), True, 0.0, rt.seed, 0, window=window, bounds=bounds,
                                      sink=sink, softcap=cfg.attn_softcap)
        a = F_.linear_fwd(o, wo)
        jo = _out_norm_index(cfg, ws)            # sandwich norms: ws[jo] the attention site's, ws[jo + 1] the FFN's
        if jo is None:
            x1, h2, _, rstd2 = F_.norm_fwd(x, a, w_post, None, cfg.norm_eps, True)
            rstd_a = None
        else:                   # x1 = x + RMSNorm(a) and h2 = RMSNorm(x1) in one launch
            x1, h2, rstd_a, rstd2 = F_.sandwich_fwd(x, a, ws[jo], w_post, cfg.norm_eps)
        ctx.moe = None
        router_losses = None
        if cfg.n_experts:       # top-k routed experts instead of the dense FFN; gu / hh are per expert, in ctx.moe
            m, ctx.moe, *rest = _moe_fwd(model, i, h2, ws[4:nb])
            gu = hh = None
            if rest:            # the layer's (balance, z): a second, differentiable output (not kept on ctx)
                router_losses = rest[0]
        else:
            wgu, wd = ws[4:6]
            gu = F_.linear_fwd(h2, wgu)
            hh = F_.swiglu_fwd(gu, cfg.ffn_act)
            m = F_.linear_fwd(hh, wd)
        x2, rstd_m = _ffn_out_fwd(cfg, x1, m, None if jo is None else ws[jo + 1], rt.seed)
        rt.release_forward(unit)
        ctx.model, ctx.i = model, i
        # sandwich norms: the two sublayer outputs and their row statistics; "full" rebuilds a (and with it rstd_a)
        ctx.sand = None
        if jo is not None:
            ctx.sand = (None, None, m, rstd_m) if ctx.recompute == "full" else (a, rstd_a, m, rstd_m)
        # raw: the q|k columns before QK-norm (None without it)
        ctx.saved = (x, h1, rstd1, qkv, o, lse, aux, x1, h2, rstd2, gu, hh, raw)
        if ctx.recompute == "selective":      # the backward rebuilds h1, h2 (norm_apply) and hh (swiglu_bwd_h)
            ctx.saved = (x, None, rstd1, qkv, o, lse, aux, x1, None, rstd2, gu, None, raw)
        elif ctx.recompute == "full":         # ... and everything else but the attention output
            ctx.saved = (x, None, None, None, o, lse, None, None, None, None, None, None, None)
        ctx.bounds = bounds
        return x2 if router_losses is None else (x2, router_losses)

    @staticmethod
    def backward(ctx, dx2, daux=None):
        if ctx.recompute != "off":
            return _layer_backward_recompute(ctx, dx2), None, None
        model, i = ctx.model, ctx.i
        rt, unit = model.rt, model.unit_blocks[i]
        (x, h1, rstd1, qkv, o, lse, aux, x1, h2, rstd2, gu, hh, raw) = ctx.saved
        ctx.saved = None
        ws = rt.acquire_backward(unit)
        (w_in, wqkv, wo, w_post) = ws[:4]
        cfg = model.cfg
        nb, qkn, sink = _attn_tail(cfg, ws)
        B, T = model._cur_bt
        Hq, Hkv, D = cfg.n_head, cfg.kv_heads, cfg.head_dim
        dx2 = dx2.contiguous()
        s = [rt.grad_slot(unit, j) for j in range(len(ws))]
        shared = rt.grad_reducer()
        red = shared if shared is not None else F_.GradReducer()
        jo = _out_norm_index(cfg, ws)
        dm = dx2                # the gradient of the FFN output m: through the FFN site's out-norm under sandwich norms
        if jo is not None:
            a, rstd_a, m, rstd_m = ctx.sand
            ctx.sand = None
            dm = F_.norm_bwd(dx2, m, ws[jo + 1], None, rstd_m, None, s[jo + 1][0], None, s[jo + 1][1], True, red=red)
            del m
        if ctx.moe is not None:
            dh2 = _moe_bwd(model, unit, dm, h2, ws[:nb], s[:nb], ctx.moe, daux)
            ctx.moe = None
        else:
            wgu, wd = ws[4:6]
            F_.linear_wgrad(dm, hh, s[5][0], None, s[5][1])
            dhh = F_.linear_dgrad(dm, wd, rt.weight_t(unit, 5, wd))
            dgu = F_.swiglu_bwd(dhh, gu, cfg.ffn_act)
            F_.linear_wgrad(dgu, h2, s[4][0], None, s[4][1])
            dh2 = F_.linear_dgrad(dgu, wgu, rt.weight_t(unit, 4, wgu))
        if jo is None:
            dx1 = F_.norm_bwd(dh2, x1, w_post, None, rstd2, dx2, s[3][0], None, s[3][1], True, red=red)
            da = dx1
        else:                   # dx1 = dx2 + the pre-norm's backward, da = the attention site's out-norm backward of dx1
            dx1, da = F_.sandwich_bwd(dh2, x1, w_post, rstd2, dx2, a, ws[jo], rstd_a, s[3], s[jo], red)
        F_.linear_wgrad(da, o, s[2][0], None, s[2][1])
        do = F_.linear_dgrad(da, wo, rt.weight_t(unit, 2, wo))
        qd, kd = Hq * D, Hkv * D
        dqkv = torch.empty_like(qkv)
        window = 0 if ctx.bounds is not None else cfg.sliding_window or 0
        if model.cp is not None:      # aux: the gathered K | V of the forward
            _cp_attn_bwd(model, qkv, aux, o, do, lse, dqkv, Hq, Hkv, D, window, ctx.bounds, rt.seed, qkn, raw,
                         s[nb] if qkn else None, s[nb + 1] if qkn else None, red, sink, s[-1])
        else:
            dsink = F_.attn_bwd(qkv[:, :qd], qkv[:, qd:qd + kd], qkv[:, qd + kd:], o, do, lse, aux,
                                dqkv[:, :qd], dqkv[:, qd:qd + kd], dqkv[:, qd + kd:], B, T, Hq, Hkv,
                                1.0 / math.sqrt(D), True, 0.0, rt.seed, 0, window=window, bounds=ctx.bounds,
                                sink=sink, softcap=cfg.attn_softcap)
            if sink is not None:      # the sink-gradient partials join the layer's norm partials
                F_.reduce_partials(red, dsink, s[-1][0], s[-1][1])
            _rope_bwd(model, dqkv, T, Hq, Hkv, D, qkn, raw, s[nb] if qkn else None, s[nb + 1] if qkn else None, red)
        ctx.bounds = None
        F_.linear_wgrad(dqkv, h1, s[1][0], None, s[1][1])
        dh1 = F_.linear_dgrad(dqkv, wqkv, rt.weight_t(unit, 1, wqkv))
        dx = F_.norm_bwd(dh1, x, w_in, None, rstd1, dx1, s[0][0], None, s[0][1], True, red=red)
        if shared is None:
            red.flush()
        rt.grads_ready(unit)
        rt.release_backward(unit)
        return dx, None, None


def _moe_fwd(model, i, h2, ws):
    """The routed FFN of layer ``i`` on the rows ``h2`` [N, d]; ``ws``: the router, then (gate_up, down) per expert.
    Route (top-k, softmax gates), assign slots (fixed capacity C per expert, row-major order, overflow dropped),
    gather the rows into ``xe`` [E C, d], run each expert's SwiGLU FFN on its [C, d] slab with the dense path's
    GEMM calls, and combine.  Every shape is static.  Returns (m, what the backward needs).  With an auxiliary loss
    on (``cfg.moe_aux_on``) the backward's tuple has three more entries -- the router logits, their log-sum-exp and the
    layer's own copy of the counts -- and a third value is returned: the [2] tensor (balance, z), which also goes to
    row ``i`` of ``model.moe_aux``."""
    cfg = model.cfg
    if cfg.moe_dropless:
        return _moe_fwd_dropless(model, i, h2, ws)
    E, K = cfg.n_experts, cfg.moe_top_k
    C = ref.moe_capacity(h2.shape[0], E, K, cfg.moe_capacity_factor)
    expert, gate, logits = F_.moe_route(h2, ws[0], K)
    extra = ()
    if cfg.moe_aux_on:
        # the backward reads the counts again (f in moe_aux_bwd_), and the model's row i is overwritten by the next
        # forward, which may come before this one's backward: the layer keeps a tensor of its own, at the price of one
        # small copy launch that fills the model's row for the record
        slot, src, _, counts = F_.moe_assign(expert, E, C)
        model.moe_counts(h2.device)[i].copy_(counts)
        lse, aux = F_.moe_aux_fwd(logits, counts, K, model.moe_aux(h2.device)[i])
        extra = (logits, lse, counts)
    else:
        slot, src, _, _ = F_.moe_assign(expert, E, C, model.moe_counts(h2.device)[i])
    del logits
    xe = F_.moe_dispatch(h2, src)
    ye = torch.empty_like(xe)
    gus, hhs = [], []
    for e in range(E):
        rows = slice(e * C, (e + 1) * C)
        gu = F_.linear_fwd(xe[rows], ws[1 + 2 * e])
        hh = F_.swiglu_fwd(gu, cfg.ffn_act)
        ye[rows].copy_(F_.linear_fwd(hh, ws[2 + 2 * e]))
        gus.append(gu)
        hhs.append(hh)
    m = F_.moe_combine(ye, slot, gate)
    saved = (expert, gate, slot, src, xe, ye, gus, hhs, C) + extra
    return (m, saved, aux) if extra else (m, saved)


def _moe_bwd(model, unit, dm, h2, ws, s, saved, daux=None):
    """The backward of :func:`_moe_fwd`, in gather form throughout: returns dh2 and writes the router's and every
    expert's weight gradient into its slot (``ws`` / ``s``: the unit's parameters and gradient slots; the router is
    parameter 4, expert e's pair 5 + 2e and 6 + 2e).  An expert without tokens sees zero slabs, so its gradients
    are exact zeros.  ``daux``: the gradient of the layer's (balance, z) when an auxiliary loss is on; its term is
    added to the dense dlogits before the router's two gradient kernels read them."""
    rt = model.rt
    (expert, gate, slot, src, xe, ye, gus, hhs, C) = saved[:9]
    E = model.cfg.n_experts
    dye, _, dlogits = F_.moe_combine_bwd(dm, ye, slot, src, expert, gate, E)
    del ye
    dense = len(saved) > 9
    if dense:
        logits, lse, counts = saved[9:]
        g = torch.zeros(2, dtype=logits.dtype, device=logits.device) if daux is None \
            else daux.to(logits.dtype).contiguous()
        F_.moe_aux_bwd_(dlogits, logits, lse, counts, g, model.cfg.moe_top_k)
        del logits, lse, counts
    if model.cfg.moe_dropless:
        dxe = _moe_experts_bwd_dropless(rt, unit, dye, ws, s, saved, model.cfg.ffn_act)
        F_.moe_router_wgrad(dlogits, h2, s[4][0], s[4][1], dense=dense)
        return F_.moe_dispatch_bwd(dxe, slot, dlogits, ws[4])
    dxe = torch.empty_like(xe)
    for e in range(E):
        rows = slice(e * C, (e + 1) * C)
        ju, jd = 5 + 2 * e, 6 + 2 * e
        wgu, wd = ws[ju], ws[jd]
        F_.linear_wgrad(dye[rows], hhs[e], s[jd][0], None, s[jd][1])
        dhh = F_.linear_dgrad(dye[rows], wd, rt.weight_t(unit, jd, wd))
        dgu = F_.swiglu_bwd(dhh, gus[e], model.cfg.ffn_act)
        gus[e] = hhs[e] = None
        F_.linear_wgrad(dgu, xe[rows], s[ju][0], None, s[ju][1])
        dxe[rows].copy_(F_.linear_dgrad(dgu, wgu, rt.weight_t(unit, ju, wgu)))
    F_.moe_router_wgrad(dlogits, h2, s[4][0], s[4][1], dense=dense)
    return F_.moe_dispatch_bwd(dxe, slot, dlogits, ws[4])


def _moe_fwd_dropless(model, i, h2, ws):
    """:func:`_moe_fwd` with ``cfg.moe_dropless``: the same router, gates, tie rule, row-major order and combine, but
    no capacity.  The assignments of expert e fill the segment [offsets[e], offsets[e + 1]) of one packed row space of
    R = ``ref.moe_dropless_rows`` rows (128-aligned segments, static R), ``xe`` is [R, d], and the experts run as
    two grouped GEMMs (gate|up on [R, 2f], down written straight into ``ye``) that read ``offsets`` on the device, so
    a captured step replays with any routing.  Padding and tail rows are zero in ``xe`` and stay zero through SwiGLU.
    The backward's tuple has ``gu`` / ``hh`` as single [R, .] tensors and ``offsets`` in place of C."""
    cfg = model.cfg
    E, K = cfg.n_experts, cfg.moe_top_k
    expert, gate, logits = F_.moe_route(h2, ws[0], K)
    extra = ()
    if cfg.moe_aux_on:          # the layer keeps its own counts for the backward: see _moe_fwd
        slot, src, _, counts, offsets = F_.moe_assign_dropless(expert, E)
        model.moe_counts(h2.device)[i].copy_(counts)
        lse, aux = F_.moe_aux_fwd(logits, counts, K, model.moe_aux(h2.device)[i])
        extra = (logits, lse, counts)
    else:
        slot, src, _, _, offsets = F_.moe_assign_dropless(expert, E, model.moe_counts(h2.device)[i])
    del logits
    xe = F_.moe_dispatch(h2, src)
    gu = F_.gemm_grouped_nt(xe, offsets, [ws[1 + 2 * e] for e in range(E)])
    hh = F_.swiglu_fwd(gu, cfg.ffn_act)
    ye = F_.gemm_grouped_nt(hh, offsets, [ws[2 + 2 * e] for e in range(E)])
    m = F_.moe_combine(ye, slot, gate)
    saved = (expert, gate, slot, src, xe, ye, gu, hh, offsets) + extra
    return (m, saved, aux) if extra else (m, saved)


def _moe_weights_t(rt, unit, ws, js):
    """W^T of the parameters ``js`` of ``unit`` for a grouped data-gradient product: the engine's cached transposes
    where it keeps them (``rt.weight_t``), else copies made here with ``transpose_into`` into one scratch tensor
    [len(js), in, out] that lives until the product has run (engines whose parameters do not stay resident)."""
    wts = [rt.weight_t(unit, j, ws[j]) for j in js]
    if all(t is not None for t in wts):
        return wts
    w0 = ws[js[0]]
    buf = torch.empty(len(js), w0.shape[1], w0.shape[0], dtype=w0.dtype, device=w0.device)
    for t, j in zip(buf, js):
        F_.transpose_into(ws[j], t)
    return list(buf)


def _moe_experts_bwd_dropless(rt, unit, dye, ws, s, saved, act="swiglu"):
    """The experts' part of :func:`_moe_bwd` on the packed layout: two grouped TN products write every expert's two
    weight gradients into their slots (an expert without rows gets exact zeros, or keeps its slot when accumulating)
    and two grouped NT products on W^T give the data gradients -- four launches instead of 4 E GEMM calls and 2 E
    slab copies.  Returns dxe [R, d] (zero in the padding and tail rows)."""
    xe, gu, hh, offsets = saved[4], saved[6], saved[7], saved[8]
    E = (len(ws) - 5) // 2
    ju, jd = [5 + 2 * e for e in range(E)], [6 + 2 * e for e in range(E)]
    F_.gemm_grouped_tn(dye, hh, offsets, [s[j][0] for j in jd], [s[j][1] for j in jd])
    dhh = F_.gemm_grouped_nt(dye, offsets, _moe_weights_t(rt, unit, ws, jd))
    dgu = F_.swiglu_bwd(dhh, gu, act)
    del dhh
    F_.gemm_grouped_tn(dgu, xe, offsets, [s[j][0] for j in ju], [s[j][1] for j in ju])
    return F_.gemm_grouped_nt(dgu, offsets, _moe_weights_t(rt, unit, ws, ju))


RECOMPUTE_MODES = ("off", "selective", "full")


def _check_recompute(mode):
    if mode not in RECOMPUTE_MODES:
        raise ValueError(f"activation_recompute must be one of {', '.join(RECOMPUTE_MODES)}, got {mode!r}")
    return mode


def _layer_backward_recompute(ctx, dx2):
    """:meth:`_LayerFn.backward` for a forward that kept a reduced set (``model.activation_recompute``):

    * ``selective`` kept everything but the norm outputs h1, h2 and the SwiGLU output hh; they come back from
      elementwise kernels (``norm_apply`` from the kept row statistics, ``swiglu_bwd_h`` inside the SwiGLU backward).
    * with QK-norm both modes treat ``raw`` like qkv: ``selective`` keeps it, ``full`` rebuilds it with qkv.
    * attention sinks keep nothing more in either mode: the kept o and lse already include the sink; nor does
      ``attn_softcap`` (the kept lse is that of the capped scores).
    * sandwich norms: both modes also hold the FFN output m and its rstd row (the down projection is never re-run);
      ``selective`` keeps a and its rstd row too, ``full`` rebuilds them with x1 / h2 / rstd2 (``sandwich_fwd``).
    * ``full`` kept x, o, lse.  The MLP half (a = o Wo^T, x1 / h2 / rstd2, gu) is rebuilt first and the attention
      half (h1 / rstd1, qkv + RoPE, under context parallelism the gathered K | V) only when the MLP half has been
      consumed and freed, so the rebuilt working set is half a layer's.  Attention itself and the down projection
      are not re-run.

    Every rebuilt tensor is the forward's bit for bit (same kernels on the same inputs; hash-seeded randomness),
    the gradient kernels are ``off``'s with ``swiglu_bwd`` replaced by ``swiglu_bwd_h`` (the wd weight gradient
    moves behind it), and each tensor is dropped after its last consumer."""
    model, i = ctx.model, ctx.i
    full = ctx.recompute == "full"
    rt, unit = model.rt, model.unit_blocks[i]
    (x, _, rstd1, qkv, o, lse, aux, x1, _, rstd2, gu, _, raw) = ctx.saved
    ctx.saved = None
    ws = rt.acquire_backward(unit)
    (w_in, wqkv, wo, w_post, wgu, wd) = ws[:6]
    cfg = model.cfg
    nb, qkn, sink = _attn_tail(cfg, ws)     # dense layer: nb = 6; the QK-norm pair at 6, 7, the sinks last
    B, T = model._cur_bt
    Hq, Hkv, D = cfg.n_head, cfg.kv_heads, cfg.head_dim
    qd, kd = Hq * D, Hkv * D
    dx2 = dx2.contiguous()
    s = [rt.grad_slot(unit, j) for j in range(len(ws))]
    sq, sk = (s[nb], s[nb + 1]) if qkn else (None, None)
    shared = rt.grad_reducer()
    red = shared if shared is not None else F_.GradReducer()
    jo = _out_norm_index(cfg, ws)
    a = rstd_a = None
    if jo is not None:
        a, rstd_a, m, rstd_m = ctx.sand
        ctx.sand = None
    # ---- MLP half
    if full:
        a = F_.linear_fwd(o, wo)
        if jo is None:
            x1, h2, _, rstd2 = F_.norm_fwd(x, a, w_post, None, cfg.norm_eps, True)
            a = None
        else:
            x1, h2, rstd_a, rstd2 = F_.sandwich_fwd(x, a, ws[jo], w_post, cfg.norm_eps)
        gu = F_.linear_fwd(h2, wgu)
    else:
        h2 = F_.norm_apply(x1, w_post, None, None, rstd2, True)
    dm = dx2
    if jo is not None:
        dm = F_.norm_bwd(dx2, m, ws[jo + 1], None, rstd_m, None, s[jo + 1][0], None, s[jo + 1][1], True, red=red)
        del m, rstd_m
    dhh = F_.linear_dgrad(dm, wd, rt.weight_t(unit, 5, wd))
    dgu, hh = F_.swiglu_bwd_h(dhh, gu, cfg.ffn_act)
    del dhh, gu
    F_.linear_wgrad(dm, hh, s[5][0], None, s[5][1])
    del hh, dm
    F_.linear_wgrad(dgu, h2, s[4][0], None, s[4][1])
    del h2
    dh2 = F_.linear_dgrad(dgu, wgu, rt.weight_t(unit, 4, wgu))
    del dgu
    if jo is None:
        dx1 = F_.norm_bwd(dh2, x1, w_post, None, rstd2, dx2, s[3][0], None, s[3][1], True, red=red)
        da = dx1
    else:
        dx1, da = F_.sandwich_bwd(dh2, x1, w_post, rstd2, dx2, a, ws[jo], rstd_a, s[3], s[jo], red)
    del dh2, x1, rstd2, dx2, a, rstd_a
    F_.linear_wgrad(da, o, s[2][0], None, s[2][1])
    do = F_.linear_dgrad(da, wo, rt.weight_t(unit, 2, wo))
    del da
    # ---- attention half
    window = 0 if ctx.bounds is not None else cfg.sliding_window or 0
    if full:
        _, h1, _, rstd1 = F_.norm_fwd(x, None, w_in, None, cfg.norm_eps, True)
        qkv = F_.linear_fwd(h1, wqkv)
        if model.cp is not None:      # the re-gather: one more all-gather per layer, in layer order on every rank
            aux, raw = _cp_rope_gather(model, qkv, Hq, Hkv, D, qkn)
        else:
            raw = _rope_fwd(model, qkv, T, Hq, Hkv, D, qkn)
    else:
        h1 = F_.norm_apply(x, w_in, None, None, rstd1, True)
    dqkv = torch.empty_like(qkv)
    if model.cp is not None:
        _cp_attn_bwd(model, qkv, aux, o, do, lse, dqkv, Hq, Hkv, D, window, ctx.bounds, rt.seed, qkn, raw, sq, sk, red,
                     sink, s[-1])
    else:
        dsink = F_.attn_bwd(qkv[:, :qd], qkv[:, qd:qd + kd], qkv[:, qd + kd:], o, do, lse, aux,
                            dqkv[:, :qd], dqkv[:, qd:qd + kd], dqkv[:, qd + kd:], B, T, Hq, Hkv,
                            1.0 / math.sqrt(D), True, 0.0, rt.seed, 0, window=window, bounds=ctx.bounds, sink=sink,
                            softcap=cfg.attn_softcap)
        if sink is not None:
            F_.reduce_partials(red, dsink, s[-1][0], s[-1][1])
        _rope_bwd(model, dqkv, T, Hq, Hkv, D, qkn, raw, sq, sk, red)
    ctx.bounds = None
    del qkv, aux, o, do, lse, raw
    F_.linear_wgrad(dqkv, h1, s[1][0], None, s[1][1])
    del h1
    dh1 = F_.linear_dgrad(dqkv, wqkv, rt.weight_t(unit, 1, wqkv))
    del dqkv
    dx = F_.norm_bwd(dh1, x, w_in, None, rstd1, dx1, s[0][0], None, s[0][1], True, red=red)
    if shared is None:
        red.flush()
    rt.grads_ready(unit)
    rt.release_backward(unit)
    return dx


def _check_head_chunk(n):
    if n is None:
        return None
    if isinstance(n, bool) or not isinstance(n, int) or n <= 0:
        raise ValueError(f"head_chunk must be None or a positive integer (rows per chunk), got {n!r}")
    return n


def head_chunks(rows, n):
    """How many chunks the head runs for ``rows`` rows under ``head_chunk = n``: 1 when off or when one chunk
    would hold every row (then today's unchunked path runs: there is nothing to save)."""
    return 1 if n is None or n >= rows else -(-rows // n)


def _head_loss_opts(cfg):
    """The loss kernels' options of ``cfg.final_softcap`` / ``cfg.lm_z_loss_coef``; none when both are off, so the
    calls (and their launches) are those of a config without the fields."""
    if cfg.final_softcap or cfg.lm_z_loss_coef:
        return {"softcap": float(cfg.final_softcap), "z_coef": float(cfg.lm_z_loss_coef)}
    return {}


def _capped_logits(logits, cap, copy):
    """The logits a caller gets back (``return_logits`` / no targets; off the training path): under
    ``final_softcap`` = cap the capped ones, ``cap * tanh(z / cap)`` formed in fp32 and rounded to the model's
    format.  The loss is never formed from these: the kernels cap the raw product themselves, in registers."""
    if cap:
        return (cap * torch.tanh(logits.float() / cap)).to(logits.dtype)
    return logits.clone() if copy else logits


def _head_forward_chunked(ctx, x, model, targets, n):
    """:meth:`_HeadFn.forward` under ``model.head_chunk = n < rows``: the logits exist one [n, V] chunk at a time
    (each chunk's block returns to the allocator before the next product asks for it) and only their loss and
    log-sum-exp rows are kept.  The loss rows are the unchunked path's wherever the chunk product's rows are."""
    rt, unit = model.rt, model.unit_head
    w_norm, w_head = rt.acquire(unit)
    _, h, _, rstd = F_.norm_fwd(x, None, w_norm, None, model.cfg.norm_eps, True)
    tg = targets.reshape(-1)
    R = h.shape[0]
    loss_rows = torch.empty(R, dtype=torch.float32, device=h.device)
    lse = torch.empty(R, dtype=torch.float32, device=h.device)
    for r0 in range(0, R, n):
        r1 = min(r0 + n, R)
        logits = F_.linear_fwd(h[r0:r1], w_head)
        F_.xent_lse(logits, tg[r0:r1], -1, loss_rows[r0:r1], lse[r0:r1], **_head_loss_opts(model.cfg))
        del logits
    lc = F_.xent_mean(loss_rows, tg, -1)          # (mean, count) over all rows, as unchunked
    loss, count = lc[0], lc[1:2]
    rt.release_forward(unit)
    ctx.model, ctx.no_loss, ctx.chunk = model, False, n
    ctx.saved = (x, h, rstd, lse, tg, count)
    out_logits = h.new_empty(0)
    ctx.mark_non_differentiable(out_logits)
    return out_logits, loss


def _head_backward_chunked(ctx, dloss):
    """The backward of :func:`_head_forward_chunked`: per chunk the forward product again (same call, same inputs,
    so the forward's logits bit for bit), dlogits in place from the kept log-sum-exp, then the two gradient
    products -- the weight gradient accumulating into its slot from the second chunk on.  The scale g and the
    scaled hs are the whole batch's, and the norm backward runs once on the assembled dh."""
    model, n = ctx.model, ctx.chunk
    rt, unit = model.rt, model.unit_head
    (x, h, rstd, lse, tg, count) = ctx.saved
    ctx.saved = None
    w_norm, w_head = rt.acquire_backward(unit)
    dwh, acc_h = rt.grad_slot(unit, 1)
    hs, g = F_.scale_by(h, dloss, count)                      # g = dloss / count (device)
    wt = rt.weight_t(unit, 1, w_head)
    R = h.shape[0]
    dh = torch.empty_like(h)
    for r0 in range(0, R, n):
        r1 = min(r0 + n, R)
        dl = F_.linear_fwd(h[r0:r1], w_head)
        F_.xent_bwd_lse_(dl, tg[r0:r1], lse[r0:r1], -1, **_head_loss_opts(model.cfg))
        F_.linear_wgrad(dl, hs[r0:r1], dwh, None, acc_h if r0 == 0 else True)
        dh[r0:r1].copy_(F_.head_dgrad(dl, w_head, wt, g))
        del dl
    del h, hs, lse
    gw, acc = rt.grad_slot(unit, 0)
    dx = F_.norm_bwd(dh, x, w_norm, None, rstd, None, gw, None, acc, True)
    rt.grads_ready(unit)
    rt.release_backward(unit)
    return dx


class _HeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, model, targets, return_logits):
        n = _check_head_chunk(model.head_chunk)
        ctx.chunk = None
        # the caller wants the logits (no targets, return_logits), or one chunk holds them all: the unchunked path
        if n is not None and n < x.shape[0] and targets is not None and not return_logits:
            return _head_forward_chunked(ctx, x, model, targets, n)
        rt, unit = model.rt, model.unit_head
        w_norm, w_head = rt.acquire(unit)
        _, h, _, rstd = F_.norm_fwd(x, None, w_norm, None, model.cfg.norm_eps, True)
        logits = F_.linear_fwd(h, w_head)
        if targets is None:
            rt.release_forward(unit)
            logits = _capped_logits(logits, model.cfg.final_softcap, False)
            ctx.mark_non_differentiable(logits)
            ctx.no_loss = True
            return logits, logits.new_zeros(())
        kept = _capped_logits(logits, model.cfg.final_softcap, True) if return_logits else None
        tg = targets.reshape(-1)
        loss_rows = F_.xent_fwd_bwd_(logits, tg, -1, **_head_loss_opts(model.cfg))
        lc = F_.xent_mean(loss_rows, tg, -1)          # (mean, count) on the device
        loss, count = lc[0], lc[1:2]
        rt.release_forward(unit)
        ctx.model, ctx.no_loss = model, False
        ctx.saved = (x, h, rstd, logits, count)
        out_logits = kept if kept is not None else logits.new_empty(0)
        ctx.mark_non_differentiable(out_logits)
        return out_logits, loss

    @staticmethod
    def backward(ctx, dlogits_unused, dloss):
        if ctx.no_loss:
            return None, None, None, None
        if ctx.chunk is not None:
            return _head_backward_chunked(ctx, dloss), None, None, None
        model = ctx.model
        rt, unit = model.rt, model.unit_head
        (x, h, rstd, dl, count) = ctx.saved
        ctx.saved = None
        w_norm, w_head = rt.acquire_backward(unit)
        dwh, acc_h = rt.grad_slot(unit, 1)
        hs, g = F_.scale_by(h, dloss, count)                      # g = dloss / count (device)
        F_.linear_wgrad(dl, hs, dwh, None, acc_h)
        dh = F_.head_dgrad(dl, w_head, rt.weight_t(unit, 1, w_head), g)
        gw, acc = rt.grad_slot(unit, 0)
        dx = F_.norm_bwd(dh, x, w_norm, None, rstd, None, gw, None, acc, True)
        rt.grads_ready(unit)
        rt.release_backward(unit)
        return dx, None, None, None


class MistralLM(nn.Module):
    def __init__(self, cfg: ModelConfig):
        super().__init__()
        assert cfg.n_embd % cfg.n_head == 0 and cfg.n_head % cfg.kv_heads == 0
        self.cfg = cfg
        self.model = nn.Module()
        self.model.embed_tokens = nn.Embedding(cfg.vocab_size, cfg.n_embd)
        self.model.layers = nn.ModuleList([MistralLayer(cfg) for _ in range(cfg.n_layer)])
        self.model.norm = _RMSNorm(cfg.n_embd)
        self.lm_head = nn.Linear(cfg.n_embd, cfg.vocab_size, bias=False)
        for mod in self.modules():
            if isinstance(mod, (nn.Linear, nn.Embedding)):
                nn.init.normal_(mod.weight, mean=0.0, std=0.02)
        self.rt = EAGER
        self.drop_p = 0.0
        self._rope = {}
        self.cp = None          # parallel.context.ContextParallel.attach(): a layout, not a model property
        # which of a layer's activations its forward keeps for the backward (set by the harness, like cp):
        # "off" all twelve (thirteen with QK-norm's raw), "selective" without h1 / h2 / hh, "full" only x, o, lse
        # (_layer_backward_recompute)
        self.activation_recompute = "off"
        # rows per chunk of the LM head (set by the harness too): None materialises the [rows, V] logits and keeps
        # them as dlogits for the backward; N keeps their log-sum-exp rows and re-runs the product per chunk
        self.head_chunk = None
        self._moe_counts = None     # int32 [n_layer, n_experts]: the last micro-step's assignments per expert
        self._moe_aux = None        # fp32 [n_layer, 2]: the last micro-step's (balance, z) per layer (aux loss on)
        self.unit_embed = Unit("embed", [("model.embed_tokens.weight", self.model.embed_tokens.weight)], 0)
        self.unit_blocks = [Unit(f"layers.{i}", [(f"model.layers.{i}.{n}", p) for n, p in layer.param_list()], i + 1)
                            for i, layer in enumerate(self.model.layers)]
        self.unit_head = Unit("head", [("model.norm.weight", self.model.norm.weight),
                                       ("lm_head.weight", self.lm_head.weight)], len(self.unit_blocks) + 1)

    def units(self):
        return [self.unit_embed] + self.unit_blocks + [self.unit_head]

    def rope(self, device, T):
        key = (str(device), T)
        if key not in self._rope:
            self._rope[key] = ref.rope_tables(T, self.cfg.head_dim, self.cfg.rope_theta, device)
        return self._rope[key]

    def num_params(self):
        return sum(p.numel() for p in self.parameters())

    def moe_counts(self, device):
        """int32 [n_layer, n_experts], row i written by layer i's slot assignment every micro-step (before drops)."""
        if self._moe_counts is None or self._moe_counts.device.type != torch.device(device).type:
            self._moe_counts = torch.zeros(self.cfg.n_layer, self.cfg.n_experts, dtype=torch.int32, device=device)
        return self._moe_counts

    def moe_aux(self, device):
        """fp32 [n_layer, 2], row i = layer i's (load-balancing loss, router z-loss) of the last micro-step; written
        only while ``cfg.moe_aux_on``."""
        if self._moe_aux is None or self._moe_aux.device.type != torch.device(device).type:
            self._moe_aux = torch.zeros(self.cfg.n_layer, 2, dtype=torch.float32, device=device)
        return self._moe_aux

    def moe_stats(self, rows):
        """The ``moe`` block of the harness's extended record for micro-steps of ``rows`` local token rows: reads the
        last micro-step's counts (one device-to-host copy; call it after the timed steps).  The figures are the
        calling rank's alone: under world > 1 or context parallelism they cover its local rows."""
        cfg = self.cfg
        E, K = cfg.n_experts, cfg.moe_top_k
        C = ref.moe_capacity(rows, E, K, cfg.moe_capacity_factor)
        out = {"experts": E, "top_k": K, "capacity_factor": cfg.moe_capacity_factor, "capacity": C,
               "counts": None, "drop_fraction": None,
               "scope": "this rank's local token rows of the last micro-step (not summed over ranks): counts per "
                        "layer and expert before drops; drop_fraction pooled over the layers; balance_loss / z_loss "
                        "per layer, unweighted (None when both coefficients are 0).  The reported training loss is "
                        "the total: lm_loss + aux_loss_coef * sum(balance_loss) + z_loss_coef * sum(z_loss)",
               "aux_loss_coef": cfg.moe_aux_loss_coef, "z_loss_coef": cfg.moe_z_loss_coef,
               "balance_loss": None, "z_loss": None}
        if cfg.moe_dropless:        # no capacity: R packed slot rows per micro-step, nothing dropped
            out.update(dropless=True, rows=ref.moe_dropless_rows(rows, E, K), capacity=None, drop_fraction=0.0)
        if self._moe_counts is not None:
            aux_on = cfg.moe_aux_on and self._moe_aux is not None
            # one device-to-host copy: the counts and, as fp32 bit patterns beside them, the two losses
            both = self._moe_counts if not aux_on else torch.cat([self._moe_counts, self._moe_aux.view(torch.int32)], 1)
            both = both.cpu()
            counts = both[:, :E]
            out["counts"] = counts.tolist()
            total = int(counts.sum())
            if not cfg.moe_dropless:
                out["drop_fraction"] = float((counts - C).clamp(min=0).sum()) / total if total else 0.0
            if aux_on:
                aux = both[:, E:].contiguous().view(torch.float32)
                out["balance_loss"], out["z_loss"] = aux[:, 0].tolist(), aux[:, 1].tolist()
        return out

    def forward(self, idx, targets=None, return_logits=False):
        B, T = idx.shape
        assert T <= self.cfg.block_size
        # packed sequences: the document bounds of this batch, computed once (on the device, from idx, so a
        # captured step follows its static idx buffer) and shared by every layer's forward and backward
        self._cur_bounds = None
        if self.cfg.doc_eos_id is not None:
            self._cur_bounds = F_.doc_bounds(idx, self.cfg.doc_eos_id, self.cfg.sliding_window or 0)
        if self.cp is not None:
            # context parallel: every rank of the group got the same full rows (the bounds above are the full
            # row's); from here on this rank holds its ranges' tokens only, range-major, as a batch of
            # n_ranges * B shorter rows.  Targets equal inputs without a shift, so a slice carries its targets.
            self._cur_full_bt = (B, T)
            idx = self.cp.slice_rows(idx, T)
            if targets is not None:
                targets = self.cp.slice_rows(targets, T)
            B, T = idx.shape
        self._cur_bt = (B, T)
        anchor = torch.empty((), requires_grad=True)
        x = _EmbedFn.apply(anchor, idx, self)
        auxs = []
        for i in range(len(self.unit_blocks)):
            x = _LayerFn.apply(x, self, i)
            if isinstance(x, tuple):        # an auxiliary router loss is on: (x, the layer's (balance, z))
                x, aux = x
                auxs.append(aux)
        logits, loss = _HeadFn.apply(x, self, targets, return_logits)
        if targets is None:
            return logits.view(B, T, -1), None
        if auxs:        # a fixed number of small launches whatever the depth, nothing read by the host
            tot = torch.stack(auxs).sum(0).to(loss.dtype)
            if self.cfg.moe_aux_loss_coef:
                loss = loss + self.cfg.moe_aux_loss_coef * tot[0]
            if self.cfg.moe_z_loss_coef:
                loss = loss + self.cfg.moe_z_loss_coef * tot[1]
        return (logits.view(B, T, -1) if return_logits else None), loss
