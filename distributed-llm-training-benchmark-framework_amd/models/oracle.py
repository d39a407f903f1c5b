"""Plain-torch oracles of the model families (autograd through stock nn modules).

``OracleTinyGPT`` follows the reference architecture of ``train_harness.py:36-131`` op for op —
``nn.MultiheadAttention`` with no mask, pre-LN residual blocks, exact GELU, tied head — so the
fused TinyGPT can be checked against it parameter-for-parameter (same state-dict names).  It is
used only by tests and for parity checks; it is not a training path.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .config import ModelConfig


class _OracleBlock(nn.Module):
    def __init__(self, d, h, p):
        super().__init__()
        self.ln_1 = nn.LayerNorm(d)
        self.attn = nn.MultiheadAttention(d, h, dropout=p, batch_first=True)
        self.ln_2 = nn.LayerNorm(d)
        self.mlp = nn.Sequential(nn.Linear(d, 4 * d), nn.GELU(), nn.Linear(4 * d, d), nn.Dropout(p))

    def forward(self, x):
        a = self.ln_1(x)
        y, _ = self.attn(a, a, a, need_weights=False)
        x = x + y
        return x + self.mlp(self.ln_2(x))


class OracleTinyGPT(nn.Module):
    def __init__(self, cfg: ModelConfig):
        super().__init__()
        d = cfg.n_embd
        self.transformer = nn.ModuleDict({
            "wte": nn.Embedding(cfg.vocab_size, d),
            "wpe": nn.Embedding(cfg.block_size, d),
            "drop": nn.Dropout(cfg.dropout),
            "h": nn.ModuleList([_OracleBlock(d, cfg.n_head, cfg.dropout) for _ in range(cfg.n_layer)]),
            "ln_f": nn.LayerNorm(d),
        })
        self.lm_head = nn.Linear(d, cfg.vocab_size, bias=False)
        self.transformer["wte"].weight = self.lm_head.weight

    def forward(self, idx, targets=None):
        T = idx.shape[1]
        pos = torch.arange(T, device=idx.device)[None]
        x = self.transformer["drop"](self.transformer["wte"](idx) + self.transformer["wpe"](pos))
        for blk in self.transformer["h"]:
            x = blk(x)
        logits = self.lm_head(self.transformer["ln_f"](x))
        loss = None
        if targets is not None:
            loss = F.cross_entropy(logits.view(-1, logits.size(-1)), targets.view(-1), ignore_index=-1)
        return logits, loss


class _RMSNorm(nn.Module):
    def __init__(self, d, eps):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))
        self.eps = eps

    def forward(self, x):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.eps) * self.weight


def _rope(x, cos, sin):
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], -1)


def _moe_ffn(mlp, h, cfg):
    """Top-k routed experts with a fixed capacity on the rows ``h`` [N, d], differentiated by autograd alone: the
    K largest router logits per row (ties to the lower expert), softmax gates over them, slots in row-major
    (token, choice) order with overflow dropped (the integer bookkeeping is ``ops.ref.moe_assign``: nothing to
    differentiate), each expert's SwiGLU FFN on its slab, gate-weighted sum."""
    from ..ops import ref
    N = h.shape[0]
    E, K = cfg.n_experts, cfg.moe_top_k
    # dropless: a capacity of all N rows per expert, which no expert can exceed (a token chooses an expert once)
    C = -(-N // 16) * 16 if cfg.moe_dropless else ref.moe_capacity(N, E, K, cfg.moe_capacity_factor)
    vals, idx = torch.sort(mlp.router(h), dim=-1, descending=True, stable=True)
    gate = torch.softmax(vals[:, :K], -1)
    slot, src, _, _ = ref.moe_assign(idx[:, :K].to(torch.int32), E, C)
    zero = torch.zeros((), dtype=h.dtype, device=h.device)
    xe = torch.where((src >= 0)[:, None], h[src.clamp(min=0).long()], zero)
    ys = []
    for e, ex in enumerate(mlp.experts):
        g, u = ex.gate_up_proj(xe[e * C:(e + 1) * C]).chunk(2, -1)
        ys.append(ex.down_proj(_glu_act(g, cfg) * u))
    ye = torch.cat(ys, 0)
    out = torch.zeros_like(h)
    for k in range(K):
        s = slot[:, k]
        out = out + torch.where((s >= 0)[:, None], gate[:, k:k + 1] * ye[s.clamp(min=0).long()], zero)
    return out


def _moe_aux_loss(mlp, h, cfg):
    """The layer's ``a * balance + b * z`` (``cfg.moe_aux_loss_coef`` / ``cfg.moe_z_loss_coef``) on the rows ``h`` in
    stock ops, differentiated by autograd alone: balance = E sum_e f[e] mean_n softmax(logits)[n, e] with f, the
    fraction of the N K assignments that chose expert e (before drops), detached; z = mean_n logsumexp(logits)^2."""
    N = h.shape[0]
    E, K = cfg.n_experts, cfg.moe_top_k
    logits = mlp.router(h)
    idx = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :K]
    counts = torch.bincount(idx.reshape(-1), minlength=E)
    f = (counts.to(logits.dtype) / (N * K)).detach()
    balance = E * (f * torch.softmax(logits, -1).mean(0)).sum()
    z = torch.logsumexp(logits, -1).pow(2).mean()
    return cfg.moe_aux_loss_coef * balance + cfg.moe_z_loss_coef * z


def _glu_act(g, cfg):
    """The gated FFN's activation of the gate: SiLU, or the tanh form of GELU under ``cfg.ffn_act = "geglu"``."""
    return F.gelu(g, approximate="tanh") if cfg.ffn_act == "geglu" else F.silu(g)


def _out(sub, y):
    """A sublayer's output on its way into the residual stream: through ``sub.out_norm`` under ``cfg.sandwich_norm``."""
    return sub.out_norm(y) if hasattr(sub, "out_norm") else y


class OracleMistral(nn.Module):
    """Stock-op Mistral-shape decoder with the same parameter names as dltb.models.mistral."""

    def __init__(self, cfg: ModelConfig):
        super().__init__()
        self.cfg = cfg
        d, hd = cfg.n_embd, cfg.head_dim
        kvd = cfg.kv_heads * hd
        self.model = nn.Module()
        self.model.embed_tokens = nn.Embedding(cfg.vocab_size, d)
        self.model.layers = nn.ModuleList()
        for _ in range(cfg.n_layer):
            layer = nn.Module()
            layer.input_layernorm = _RMSNorm(d, cfg.norm_eps)
            layer.self_attn = nn.Module()
            layer.self_attn.qkv_proj = nn.Linear(d, d + 2 * kvd, bias=False)
            layer.self_attn.o_proj = nn.Linear(d, d, bias=False)
            if cfg.qk_norm:         # RMSNorm over head_dim of every q / k head before RoPE
                layer.self_attn.q_norm = _RMSNorm(hd, cfg.norm_eps)
                layer.self_attn.k_norm = _RMSNorm(hd, cfg.norm_eps)
            if cfg.attn_sinks:      # one learned sink logit per query head
                layer.self_attn.sinks = nn.Parameter(torch.zeros(cfg.n_head))
            layer.post_attention_layernorm = _RMSNorm(d, cfg.norm_eps)
            layer.mlp = nn.Module()
            if cfg.sandwich_norm:   # every sublayer's output through its own RMSNorm before the residual add
                layer.self_attn.out_norm = _RMSNorm(d, cfg.norm_eps)
                layer.mlp.out_norm = _RMSNorm(d, cfg.norm_eps)
            if cfg.n_experts:       # mixture of experts: a router and n_experts FFNs (autograd only, _moe_ffn)
                layer.mlp.router = nn.Linear(d, cfg.n_experts, bias=False)
                layer.mlp.experts = nn.ModuleList()
                for _e in range(cfg.n_experts):
                    ex = nn.Module()
                    ex.gate_up_proj = nn.Linear(d, 2 * cfg.ffn_dim, bias=False)
                    ex.down_proj = nn.Linear(cfg.ffn_dim, d, bias=False)
                    layer.mlp.experts.append(ex)
            else:
                layer.mlp.gate_up_proj = nn.Linear(d, 2 * cfg.ffn_dim, bias=False)
                layer.mlp.down_proj = nn.Linear(cfg.ffn_dim, d, bias=False)
            self.model.layers.append(layer)
        self.model.norm = _RMSNorm(d, cfg.norm_eps)
        self.lm_head = nn.Linear(d, cfg.vocab_size, bias=False)

    def forward(self, idx, targets=None):
        cfg = self.cfg
        B, T = idx.shape
        H, Hkv, hd = cfg.n_head, cfg.kv_heads, cfg.head_dim
        inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, hd // 2, dtype=torch.float64) * 2.0 / hd))
        ang = torch.arange(T, dtype=torch.float64)[:, None] * inv[None]
        cos = ang.cos().float().to(idx.device)[None, None]
        sin = ang.sin().float().to(idx.device)[None, None]
        x = self.model.embed_tokens(idx)
        aux = []
        for layer in self.model.layers:
            h = layer.input_layernorm(x)
            qkv = layer.self_attn.qkv_proj(h)
            q = qkv[..., :H * hd].view(B, T, H, hd).transpose(1, 2)
            k = qkv[..., H * hd:(H + Hkv) * hd].view(B, T, Hkv, hd).transpose(1, 2)
            v = qkv[..., (H + Hkv) * hd:].view(B, T, Hkv, hd).transpose(1, 2)
            if cfg.qk_norm:
                q, k = layer.self_attn.q_norm(q), layer.self_attn.k_norm(k)
            q, k = _rope(q, cos, sin), _rope(k, cos, sin)
            k = k.repeat_interleave(H // Hkv, 1)
            v = v.repeat_interleave(H // Hkv, 1)
            if cfg.sliding_window or cfg.doc_eos_id is not None or cfg.attn_sinks or cfg.attn_softcap:
                i = torch.arange(T, device=idx.device)
                band = (i[None, :] <= i[:, None]).expand(B, 1, T, T)
                if cfg.sliding_window:      # band mask: query i sees keys i - W < j <= i
                    band = band & (i[None, :] > i[:, None] - cfg.sliding_window)
                if cfg.doc_eos_id is not None:
                    # document mask: token t belongs to document number (EOS tokens before t); an EOS ends its own
                    eos = (idx == cfg.doc_eos_id).to(torch.int64)
                    doc = eos.cumsum(1) - eos
                    band = band & (doc[:, None, :, None] == doc[:, None, None, :])
                if cfg.attn_sinks:
                    # explicit softmax over [scores | sink]: the sink is one more column per head, raw (not scaled),
                    # and carries no value, so its column is dropped before the product with v
                    sc = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
                    sc = sc.masked_fill(~band, float("-inf"))
                    sk = layer.self_attn.sinks.to(sc.dtype).view(1, H, 1, 1).expand(B, H, T, 1)
                    o = torch.softmax(torch.cat([sc, sk], -1), -1)[..., :T] @ v
                elif cfg.attn_softcap:
                    # explicit softmax over the capped scores cap * tanh(x / cap); the masks apply after the cap
                    sc = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
                    sc = cfg.attn_softcap * torch.tanh(sc / cfg.attn_softcap)
                    o = torch.softmax(sc.masked_fill(~band, float("-inf")), -1) @ v
                else:
                    o = F.scaled_dot_product_attention(q, k, v, attn_mask=band)
            else:
                o = F.scaled_dot_product_attention(q, k, v, is_causal=True)
            x = x + _out(layer.self_attn, layer.self_attn.o_proj(o.transpose(1, 2).reshape(B, T, H * hd)))
            if cfg.n_experts:
                h2 = layer.post_attention_layernorm(x).reshape(B * T, -1)
                if cfg.moe_aux_loss_coef or cfg.moe_z_loss_coef:
                    aux.append(_moe_aux_loss(layer.mlp, h2, cfg))
                x = x + _out(layer.mlp, _moe_ffn(layer.mlp, h2, cfg).view_as(x))
                continue
            gu = layer.mlp.gate_up_proj(layer.post_attention_layernorm(x))
            g, u = gu.chunk(2, -1)
            x = x + _out(layer.mlp, layer.mlp.down_proj(_glu_act(g, cfg) * u))
        logits = self.lm_head(self.model.norm(x))
        if cfg.final_softcap:       # final-logit soft-capping: the loss and the returned logits are the capped ones
            logits = cfg.final_softcap * torch.tanh(logits / cfg.final_softcap)
        loss = None
        if targets is not None:
            loss = F.cross_entropy(logits.view(-1, logits.size(-1)), targets.view(-1), ignore_index=-1)
            if cfg.lm_z_loss_coef:  # z-loss: mean over the valid rows of logsumexp(logits)^2
                tg = targets.view(-1)
                z2 = torch.logsumexp(logits.view(-1, logits.size(-1)), -1).pow(2)
                loss = loss + cfg.lm_z_loss_coef * (z2 * (tg != -1)).sum() / (tg != -1).sum().clamp(min=1)
            for term in aux:
                loss = loss + term
        return logits, loss
