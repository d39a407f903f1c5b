"""Model configurations.

Tier table of the reference (``benchmarking/train_harness.py:157-179``):

* Tier A: vocab 32000, d 1024, 16 heads, 16 layers, block_size = seq_len  -> 236,406,784 params
* Tier B: vocab 32000, d 2048, 32 heads, 32 layers, block_size = seq_len  -> 1,681,199,104 params
  (the reference docstring calls these "1-3B" / "7-13B"; the code builds the sizes above).
* the unused TinyGPT constructor default (``train_harness.py:39-47``): d 768, 12 heads, 12 layers,
  block 4096.

Additional MI355X-era shape (not in the reference, requested by BASELINE.json config #5):

* ``M7B``: Mistral-7B shape - d 4096, 32 layers, 32 query heads / 8 KV heads (GQA), SwiGLU FFN 14336,
  RMSNorm, RoPE, causal attention, untied head, vocab 32000 (7.24B params).
"""
import math
from dataclasses import dataclass, field, asdict
from typing import Optional


FFN_ACTS = ("swiglu", "geglu")


@dataclass
class ModelConfig:
    arch: str = "tinygpt"            # "tinygpt" | "mistral"
    vocab_size: int = 32000
    n_embd: int = 768
    n_head: int = 12
    n_layer: int = 12
    block_size: int = 4096
    dropout: float = 0.1
    # mistral-shape extras
    n_kv_head: Optional[int] = None
    ffn_hidden: Optional[int] = None
    rope_theta: float = 10000.0
    norm_eps: float = 1e-5
    causal: bool = False             # TinyGPT reproduces the reference's NON-causal MHA
    tie_embeddings: bool = True
    tier: str = "custom"
    # causal sliding window W: query i sees keys i - W < j <= i (W keys including its own); None = no window
    sliding_window: Optional[int] = None
    # packed sequences: a token equal to doc_eos_id ends a document (and belongs to it); attention does not cross
    # document boundaries.  None = every row is one document.  Causal only; composes with sliding_window.
    doc_eos_id: Optional[int] = None
    # mixture of experts (mistral arch): n_experts SwiGLU FFNs per layer behind a top-k router with a fixed capacity of
    # min(ceil(moe_capacity_factor * rows * moe_top_k / n_experts), rows) slots per expert, rounded up to a multiple
    # of 16 (assignments past it are dropped).  None = the dense FFN.
    n_experts: Optional[int] = None
    moe_top_k: int = 2
    moe_capacity_factor: float = 1.25
    # auxiliary router losses, per layer on the rank's local token rows (ops/ref.py moe_aux_fwd):
    # loss = lm_loss + moe_aux_loss_coef * sum_layers balance + moe_z_loss_coef * sum_layers z.  0 = off
    moe_aux_loss_coef: float = 0.0
    moe_z_loss_coef: float = 0.0
    # dropless routing: no capacity, every assignment kept.  The experts' rows are packed into 128-aligned segments of
    # one [R, d] buffer, R = roundup(rows * moe_top_k, 128) + 128 * n_experts, and run as grouped GEMMs that read the
    # segment bounds on the device (csrc/gemm_grouped.hip); moe_capacity_factor is not used.
    moe_dropless: bool = False
    # QK-norm (mistral arch): an RMSNorm over head_dim on every query head and every key head before RoPE, with one
    # learned [head_dim] weight for q and one for k per layer (eps = norm_eps); fused with RoPE (csrc/qknorm.hip)
    qk_norm: bool = False
    # learned attention sinks (mistral arch): one raw logit per query head and layer that joins the softmax denominator
    # and carries no value, so a head can attend to "nothing" (the gpt-oss block); parameter self_attn.sinks [n_head],
    # initialised to zeros.  The forward kernel's epilogue takes it in (csrc/attention.hip SINK), csrc/attn_sink.hip
    # forms its gradient.
    attn_sinks: bool = False
    # attention logit soft-capping (mistral arch): every score x = q.k / sqrt(head_dim) becomes cap * tanh(x / cap)
    # before the masks and the softmax (Gemma-2 / Gemma-3 / Grok-1; Gemma-2 uses 50); 0 = off.  No parameter; the CAP
    # instantiations of the three attention kernels (csrc/attention.hip).  Not together with attn_sinks.
    attn_softcap: float = 0.0
    # final-logit soft-capping (mistral arch): the LM-head loss is formed from cap * tanh(logits / cap) (Gemma-2 /
    # Gemma-3 use 30); 0 = off.  No parameter; the CAP instantiations of the three loss kernels (csrc/xent.hip).
    final_softcap: float = 0.0
    # z-loss on the LM head (mistral arch; PaLM, OLMo-2, Chameleon use about 1e-4): the loss gains
    # lm_z_loss_coef * mean over the valid rows of logsumexp(logits)^2 (of the capped logits under final_softcap); 0 = off
    lm_z_loss_coef: float = 0.0
    # sandwich norms (mistral arch; Gemma-2 / Gemma-3, the placement of OLMo-2 and Grok-1): every sublayer's output goes
    # through its own RMSNorm before it joins the residual stream, x1 = x + RMSNorm(attn), x2 = x1 + RMSNorm(ffn), on top
    # of the two pre-norms; two [n_embd] weights per layer, self_attn.out_norm.weight and mlp.out_norm.weight,
    # initialised to ones (csrc/sandwich_norm.hip)
    sandwich_norm: bool = False
    # the gated FFN's activation (mistral arch): "swiglu" = silu(gate) * up, "geglu" = gelu_tanh(gate) * up (Gemma);
    # the GEGLU instantiations of the three gated-FFN kernels (csrc/elementwise.hip), dense and both MoE routings
    ffn_act: str = "swiglu"

    def __post_init__(self):
        self.validate()

    def validate(self):
        """Raises ValueError for an inconsistent config (also called again where a field is set later)."""
        w = self.sliding_window
        if w is not None:
            if isinstance(w, bool) or not isinstance(w, int) or w < 1:
                raise ValueError(f"sliding_window must be an integer >= 1 or None, got {w!r}")
            if not self.causal:
                raise ValueError("sliding_window needs causal=True")
        e = self.doc_eos_id
        if e is not None:
            if isinstance(e, bool) or not isinstance(e, int) or not 0 <= e < self.vocab_size:
                raise ValueError(f"doc_eos_id must be an integer in [0, vocab_size) or None, got {e!r}")
            if not self.causal:
                raise ValueError("doc_eos_id (document-masked attention) needs causal=True")
        if not isinstance(self.qk_norm, bool):
            raise ValueError(f"qk_norm must be a bool, got {self.qk_norm!r}")
        if self.qk_norm:
            if self.arch != "mistral":
                raise ValueError(f"qk_norm (QK-norm fused with RoPE) needs the mistral arch, got arch {self.arch!r}")
            if self.head_dim not in (64, 128):
                raise ValueError(f"qk_norm needs head_dim 64 or 128, got {self.head_dim}")
        if not isinstance(self.attn_sinks, bool):
            raise ValueError(f"attn_sinks must be a bool, got {self.attn_sinks!r}")
        if self.attn_sinks and self.arch != "mistral":
            raise ValueError(f"attn_sinks (learned attention sinks) needs the mistral arch, got arch {self.arch!r}")
        c = self.attn_softcap
        if isinstance(c, bool) or not isinstance(c, (int, float)) or not math.isfinite(c) or c < 0:
            raise ValueError(f"attn_softcap must be a finite number >= 0 (0 = off), got {c!r}")
        if c > 0 and self.arch != "mistral":
            raise ValueError(f"attn_softcap (attention logit soft-capping) needs the mistral arch, got arch "
                             f"{self.arch!r}")
        if c > 0 and self.attn_sinks:
            raise ValueError("attn_softcap together with attn_sinks is not supported")
        for name, what in (("final_softcap", "final-logit soft-capping"), ("lm_z_loss_coef", "LM-head z-loss")):
            c = getattr(self, name)
            if isinstance(c, bool) or not isinstance(c, (int, float)) or not math.isfinite(c) or c < 0:
                raise ValueError(f"{name} must be a finite number >= 0 (0 = off), got {c!r}")
            if c > 0 and self.arch != "mistral":
                raise ValueError(f"{name} ({what}) needs the mistral arch, got arch {self.arch!r}")
        if not isinstance(self.sandwich_norm, bool):
            raise ValueError(f"sandwich_norm must be a bool, got {self.sandwich_norm!r}")
        if self.sandwich_norm and self.arch != "mistral":
            raise ValueError(f"sandwich_norm (an RMSNorm on every sublayer's output) needs the mistral arch, got arch "
                             f"{self.arch!r}")
        if self.ffn_act not in FFN_ACTS:
            raise ValueError(f"ffn_act must be one of {', '.join(FFN_ACTS)}, got {self.ffn_act!r}")
        if self.ffn_act != "swiglu" and self.arch != "mistral":
            raise ValueError(f"ffn_act = {self.ffn_act!r} (the gated FFN's activation) needs the mistral arch, got arch "
                             f"{self.arch!r}")
        k, cf = self.moe_top_k, self.moe_capacity_factor
        if isinstance(k, bool) or not isinstance(k, int) or k not in (1, 2, 4):
            raise ValueError(f"moe_top_k must be 1, 2 or 4, got {k!r}")
        if isinstance(cf, bool) or not isinstance(cf, (int, float)) or not 0.0 < cf < float("inf"):
            raise ValueError(f"moe_capacity_factor must be a positive finite number, got {cf!r}")
        for name in ("moe_aux_loss_coef", "moe_z_loss_coef"):
            c = getattr(self, name)
            if isinstance(c, bool) or not isinstance(c, (int, float)) or not 0.0 <= c < float("inf"):
                raise ValueError(f"{name} must be a finite number >= 0, got {c!r}")
        ne = self.n_experts
        if not isinstance(self.moe_dropless, bool):
            raise ValueError(f"moe_dropless must be a bool, got {self.moe_dropless!r}")
        if self.moe_dropless:
            if ne is None or self.arch != "mistral":
                raise ValueError("moe_dropless needs n_experts (the mixture-of-experts FFN of the mistral arch), got "
                                 f"n_experts {ne!r}, arch {self.arch!r}")
            if self.n_embd % 128 or self.ffn_dim % 128:
                raise ValueError("moe_dropless needs n_embd and ffn_hidden to be multiples of 128 (the grouped GEMM's "
                                 f"tile), got n_embd {self.n_embd}, ffn_hidden {self.ffn_dim}")
        if ne is None and self.moe_aux_on:
            raise ValueError("moe_aux_loss_coef / moe_z_loss_coef need n_experts (the mixture-of-experts FFN of the "
                             f"mistral arch), got n_experts None, arch {self.arch!r}")
        if ne is not None:
            if isinstance(ne, bool) or not isinstance(ne, int) or not 2 <= ne <= 64:
                raise ValueError(f"n_experts must be an integer in [2, 64] or None, got {ne!r}")
            if self.arch != "mistral":
                raise ValueError(f"n_experts (mixture-of-experts FFN) needs the mistral arch, got arch {self.arch!r}")
            if k > ne:
                raise ValueError(f"moe_top_k = {k} exceeds n_experts = {ne}")
            if self.n_embd % 64:
                raise ValueError(f"n_experts needs n_embd to be a multiple of 64, got {self.n_embd}")
        elif self.arch != "mistral" and (k != 2 or cf != 1.25):
            raise ValueError(f"moe_top_k / moe_capacity_factor need the mistral arch, got arch {self.arch!r}")

    @property
    def moe_aux_on(self) -> bool:
        """An auxiliary router loss is on: the layers return (balance, z) and the router gradient is dense."""
        return bool(self.moe_aux_loss_coef or self.moe_z_loss_coef)

    @property
    def head_dim(self) -> int:
        return self.n_embd // self.n_head

    @property
    def kv_heads(self) -> int:
        return self.n_kv_head or self.n_head

    @property
    def ffn_dim(self) -> int:
        return self.ffn_hidden or 4 * self.n_embd

    def to_dict(self):
        return asdict(self)

    def num_params(self) -> int:
        """Exact parameter count (tied weights counted once), matching ``sum(p.numel())``."""
        d, V, L = self.n_embd, self.vocab_size, self.n_layer
        if self.arch == "tinygpt":
            per_block = (2 * d) + (3 * d * d + 3 * d) + (d * d + d) + (2 * d) \
                + (self.ffn_dim * d + self.ffn_dim) + (d * self.ffn_dim + d)
            return V * d + self.block_size * d + L * per_block + 2 * d
        hd = self.head_dim
        kvd = self.kv_heads * hd
        ffn = 3 * d * self.ffn_dim
        if self.n_experts:       # every expert's FFN plus the router
            ffn = self.n_experts * ffn + self.n_experts * d
        per_block = d + (d * d + 2 * kvd * d) + d * d + d + ffn
        if self.qk_norm:         # the q and the k weight, [head_dim] each
            per_block += 2 * hd
        if self.sandwich_norm:   # the attention site's and the FFN site's output norm, [n_embd] each
            per_block += 2 * d
        if self.attn_sinks:      # one sink logit per query head
            per_block += self.n_head
        head = 0 if self.tie_embeddings else V * d
        return V * d + L * per_block + d + head

    def train_flops_per_token(self, seq_len: int, visible_pairs_per_row: Optional[float] = None) -> float:
        """6 * N_matmul + attention (12 * L * T * d non-causal, halved when causal; with a sliding window
        W < T a row sees (W (T - W) + W^2 / 2) / T keys on average instead of T / 2).
        ``visible_pairs_per_row``: the measured number of visible (query, key) pairs of a row of ``seq_len``
        tokens (a document mask depends on the data: ``SyntheticDataset.visible_pairs_per_row``); it replaces
        the T^2 / 2 (or window) count.  Without it the result is exactly the formula above.  With ``n_experts`` the
        FFN term counts ``moe_top_k`` experts and the router product per token.  ``qk_norm`` changes nothing here: it
        adds no matrix product (its 2 * head_dim weights per layer are elementwise), like the other norms; nor does
        ``attn_sinks`` (one more softmax term per query row and head), ``attn_softcap`` (elementwise on the
        scores), ``final_softcap`` / ``lm_z_loss_coef`` (elementwise on the logits, inside the loss kernels),
        ``sandwich_norm`` (two more row norms per layer) or ``ffn_act`` (elementwise)."""
        d, L = self.n_embd, self.n_layer
        if self.arch == "tinygpt":
            n_mat = L * (4 * d * d + 2 * d * self.ffn_dim) + self.vocab_size * d
        else:
            kvd = self.kv_heads * self.head_dim
            ffn = 3 * d * self.ffn_dim
            if self.n_experts:   # nominal: the moe_top_k experts a token is routed to (drops not subtracted) + router
                ffn = self.moe_top_k * ffn + self.n_experts * d
            n_mat = L * (2 * d * d + 2 * kvd * d + ffn) + self.vocab_size * d
        attn = 12 * L * seq_len * d * (0.5 if self.causal else 1.0)
        w = self.sliding_window
        if self.causal and w is not None and w < seq_len:
            attn = 12 * L * d * (w * (seq_len - w) + w * w / 2.0) / seq_len
        if visible_pairs_per_row is not None:
            attn = 12 * L * d * float(visible_pairs_per_row) / seq_len
        return 6.0 * n_mat + attn


TIERS = ("A", "B", "default", "M7B", "M7B_narrow", "tiny", "mtiny")


def get_model_config(tier: str, seq_len: int, dropout: float = 0.1) -> ModelConfig:
    """Reference ``get_model_config(tier, seq_len)`` plus the M7B / tiny (tests) shapes."""
    if tier == "A":
        return ModelConfig(vocab_size=32000, n_embd=1024, n_head=16, n_layer=16,
                           block_size=seq_len, dropout=dropout, tier="A")
    if tier == "B":
        return ModelConfig(vocab_size=32000, n_embd=2048, n_head=32, n_layer=32,
                           block_size=seq_len, dropout=dropout, tier="B")
    if tier == "default":
        return ModelConfig(vocab_size=32000, n_embd=768, n_head=12, n_layer=12,
                           block_size=4096, dropout=dropout, tier="default")
    if tier == "M7B":
        return ModelConfig(arch="mistral", vocab_size=32000, n_embd=4096, n_head=32, n_kv_head=8,
                           n_layer=32, ffn_hidden=14336, block_size=seq_len, dropout=0.0,
                           causal=True, tie_embeddings=False, rope_theta=10000.0, tier="M7B")
    if tier == "tiny":   # unit-test shape (CPU friendly)
        return ModelConfig(vocab_size=128, n_embd=64, n_head=4, n_layer=2, block_size=seq_len,
                           dropout=dropout, tier="tiny")
    if tier == "M7B_narrow":   # the M7B unit / collective structure (32 layers, GQA 4:1, untied head) at d 512:
        # the host-cost proxy of an eager N-rank Mistral-7B step (scripts/m7b_host_proxy.sh)
        return ModelConfig(arch="mistral", vocab_size=4096, n_embd=512, n_head=8, n_kv_head=2, n_layer=32,
                           ffn_hidden=1792, block_size=seq_len, dropout=0.0, causal=True, tie_embeddings=False,
                           rope_theta=10000.0, tier="M7B_narrow")
    if tier == "mtiny":  # Mistral-shape unit-test model: GQA 2:1, head_dim 64 (the GPU attention's smallest)
        return ModelConfig(arch="mistral", vocab_size=256, n_embd=128, n_head=2, n_kv_head=1, n_layer=2,
                           ffn_hidden=256, block_size=seq_len, dropout=0.0, causal=True,
                           tie_embeddings=False, rope_theta=10000.0, tier="mtiny")
    raise ValueError(f"Unknown tier: {tier}")
