"""train_harness-compatible benchmark driver for MI355X.

Reference: ``benchmarking/train_harness.py`` (``main`` :465-504, ``train`` :278-458).  Same CLI
flags, same result record / file name / stdout markers, same per-strategy semantics by default,
re-implemented on dltb's fused HIP kernels and native parallelism engines:

    setup_distributed -> seed -> TinyGPT(tier) -> engine (ddp | fsdp | zero2 | zero3)
    -> synthetic data -> STEP LOOP (engine(batch) / engine.backward / engine.step)
    -> metrics (rank 0) -> result_{S}_ws{WS}_seq{T}_tier{X}.json + JSON markers

Differences that make the numbers honest (recorded in the extended sidecar):
* the timed region is bracketed by a barrier and a device synchronisation; mean step time is the
  synchronised wall time of the post-warmup steps divided by their count, max over ranks;
* per-step losses stay on the device and are read once at the end (the reference syncs every step).
Extra flags (all optional): --accum-semantics, --grad-reduce, --dtype, --device, --bucket-mb, --dropout, --seed,
--profile, --debug-collectives, --fail-at-step, --timeout-min, --data-loader, --model-tier, --sliding-window,
--doc-len, --context-parallel, --cp-layout, --activation-recompute, --head-chunk, --moe-experts, --moe-top-k,
--moe-capacity-factor, --moe-aux-loss-coef, --moe-z-loss-coef, --moe-dropless, --qk-norm,
--attn-sinks, --attn-softcap, --final-softcap, --lm-z-loss-coef, --sandwich-norm, --ffn-act.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

from .data import SyntheticDataset, make_batcher
from .models import build_model, get_model_config
from .parallel.checkpoint import export_consolidated, load_checkpoint, save_checkpoint
from .parallel.graphs import GraphedStep, graphs_enabled
from .ops._ext import available as ext_available, so_path
from .ops import functional as _functional
from .ops.functional import torch_fallbacks
from .comm import describe as comm_describe
from .parallel import STRATEGIES, engine_config, make_engine
from .parallel import context as _context
from .parallel.ds_config import ds_precision
from .parallel.strategy import default_config_path, load_deepspeed_config, load_fsdp_config
from .results import make_record, print_markers, print_result, write_result
from .utils.dist import all_reduce_max, barrier, cleanup_distributed, resolve_ranks, setup_distributed
from .utils.gemm_tuning import flush_tunableop, setup_tunableop
from .utils.platform import MI355X_DENSE_BF16_FLOPS, device_info
from .utils.timers import PhaseTimers

# bf16: the ZeRO configs' precision; fp16: the reference's DDP/FSDP autocast + GradScaler path
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def build_parser():
    p = argparse.ArgumentParser(description="MI355X Distributed Training Benchmark (dltb)")
    # strategy / distributed (reference flags; rank/world default to the torchrun environment)
    p.add_argument("--strategy", type=str, required=True, choices=list(STRATEGIES))
    p.add_argument("--world-size", type=int, default=None, help="Total number of GPUs (default: $WORLD_SIZE or 1)")
    p.add_argument("--rank", type=int, default=None, help="Global rank (default: $RANK or 0)")
    p.add_argument("--local-rank", type=int, default=None, help="Local rank (default: $LOCAL_RANK or 0)")
    p.add_argument("--master-addr", type=str, default=None)
    p.add_argument("--master-port", type=int, default=None)
    # model & data
    p.add_argument("--tier", type=str, required=True, choices=["A", "B", "default", "M7B", "M7B_narrow", "tiny", "mtiny"])
    p.add_argument("--seq-len", type=int, required=True)
    p.add_argument("--sliding-window", type=int, default=None, metavar="N",
                   help="causal tiers (M7B, M7B_narrow, mtiny): query i attends to keys i - N < j <= i (N keys "
                        "including its own, the Mistral mask); default: no window")
    p.add_argument("--doc-len", type=int, default=None, metavar="N",
                   help="causal tiers: pack documents of mean length N (uniform in [1, 2N - 1]) into every row and "
                        "mask attention at the document boundaries; default: every row is one document")
    p.add_argument("--eos-id", type=int, default=None, metavar="ID",
                   help="token that ends a document with --doc-len (default: vocab_size - 1)")
    p.add_argument("--context-parallel", type=int, default=1, metavar="N",
                   help="causal tiers: split every sequence over groups of N consecutive ranks (all-gather of K | V, "
                        "query-range attention kernels; parallel/context.py); N must divide the world size")
    p.add_argument("--cp-layout", choices=["auto", "contiguous", "zigzag"], default="auto",
                   help="which tokens a rank of a context-parallel group owns; auto: zigzag (balanced causal work) "
                        "without --sliding-window, contiguous with it")
    p.add_argument("--activation-recompute", choices=["off", "selective", "full"], default="off",
                   help="causal tiers: what a layer's forward keeps for its backward.  selective drops the two norm "
                        "outputs and the SwiGLU output (-32 %% of the saved activations; rebuilt by elementwise "
                        "kernels); full keeps only the layer input and the attention output (-88 %%) and re-runs "
                        "the qkv, o and gate|up projections in the backward (about a quarter more GEMM work per "
                        "step); attention itself is never re-run")
    p.add_argument("--head-chunk", type=int, default=None, metavar="N",
                   help="causal tiers: the LM head processes its rows (per_device_batch * seq_len / context_parallel) "
                        "in chunks of N, a positive multiple of 16, and keeps their log-sum-exp instead of the "
                        "[rows, vocab] logits; its backward re-runs the head product per chunk.  Default: off")
    p.add_argument("--moe-experts", type=int, default=None, metavar="E",
                   help="causal tiers: replace every layer's FFN by E (2..64) SwiGLU experts behind a top-k router with "
                        "a fixed capacity per expert (assignments past it are dropped); default: the dense FFN")
    p.add_argument("--moe-top-k", type=int, default=None, metavar="K",
                   help="experts per token with --moe-experts: 1, 2 or 4 (default 2)")
    p.add_argument("--moe-capacity-factor", type=float, default=None, metavar="F",
                   help="with --moe-experts: slots per expert = min(ceil(F * rows * K / E), rows) rounded up to a "
                        "multiple of 16, rows = per_device_batch * seq_len / context_parallel (default 1.25)")
    p.add_argument("--moe-aux-loss-coef", type=float, default=None, metavar="A",
                   help="with --moe-experts: add A times the load-balancing loss E * sum_e f_e * P_e of every layer to "
                        "the loss (f_e: the fraction of the rank's assignments that chose expert e, P_e: its mean "
                        "router probability); default 0: off")
    p.add_argument("--moe-z-loss-coef", type=float, default=None, metavar="B",
                   help="with --moe-experts: add B times the router z-loss mean(logsumexp(logits)^2) of every layer "
                        "to the loss; default 0: off")
    p.add_argument("--moe-dropless", action="store_true",
                   help="with --moe-experts: no capacity, every assignment is kept; the experts' rows are packed into "
                        "128-aligned segments of roundup(rows * K, 128) + 128 * E slot rows and run as grouped GEMMs "
                        "(not together with --moe-capacity-factor); default: the fixed-capacity path")
    p.add_argument("--qk-norm", action="store_true",
                   help="causal tiers: RMSNorm over head_dim on every query and key head before RoPE, with one learned "
                        "[head_dim] weight for q and one for k per layer (Qwen3 / OLMo-2 / Gemma-3 style), fused with "
                        "RoPE into one pass; default: off")
    p.add_argument("--attn-sinks", action="store_true",
                   help="causal tiers: one learned sink logit per query head and layer that joins the attention "
                        "softmax's denominator and carries no value (gpt-oss style), taken in by the forward "
                        "attention kernel's epilogue; default: off")
    p.add_argument("--sandwich-norm", action="store_true",
                   help="causal tiers: every sublayer's output goes through its own RMSNorm before it joins the "
                        "residual stream (Gemma-2 / Gemma-3 sandwich norms; the placement of OLMo-2 and Grok-1), two "
                        "more [n_embd] weights per layer, fused with the residual add and the next pre-norm; "
                        "default: off")
    p.add_argument("--ffn-act", choices=["swiglu", "geglu"], default="swiglu",
                   help="causal tiers: the gated FFN's activation, silu(gate) * up or gelu_tanh(gate) * up (the Gemma "
                        "FFN), dense and mixture-of-experts; default: swiglu")
    p.add_argument("--attn-softcap", type=float, default=0.0, metavar="C",
                   help="causal tiers: attention logit soft-capping, every score x becomes C * tanh(x / C) before the "
                        "softmax (Gemma-2 uses 50), in capped instantiations of the three attention kernels; not "
                        "together with --attn-sinks; default: 0 = off")
    p.add_argument("--final-softcap", type=float, default=0.0, metavar="C",
                   help="causal tiers: final-logit soft-capping, the LM-head loss is formed from C * tanh(logits / C) "
                        "(Gemma-2 / Gemma-3 use 30), in capped instantiations of the three loss kernels; default: "
                        "0 = off")
    p.add_argument("--lm-z-loss-coef", type=float, default=0.0, metavar="B",
                   help="causal tiers: add B times the mean over the valid rows of logsumexp(logits)^2 to the LM-head "
                        "loss (PaLM / OLMo-2 / Chameleon use about 1e-4), inside the loss kernels; the reported loss "
                        "is the total; default: 0 = off")
    p.add_argument("--synthetic", action="store_true", help="accepted for compatibility (data is always synthetic)")
    # training
    p.add_argument("--steps", type=int, required=True)
    p.add_argument("--warmup-steps", type=int, default=5)
    p.add_argument("--per-device-batch", type=int, required=True)
    p.add_argument("--grad-accum", type=int, required=True)
    # configs
    p.add_argument("--deepspeed-config", type=str, default=None, help="DeepSpeed JSON (read without DeepSpeed)")
    p.add_argument("--fsdp-config", type=str, default=None, help="FSDP YAML (honoured, unlike the reference)")
    # output
    p.add_argument("--results-dir", type=str, required=True)
    # MI355X extras
    p.add_argument("--accum-semantics", choices=["reference", "uniform"], default="reference")
    p.add_argument("--ddp-shard-optimizer", action="store_true",
                   help="ddp: shard the AdamW state over the ranks (torch DDP + ZeroRedundancyOptimizer): "
                        "reduce-scatter + all-gather instead of all-reduce, same update")
    p.add_argument("--grad-reduce", choices=["micro", "window"], default="micro",
                   help="ZeRO-2 gradient reduce-scatter every micro-step (DeepSpeed) or once per "
                        "accumulation window")
    p.add_argument("--optimizer-state", choices=["fp32", "fp8"], default="fp32",
                   help="AdamW moments: fp32, or fp8 = block-scaled OCP E4M3 codes (one byte per element for exp_avg "
                        "and for sqrt(exp_avg_sq), one fp32 power-of-two scale per 256 elements, stochastic "
                        "rounding): 6 bytes of optimizer state per parameter instead of 12; master weights stay "
                        "fp32; every strategy and tier")
    p.add_argument("--grad-comm-dtype", choices=["auto", "bf16", "fp16", "fp32"], default="auto",
                   help="DDP gradient all-reduce dtype: the compute dtype or fp32; auto = fp32 when DDP "
                        "runs the reference's fp16 path (torch DDP reduces fp32 grads), else the compute dtype")
    p.add_argument("--dtype", choices=["auto"] + list(DTYPES), default="auto",
                   help="compute dtype; auto = the reference's precision per strategy: fp16 + dynamic loss "
                        "scaling for ddp / fsdp (autocast + GradScaler), bf16 for zero2 / zero3 (DS configs)")
    p.add_argument("--device", choices=["cuda", "cpu"], default="cuda" if torch.cuda.is_available() else "cpu")
    p.add_argument("--bucket-mb", type=float, default=None,
                   help="gradient bucket cap (MiB); default: comm.topology.recommend_bucket_mb(world), "
                        "from the measured xGMI sweep (profiles/xgmi_buckets.json) when present")
    p.add_argument("--strategy-label", type=str, default=None,
                   help="name of this run in the result record / file name / CSV (e.g. fsdp_root, "
                        "ddp_uniform); default: --strategy")
    p.add_argument("--dropout", type=float, default=None, help="override the model dropout (reference: 0.1)")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--data-loader", choices=["device", "host"], default="device")
    p.add_argument("--profile", type=str, default=None, help="write a torch.profiler chrome trace to this dir")
    p.add_argument("--profile-steps", type=int, default=3)
    p.add_argument("--phase-timers", action="store_true",
                   help="per-phase times (forward / backward / exposed comm wait / optimizer) from HIP events; "
                        "runs eagerly (a graph replay has no phase boundaries)")
    p.add_argument("--debug-collectives", action="store_true", help="TORCH_DISTRIBUTED_DEBUG=DETAIL")
    p.add_argument("--fail-at-step", type=int, default=None, help="inject a failure (tests the suite runner)")
    p.add_argument("--timeout-min", type=int, default=30, help="collective timeout")
    p.add_argument("--log-every", type=int, default=None,
                   help="log cadence in steps (default: the DeepSpeed config's steps_per_print, else 10)")
    p.add_argument("--no-extended", action="store_true", help="do not write the extended sidecar")
    p.add_argument("--resume", type=str, default=None, help="load a sharded checkpoint dir before training")
    p.add_argument("--save-dir", type=str, default=None, help="write a sharded checkpoint at the end (window boundary)")
    p.add_argument("--export-model", type=str, default=None, help="write the consolidated bf16 model (.safetensors)")
    p.add_argument("--graphs", default="auto", choices=["auto", "on", "off"],
                   help="replay micro-steps as captured HIP graphs (parallel/graphs.py; off with --profile)")
    p.add_argument("--tunableop", default="auto", choices=["auto", "use", "tune", "off"],
                   help="hipBLASLt GEMM solutions (TunableOp results shipped in configs/tunableop)")
    p.add_argument("--strict-kernels", action="store_true",
                   help="a GPU product that would run as a plain torch GEMM (torch_gemm_fallbacks) is an error")
    return p


def _engine_for(args, model, device):
    ds = fc = None
    if args.strategy in ("zero2", "zero3"):
        path = args.deepspeed_config or default_config_path(args.strategy)
        ds = load_deepspeed_config(path)
        # train_harness.py:251-262: batch keys are injected at runtime
        for k in ("train_batch_size", "train_micro_batch_size_per_gpu", "gradient_accumulation_steps"):
            ds.pop(k, None)
    if args.strategy == "fsdp":
        path = args.fsdp_config or default_config_path("fsdp")
        if path and os.path.exists(path):
            fc = load_fsdp_config(path)
        if getattr(args, "fsdp_wrap", None) == "root":      # the reference's single root FlatParameter
            fc = dict(fc or {}, auto_wrap_policy="size_based")
        if getattr(args, "fsdp_sharding", None):            # bench.py --fsdp-sharding (FSDP sharding_strategy)
            fc = dict(fc or {}, sharding_strategy=args.fsdp_sharding)
    cfg = engine_config(args.strategy, args.grad_accum, args.accum_semantics, ds, fc,
                        compute_dtype=DTYPES[args.dtype], bucket_mb=args.bucket_mb, seed=args.seed,
                        grad_reduce=getattr(args, "grad_reduce", "micro"),
                        optimizer_state=getattr(args, "optimizer_state", "fp32"))
    cfg.extra["grad_comm_dtype"] = "fp32" if getattr(args, "grad_comm_dtype", None) == "fp32" else "compute"
    if args.strategy == "ddp" and getattr(args, "ddp_shard_optimizer", False):
        cfg.extra["shard_optimizer"] = True       # DDP + ZeroRedundancyOptimizer (parallel/replicated.py)
    return make_engine(model, cfg, device), cfg


def tokens_per_micro_step(per_device_batch, seq_len, world, cp=1):
    """Tokens one micro-step processes over all ranks: the ranks of a context-parallel group share their rows,
    each holding seq_len / cp tokens of them."""
    return per_device_batch * (seq_len // cp) * world


def check_context_parallel(cp, layout, world, mcfg, seq_len):
    """The layout ``--context-parallel`` runs with; ValueError when the job cannot run context-parallel."""
    _context.check_world(cp, world)
    layout = _context.resolve_layout(layout, mcfg.sliding_window)
    if cp > 1:
        if not mcfg.causal:
            raise ValueError("--context-parallel needs a causal tier (M7B, M7B_narrow, mtiny); the TinyGPT tiers "
                             "attend non-causally, with dropout and learned positions")
        _context.check_divisible(layout, seq_len, cp)
    return layout


def check_activation_recompute(mode, mcfg, tier):
    """ValueError when ``--activation-recompute`` is set for a tier whose layers cannot drop activations."""
    if mode != "off" and not mcfg.causal:
        raise ValueError(f"--activation-recompute needs a causal tier (M7B, M7B_narrow, mtiny); tier {tier} keeps "
                         "its activations in layer-strided buffers that its window-wide weight-gradient queue reads")


def check_head_chunk(n, mcfg, tier):
    """ValueError when ``--head-chunk`` is set for a tier without the chunked head, or to a value it cannot take."""
    if n is None:
        return
    if not mcfg.causal:
        raise ValueError(f"--head-chunk needs a causal tier (M7B, M7B_narrow, mtiny); tier {tier} ties its head to "
                         "the token embedding and has no chunked head")
    if n <= 0 or n % 16:
        raise ValueError(f"--head-chunk must be a positive multiple of 16, got {n}")


def check_qk_norm(on, mcfg, tier):
    """ValueError when ``--qk-norm`` is set for a tier without RoPE attention; sets it on ``mcfg``."""
    if not on:
        return
    if not mcfg.causal:
        raise ValueError(f"--qk-norm needs a causal tier (M7B, M7B_narrow, mtiny); tier {tier} has the reference's "
                         "attention with learned positions and no RoPE")
    mcfg.qk_norm = True
    mcfg.validate()


def check_sandwich_norm(on, mcfg, tier):
    """ValueError when ``--sandwich-norm`` is set for a tier without the causal decoder block; sets it on ``mcfg``."""
    if not on:
        return
    if not mcfg.causal:
        raise ValueError(f"--sandwich-norm needs a causal tier (M7B, M7B_narrow, mtiny); tier {tier} has the "
                         "reference's LayerNorm block")
    mcfg.sandwich_norm = True
    mcfg.validate()


def check_ffn_act(act, mcfg, tier):
    """ValueError when ``--ffn-act`` is not swiglu for a tier without the gated FFN; sets it on ``mcfg``."""
    act = act or "swiglu"
    if act == "swiglu":
        return
    if not mcfg.causal:
        raise ValueError(f"--ffn-act {act} needs a causal tier (M7B, M7B_narrow, mtiny); tier {tier} has the "
                         "reference's GELU MLP without a gate")
    mcfg.ffn_act = act
    mcfg.validate()


def check_attn_sinks(on, mcfg, tier):
    """ValueError when ``--attn-sinks`` is set for a tier without causal attention; sets it on ``mcfg``."""
    if not on:
        return
    if not mcfg.causal:
        raise ValueError(f"--attn-sinks needs a causal tier (M7B, M7B_narrow, mtiny); tier {tier} has the reference's "
                         "non-causal attention with dropout")
    mcfg.attn_sinks = True
    mcfg.validate()


def check_attn_softcap(cap, sinks, mcfg, tier):
    """ValueError when ``--attn-softcap`` is not a finite number >= 0, is set for a tier without causal attention or
    together with ``--attn-sinks``; sets it on ``mcfg``."""
    cap = float(cap or 0.0)
    if cap == 0.0:
        return
    if not math.isfinite(cap) or cap < 0:
        raise ValueError(f"--attn-softcap must be a finite number >= 0 (0 = off), got {cap}")
    if not mcfg.causal:
        raise ValueError(f"--attn-softcap needs a causal tier (M7B, M7B_narrow, mtiny); tier {tier} has the "
                         "reference's non-causal attention with dropout")
    if sinks:
        raise ValueError("--attn-softcap together with --attn-sinks is not supported")
    mcfg.attn_softcap = cap
    mcfg.validate()


def check_final_softcap(cap, mcfg, tier):
    """ValueError when ``--final-softcap`` is not a finite number >= 0 or is set for a tier without the untied causal
    head; sets it on ``mcfg``."""
    cap = float(cap or 0.0)
    if cap == 0.0:
        return
    if not math.isfinite(cap) or cap < 0:
        raise ValueError(f"--final-softcap must be a finite number >= 0 (0 = off), got {cap}")
    if not mcfg.causal:
        raise ValueError(f"--final-softcap needs a causal tier (M7B, M7B_narrow, mtiny); tier {tier} has the "
                         "reference's plain softmax cross-entropy on its tied head")
    mcfg.final_softcap = cap
    mcfg.validate()


def check_lm_z_loss(coef, mcfg, tier):
    """ValueError when ``--lm-z-loss-coef`` is not a finite number >= 0 or is set for a tier without the untied causal
    head; sets it on ``mcfg``."""
    coef = float(coef or 0.0)
    if coef == 0.0:
        return
    if not math.isfinite(coef) or coef < 0:
        raise ValueError(f"--lm-z-loss-coef must be a finite number >= 0 (0 = off), got {coef}")
    if not mcfg.causal:
        raise ValueError(f"--lm-z-loss-coef needs a causal tier (M7B, M7B_narrow, mtiny); tier {tier} has the "
                         "reference's plain softmax cross-entropy on its tied head")
    mcfg.lm_z_loss_coef = coef
    mcfg.validate()


def check_moe(experts, top_k, factor, recompute, mcfg, tier, aux_coef=None, z_coef=None, dropless=False):
    """ValueError when the ``--moe-*`` flags are set for a tier without the routed FFN or together with
    ``--activation-recompute``, or ``--moe-dropless`` together with an explicit ``--moe-capacity-factor``; sets them
    on ``mcfg`` (whose ``validate`` refuses out-of-range values)."""
    if dropless:
        if not mcfg.causal:
            raise ValueError(f"--moe-dropless needs --moe-experts on a causal tier (M7B, M7B_narrow, mtiny); tier "
                             f"{tier} has the reference's dense GELU MLP")
        if experts is None:
            raise ValueError("--moe-dropless is only used together with --moe-experts")
        if factor is not None:
            raise ValueError(f"--moe-dropless has no capacity: --moe-capacity-factor {factor} cannot be given with it")
    losses = " / ".join(flag for flag, v in (("--moe-aux-loss-coef", aux_coef), ("--moe-z-loss-coef", z_coef))
                        if v is not None)
    if losses and not mcfg.causal:
        raise ValueError(f"{losses}: the router losses need --moe-experts on a causal tier (M7B, M7B_narrow, mtiny); "
                         f"tier {tier} has the reference's dense GELU MLP")
    if experts is None:
        if top_k is not None or factor is not None:
            raise ValueError("--moe-top-k / --moe-capacity-factor are only used together with --moe-experts")
        if losses:
            raise ValueError(f"{losses}: only used together with --moe-experts")
        return
    if not mcfg.causal:
        raise ValueError(f"--moe-experts needs a causal tier (M7B, M7B_narrow, mtiny); tier {tier} has the "
                         "reference's dense GELU MLP")
    if recompute != "off":
        raise ValueError(f"--activation-recompute {recompute} is not supported together with --moe-experts")
    mcfg.n_experts = experts
    if top_k is not None:
        mcfg.moe_top_k = top_k
    if factor is not None:
        mcfg.moe_capacity_factor = factor
    if dropless:
        mcfg.moe_dropless = True
    for flag, name, v in (("--moe-aux-loss-coef", "moe_aux_loss_coef", aux_coef),
                          ("--moe-z-loss-coef", "moe_z_loss_coef", z_coef)):
        if v is not None:
            if not 0.0 <= v < float("inf"):
                raise ValueError(f"{flag} must be a finite number >= 0, got {v!r}")
            setattr(mcfg, name, v)
    mcfg.validate()


def train(args):
    world, rank, local_rank = resolve_ranks(args.world_size, args.rank, args.local_rank)
    args.world_size, args.rank, args.local_rank = world, rank, local_rank
    cp_n = int(getattr(args, "context_parallel", 1) or 1)
    _context.check_world(cp_n, world)
    auto_bucket = args.bucket_mb is None
    label = args.strategy_label or args.strategy
    if not args.strategy_label and args.strategy == "ddp" and getattr(args, "ddp_shard_optimizer", False):
        label = "ddp_zero1"          # DDP + sharded optimizer state: its own row in metrics.csv
    ds_cfg = None
    if args.strategy in ("zero2", "zero3"):
        ds_cfg = load_deepspeed_config(args.deepspeed_config or default_config_path(args.strategy))
    if args.dtype == "auto":
        args.dtype = "fp16" if args.strategy in ("ddp", "fsdp") else ds_precision(ds_cfg)
    if args.log_every is None:               # DeepSpeed's steps_per_print (zero2/3.json: 10)
        args.log_every = int((ds_cfg or {}).get("steps_per_print", 10))
    if (ds_cfg or {}).get("wall_clock_breakdown"):
        args.phase_timers = True             # DeepSpeed's wall-clock breakdown: per-phase HIP-event timers
    if args.grad_comm_dtype == "auto":
        args.grad_comm_dtype = "fp32" if (args.strategy == "ddp" and args.dtype == "fp16") else args.dtype
    if args.grad_comm_dtype not in ("fp32", args.dtype):
        raise ValueError(f"--grad-comm-dtype {args.grad_comm_dtype}: must be fp32 or the compute dtype {args.dtype}")
    device = setup_distributed(world, rank, local_rank, args.master_addr, args.master_port, args.device,
                               args.timeout_min, args.debug_collectives)
    is_main = rank == 0
    fabric = None
    strict_before = _functional.strict_kernels       # --strict-kernels holds for this run only
    if auto_bucket:
        from .comm.topology import calibrate_fabric, measured_params, recommend_bucket_mb
        if (world > 1 and measured_params(world)[2] == "default"
                and (device.type != "cuda" or os.environ.get("DLTB_COMM", "rccl") != "host")):
            # this job's own collective alpha-beta before the engine plans its buckets (bench.py does the same)
            fabric = calibrate_fabric(device, sizes_mb=(4, 16, 64) if device.type == "cuda" else (0.25, 1.0))
        args.bucket_mb = recommend_bucket_mb(world)
    try:
        _functional.strict_kernels = strict_before or bool(getattr(args, "strict_kernels", False))
        if device.type == "cuda" and not ext_available():
            raise RuntimeError("dltb._C is not built: run `python csrc/build.py` (the GPU path has no fallback)")
        gemm_mode = setup_tunableop(args.tunableop if (args.tunableop != "tune" or is_main) else "use") \
            if device.type == "cuda" else "off"
        torch.manual_seed(args.seed)        # identical init on every rank (the reference uses 42+rank + DDP broadcast)
        if is_main:
            print("\n" + "=" * 80)
            print(f"Benchmark Config: {args.strategy.upper()} | Tier {args.tier} | WS={world} | SeqLen={args.seq_len}")
            print("=" * 80 + "\n", flush=True)
        mcfg = get_model_config(args.tier, args.seq_len)
        if args.dropout is not None:
            mcfg.dropout = args.dropout
        if getattr(args, "sliding_window", None) is not None:
            mcfg.sliding_window = args.sliding_window
            mcfg.validate()
        doc_len = getattr(args, "doc_len", None)
        eos_id = None
        if doc_len is not None:
            eos_id = args.eos_id if getattr(args, "eos_id", None) is not None else mcfg.vocab_size - 1
            mcfg.doc_eos_id = eos_id
            mcfg.validate()
        cp_layout = check_context_parallel(cp_n, getattr(args, "cp_layout", "auto"), world, mcfg, args.seq_len)
        recompute = getattr(args, "activation_recompute", None) or "off"
        check_activation_recompute(recompute, mcfg, args.tier)
        head_chunk = getattr(args, "head_chunk", None)
        check_head_chunk(head_chunk, mcfg, args.tier)
        check_moe(getattr(args, "moe_experts", None), getattr(args, "moe_top_k", None),
                  getattr(args, "moe_capacity_factor", None), recompute, mcfg, args.tier,
                  getattr(args, "moe_aux_loss_coef", None), getattr(args, "moe_z_loss_coef", None),
                  bool(getattr(args, "moe_dropless", False)))
        check_qk_norm(bool(getattr(args, "qk_norm", False)), mcfg, args.tier)
        check_attn_sinks(bool(getattr(args, "attn_sinks", False)), mcfg, args.tier)
        check_sandwich_norm(bool(getattr(args, "sandwich_norm", False)), mcfg, args.tier)
        check_ffn_act(getattr(args, "ffn_act", "swiglu"), mcfg, args.tier)
        check_attn_softcap(getattr(args, "attn_softcap", 0.0), bool(getattr(args, "attn_sinks", False)), mcfg,
                           args.tier)
        check_final_softcap(getattr(args, "final_softcap", 0.0), mcfg, args.tier)
        check_lm_z_loss(getattr(args, "lm_z_loss_coef", 0.0), mcfg, args.tier)
        with torch.device(device):      # init directly on the GPU (no fp32 host copy of a 7B model)
            model = build_model(mcfg)
        if recompute != "off":          # a layout like cp, not a model property: the harness sets it on the model
            model.activation_recompute = recompute
            if is_main:
                print(f"Activation recompute: {recompute}", flush=True)
        head_rows = args.per_device_batch * (args.seq_len // cp_n)      # the rows the head sees per micro-step
        n_head_chunks = 1
        if head_chunk is not None:
            from .models.mistral import head_chunks
            model.head_chunk = head_chunk
            n_head_chunks = head_chunks(head_rows, head_chunk)
            if is_main:
                print(f"Head chunk: {head_chunk} rows, {n_head_chunks} chunk(s) of the {head_rows} rows per micro-step"
                      + ("" if n_head_chunks > 1 else " (one chunk holds them all: the unchunked head runs)"),
                      flush=True)
        if mcfg.n_experts and mcfg.moe_dropless and is_main:
            from .ops.ref import moe_dropless_rows
            print(f"Mixture of experts: {mcfg.n_experts} experts, top-{mcfg.moe_top_k}, dropless: "
                  f"{moe_dropless_rows(head_rows, mcfg.n_experts, mcfg.moe_top_k)} packed slot rows (R) for the "
                  f"{head_rows} rows per micro-step, grouped GEMMs, load-balancing loss coefficient "
                  f"{mcfg.moe_aux_loss_coef}, router z-loss coefficient {mcfg.moe_z_loss_coef}", flush=True)
        elif mcfg.n_experts and is_main:
            from .ops.ref import moe_capacity
            print(f"Mixture of experts: {mcfg.n_experts} experts, top-{mcfg.moe_top_k}, capacity "
                  f"{moe_capacity(head_rows, mcfg.n_experts, mcfg.moe_top_k, mcfg.moe_capacity_factor)} slots per "
                  f"expert for the {head_rows} rows per micro-step (factor {mcfg.moe_capacity_factor}), "
                  f"load-balancing loss coefficient {mcfg.moe_aux_loss_coef}, router z-loss coefficient "
                  f"{mcfg.moe_z_loss_coef}", flush=True)
        if mcfg.qk_norm and is_main:
            print(f"QK-norm: RMSNorm over head_dim {mcfg.head_dim} on q and k, fused with RoPE", flush=True)
        if (mcfg.sandwich_norm or mcfg.ffn_act != "swiglu") and is_main:
            print(f"decoder block: sandwich norms {'on' if mcfg.sandwich_norm else 'off'} (an RMSNorm on every "
                  f"sublayer's output before the residual add), gated FFN activation {mcfg.ffn_act}", flush=True)
        if mcfg.attn_sinks and is_main:
            print(f"attention sinks: one learned logit per query head ({mcfg.n_head} per layer)", flush=True)
        if mcfg.attn_softcap and is_main:
            print(f"attention soft-capping: scores capped to {mcfg.attn_softcap:g} * tanh(x / {mcfg.attn_softcap:g})",
                  flush=True)
        if mcfg.final_softcap and is_main:
            print(f"final-logit soft-capping: the loss is formed from {mcfg.final_softcap:g} * tanh(logits / "
                  f"{mcfg.final_softcap:g})", flush=True)
        if getattr(args, "optimizer_state", "fp32") == "fp8" and is_main:
            print("optimizer state: AdamW moments as block-scaled FP8 (E4M3) codes, stochastically rounded; master "
                  "weights fp32", flush=True)
        if mcfg.lm_z_loss_coef and is_main:
            print(f"LM-head z-loss: {mcfg.lm_z_loss_coef:g} * mean(logsumexp(logits)^2) over the valid rows, included "
                  "in the reported loss", flush=True)
        cp = None
        if cp_n > 1:
            cp = _context.ContextParallel(cp_n, cp_layout, mcfg.sliding_window, world, rank)
            cp.attach(model)
            if is_main:
                print(f"Context parallel: groups of {cp_n} ranks, {cp.layout} layout, rank 0 ranges "
                      f"{cp.ranges(args.seq_len)}", flush=True)
        n_params = model.num_params()
        if is_main:
            print(f"Model initialized: {n_params / 1e6:.2f}M parameters", flush=True)
        engine, ecfg = _engine_for(args, model, device)
        if is_main:
            print(f"[Rank {rank}] engine={type(engine).__name__} accum={engine.accum} clip={ecfg.grad_clip} "
                  f"sched={'WarmupLR' if ecfg.scheduler else 'constant'} dtype={engine.compute_dtype}", flush=True)
        ds = SyntheticDataset(mcfg.vocab_size, args.seq_len, size=1000, seed=42, doc_len=doc_len, eos_id=eos_id)
        if is_main:
            print(f"SyntheticDataset: {len(ds)} samples, seq_len={args.seq_len}"
                  + (f", documents of mean length {doc_len} ending in token {eos_id}" if doc_len else ""), flush=True)
        # the ranks of a context-parallel group draw the same rows: the batcher sees the groups
        batches = make_batcher(args.data_loader, ds, args.per_device_batch, world // cp_n, rank // cp_n,
                               args.strategy, device)
        if device.type == "cuda":
            torch.cuda.reset_peak_memory_stats(device)
        if is_main:
            print(f"Starting training: {args.steps} steps, warmup={args.warmup_steps}")
            print(f"Per-device batch: {args.per_device_batch}, Grad accum: {args.grad_accum}\n", flush=True)
        if args.resume:
            meta = load_checkpoint(engine, args.resume)
            if is_main:
                print(f"Resumed from {args.resume}: optimizer step {meta['opt_steps']}", flush=True)
        engine.train()
        # (auto: a warm-up no longer than one accumulation window would put the graph capture, at the
        # first window start after an eager window, inside the timed steps -> eager; as fast)
        short_warmup = (args.graphs == "auto" and args.warmup_steps <= engine.accum
                        and os.environ.get("DLTB_GRAPHS") is None)
        # (context parallel: eager -- the group's gather / reduce-scatter are waited for on the host)
        runner = GraphedStep(engine) if (graphs_enabled(args.graphs, device, world) and not args.profile
                                         and not args.phase_timers and not short_warmup and cp is None) else None
        timers = PhaseTimers(device) if args.phase_timers else None
        timed_n = max(0, args.steps - args.warmup_steps)
        # per-step losses are COPIED into a device buffer: a graph replay returns the same static
        # loss tensor for every replay of a window position, so keeping the tensors would alias
        loss_hist = torch.zeros(max(1, timed_n), dtype=torch.float32, device=device)
        n_loss = 0
        step_events = []
        host_times = []
        prof = None
        t_start = None
        t_log = [time.perf_counter(), 0]
        sync = (lambda: torch.cuda.synchronize(device)) if device.type == "cuda" else (lambda: None)
        for step in range(args.steps):
            if step == args.warmup_steps:
                barrier()
                sync()
                engine.comm.reset_stats()     # wire accounting over the timed steps only
                if cp is not None:
                    cp.comm.reset_stats()
                t_start = time.perf_counter()
                if args.profile and is_main:
                    from torch.profiler import ProfilerActivity, profile
                    prof = profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], record_shapes=False)
                    prof.__enter__()
            if args.fail_at_step is not None and step == args.fail_at_step:
                raise RuntimeError(f"injected failure at step {step} (--fail-at-step)")
            batch = next(batches)
            targets = batch          # unshifted targets = inputs (train_harness.py:359)
            ev0 = ev1 = None
            if device.type == "cuda" and step >= args.warmup_steps:
                ev0 = torch.cuda.Event(enable_timing=True)
                ev1 = torch.cuda.Event(enable_timing=True)
                ev0.record()
            h0 = time.perf_counter()
            timed_phase = timers is not None and step >= args.warmup_steps
            if timed_phase:
                engine.timers = timers
                timers.begin_step()
            if runner is not None:
                loss = runner(batch, targets)
            else:
                loss = engine(batch, targets)[1]
                if timed_phase:
                    timers.mark("fwd_end")
                engine.backward(loss)
                if timed_phase:
                    timers.mark("bwd_end")
                engine.step()
            if timed_phase:
                timers.end_step()
                engine.timers = None
            h1 = time.perf_counter()
            if ev1 is not None:
                ev1.record()
                step_events.append((ev0, ev1))
            if step >= args.warmup_steps:
                loss_hist[n_loss].copy_(loss.detach().reshape(()))
                n_loss += 1
                host_times.append(h1 - h0)
            if prof is not None and step >= args.warmup_steps + args.profile_steps - 1:
                sync()
                prof.__exit__(None, None, None)
                os.makedirs(args.profile, exist_ok=True)
                prof.export_chrome_trace(os.path.join(args.profile, f"trace_{label}_ws{world}_rank{rank}.json"))
                prof = None
            if is_main and args.log_every and step % args.log_every == 0:
                lv = loss.item()             # synchronises: Time is the mean device-synchronised
                now = time.perf_counter()    # step time since the previous log line
                dt = (now - t_log[0]) / max(1, step - t_log[1]) if step > 0 else h1 - h0
                t_log[:] = [now, step]
                print(f"[Step {step:04d}] Loss: {lv:.4f}, Time: {dt:.4f}s", flush=True)
        barrier()
        sync()
        timed = args.steps - args.warmup_steps
        # the timed region ends here: finalize / checkpoint / export below are not step time
        wall = (time.perf_counter() - t_start) if (t_start is not None and timed > 0) else 0.0
        wall = all_reduce_max(wall, device)
        engine.finalize()            # a deferred optimizer step of the last window (outside the timed region)
        if args.save_dir:
            if engine.micro % engine.accum == 0:
                save_checkpoint(engine, args.save_dir, {"tier": args.tier, "seq_len": args.seq_len})
                if is_main:
                    print(f"Checkpoint written to {args.save_dir}", flush=True)
            elif is_main:
                print("WARNING: --save-dir skipped: the run did not end on an accumulation boundary", flush=True)
        if args.export_model:
            export_consolidated(engine, args.export_model)
        cp_ops = {k: dict(v) for k, v in cp.comm.stats.items()} if cp is not None else None
        if cp is not None and n_loss:
            # a rank's loss is the mean over its slice of the rows: the group's mean is the rows' loss (one
            # collective, after the timed region)
            cp.comm.all_reduce(loss_hist, op="sum", async_op=False)
            loss_hist /= cp_n
        mean_step = wall / timed if timed > 0 else 0.0
        mean_loss = float(loss_hist[:n_loss].mean().item()) if n_loss else 0.0
        peak = torch.cuda.max_memory_allocated(device) if device.type == "cuda" else 0
        record = make_record(label, world, rank, args.seq_len, args.tier, args.steps,
                             args.per_device_batch, args.grad_accum, mean_step, mean_loss, peak)
        ev_times = [a.elapsed_time(b) / 1e3 for a, b in step_events] if step_events else []
        tokens_step = tokens_per_micro_step(args.per_device_batch, args.seq_len, world, cp_n)
        if cp_n > 1 and mean_step > 0:
            # the record's formula counts per_device_batch * seq_len per rank; a context-parallel rank holds
            # seq_len / N of its rows (the keys stay the reference's)
            record["tokens_per_sec"] = tokens_step / mean_step
            record["h2d_gbps_per_gpu"] = record["h2d_gbps_per_gpu"] / cp_n
        # a document mask depends on the data: count the table's visible pairs (window included), as the window
        # formula counts its band
        pairs = ds.visible_pairs_per_row(mcfg.sliding_window) if doc_len is not None else None
        flops_tok = mcfg.train_flops_per_token(args.seq_len, pairs)
        tflops_gpu = (tokens_step / world) * flops_tok / mean_step / 1e12 if mean_step > 0 else 0.0
        extended = {
            "record_file_semantics": "tokens_per_sec = per_device_batch*seq_len*world_size / mean_step_time_sec "
                                     "(reference formula; one micro-batch per step)"
                                     + (f"; divided by context_parallel = {cp_n}: the ranks of a group share rows"
                                        if cp_n > 1 else ""),
            "context_parallel": cp_n, "cp_layout": cp_layout if cp_n > 1 else None,
            "activation_recompute": recompute,
            "head_chunk": head_chunk, "head_chunks": n_head_chunks,
            "attn_sinks": bool(mcfg.attn_sinks),
            "sandwich_norm": bool(mcfg.sandwich_norm), "ffn_act": str(mcfg.ffn_act),
            "attn_softcap": float(mcfg.attn_softcap),
            "final_softcap": float(mcfg.final_softcap),
            "lm_z_loss_coef": float(mcfg.lm_z_loss_coef),
            "optimizer_state": engine.opt.state, "optimizer_bytes": engine.opt.state_bytes,
            # the last micro-step's assignments per layer and expert (before drops) and, with an auxiliary router
            # loss on, its per-layer values, read once, here
            "moe": model.moe_stats(head_rows) if mcfg.n_experts else None,
            "cp_ranges": (cp.describe(args.seq_len)["cp_ranges"] if cp is not None else None),
            "tokens_per_micro_step": tokens_step,
            "timing": "barrier + device sync around the timed region; max over ranks (reference: rank-0 host "
                      "perf_counter without sync)",
            "wall_time_timed_sec": wall, "timed_steps": timed,
            "host_step_time_mean_sec": (sum(host_times) / len(host_times)) if host_times else 0.0,
            "device_step_time_p50_sec": sorted(ev_times)[len(ev_times) // 2] if ev_times else None,
            "device_step_time_max_sec": max(ev_times) if ev_times else None,
            "tflops_per_gpu": tflops_gpu, "mfu_vs_2.5PF_dense_bf16": tflops_gpu * 1e12 / MI355X_DENSE_BF16_FLOPS,
            "train_flops_per_token": flops_tok, "params": n_params, "trainable_params": n_params,
            "model": mcfg.to_dict(), "engine": type(engine).__name__,
            "data": {"doc_len": doc_len, "eos_id": eos_id,
                     # visible (query, key) pairs of the table over the causal T (T + 1) / 2
                     "visible_pair_fraction": (pairs / (args.seq_len * (args.seq_len + 1) / 2.0)
                                               if pairs is not None else None)},
            "hip_graphs": bool(runner is not None and runner.graphs and not runner.disabled),
            "engine_config": {k: (str(v) if isinstance(v, torch.dtype) else v) for k, v in vars(ecfg).items()},
            "optimizer_steps": engine.opt_steps, "last_lr": engine.last_lr,
            "grad_norm": float(engine.grad_norm.item()) if engine.grad_norm is not None else None,
            "comm_bytes_per_step_per_gpu": engine.comm_bytes_per_step,
            # measured by the comm layer (host-issued calls; graph replays issue none from Python)
            "comm_wire_bytes_per_step_measured": (engine.comm.wire_bytes() / timed
                                                  if timed > 0 and not (runner is not None and runner.graphs
                                                                        and not runner.disabled) else None),
            "comm_ops_timed": {k: dict(v) for k, v in engine.comm.stats.items()},
            "cp_comm_ops_timed": cp_ops,
            "comm_topology": comm_describe(world) if (is_main and device.type == "cuda") else None,
            "fabric_calibration": fabric,
            "memory": engine.memory_report(),
            "peak_vram_reserved_gb": (torch.cuda.max_memory_reserved(device) / 1e9) if device.type == "cuda" else 0.0,
            "accum_semantics": args.accum_semantics, "grad_reduce": args.grad_reduce, "dtype": args.dtype,
            "grad_comm_dtype": getattr(engine, "grad_comm_dtype", args.grad_comm_dtype), "strategy_engine": args.strategy, "bucket_mb": args.bucket_mb, "data_loader": args.data_loader,
            "kernels": so_path(), "platform": device_info(device), "gemm_tuning": gemm_mode,
            "torch_gemm_fallbacks": dict(torch_fallbacks) or None,
            "strict_kernels": bool(_functional.strict_kernels),
            "phase_times_ms": timers.summary() if timers is not None else None,
            "loss_scaler": engine.scaler.stats() if engine.scaler is not None else None,
            "deepspeed_config_keys": ecfg.extra.get("ds_keys") or None,
            "config_keys_ignored": sorted((ecfg.extra.get("ds_keys") or {}).get("ignored", {})),
        }
        if is_main:
            print_result(record)
            path = write_result(record, args.results_dir, None if args.no_extended else extended)
            print(f"Results saved to: {path}")
            print_markers(record)
        flush_tunableop()
        return record, extended
    finally:
        _functional.strict_kernels = strict_before
        cleanup_distributed()


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.sliding_window is not None:
        if args.sliding_window < 1:
            parser.error("--sliding-window must be >= 1")
        if not get_model_config(args.tier, args.seq_len).causal:
            parser.error(f"--sliding-window needs a causal tier; tier {args.tier} attends non-causally")
    if args.doc_len is not None:
        cfg0 = get_model_config(args.tier, args.seq_len)
        if args.doc_len < 1:
            parser.error("--doc-len must be >= 1")
        if not cfg0.causal:
            parser.error(f"--doc-len needs a causal tier; tier {args.tier} attends non-causally")
        if args.eos_id is not None and not 0 <= args.eos_id < cfg0.vocab_size:
            parser.error(f"--eos-id must be in [0, {cfg0.vocab_size}) for tier {args.tier}")
    elif args.eos_id is not None:
        parser.error("--eos-id is only used together with --doc-len")
    if args.context_parallel != 1:
        cfg0 = get_model_config(args.tier, args.seq_len)
        if args.sliding_window is not None:
            cfg0.sliding_window = args.sliding_window
        world0 = resolve_ranks(args.world_size, args.rank, args.local_rank)[0]
        try:
            check_context_parallel(args.context_parallel, args.cp_layout, world0, cfg0, args.seq_len)
        except ValueError as e:
            parser.error(str(e))
    try:
        check_activation_recompute(args.activation_recompute, get_model_config(args.tier, args.seq_len), args.tier)
    except ValueError as e:
        parser.error(str(e))
    try:
        check_head_chunk(args.head_chunk, get_model_config(args.tier, args.seq_len), args.tier)
    except ValueError as e:
        parser.error(str(e))
    try:
        check_moe(args.moe_experts, args.moe_top_k, args.moe_capacity_factor, args.activation_recompute,
                  get_model_config(args.tier, args.seq_len), args.tier, args.moe_aux_loss_coef,
                  args.moe_z_loss_coef, args.moe_dropless)
    except ValueError as e:
        parser.error(str(e))
    try:
        check_qk_norm(args.qk_norm, get_model_config(args.tier, args.seq_len), args.tier)
        check_attn_sinks(args.attn_sinks, get_model_config(args.tier, args.seq_len), args.tier)
        check_sandwich_norm(args.sandwich_norm, get_model_config(args.tier, args.seq_len), args.tier)
        check_ffn_act(args.ffn_act, get_model_config(args.tier, args.seq_len), args.tier)
        check_attn_softcap(args.attn_softcap, args.attn_sinks, get_model_config(args.tier, args.seq_len), args.tier)
        check_final_softcap(args.final_softcap, get_model_config(args.tier, args.seq_len), args.tier)
        check_lm_z_loss(args.lm_z_loss_coef, get_model_config(args.tier, args.seq_len), args.tier)
    except ValueError as e:
        parser.error(str(e))
    if args.strategy in ("zero2", "zero3") and not args.deepspeed_config:
        args.deepspeed_config = default_config_path(args.strategy)
        print(f"[dltb] --deepspeed-config not given; using {args.deepspeed_config}", flush=True)
    train(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
