"""Attention logit soft-capping on the MI355X: the CAP instantiations of the three kernels of csrc/attention.hip against
dltb.ops.ref on the same 16-bit inputs, at Gemma's cap, at a cap the scores saturate, and where the exp2 of the tanh
evaluation overflows; softcap = 0 against the call without the argument; the whole model against the CPU reference
path, recompute modes, HIP-graph replay, ZeRO-3 with context parallelism on two host-staged ranks, and one step with
QK-norm, dropless MoE and a chunked head.  The CPU definitions: tests/test_attn_softcap_cpu.py.

Shapes, comparison helper and tolerances are those of tests/test_attn_sinks_gpu.py: B = 2, T = 512 (four query
blocks, eight key tiles); (2, 2, 64) takes the three-way key-split merge and (8, 2, 128) the head-split dK/dV path;
lse 8e-3 / 1e-3, O 2e-2 / 3e-2, dq / dk / dv 5e-2 / 5e-2, no element outside.  The backward reference runs on the
kernel's own o and lse.  Model comparisons: loss within 1e-2 relative, every gradient within 6e-2 in the relative
2-norm (tests/test_attn_sinks_gpu.py, from tests/test_mistral_gpu.py); two ranks: its ``compare`` tolerances.
"""
import copy
import functools
import math

import pytest
import torch

import dltb  # noqa: F401
from dltb.data import SyntheticDataset
from dltb.models import build_model, get_model_config
from dltb.models.config import ModelConfig
from dltb.ops import functional as F_
from dltb.ops import ref
from dltb.ops._ext import ext
from dltb.ops.rng import StepSeed
from dltb.parallel import GraphedStep, ParamRuntime, engine_config, make_engine

from multirank_util import compare, run

pytestmark = pytest.mark.gpu
DEV = "cuda"
SITE = 11
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
FORMATS = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
B, T = 2, 512
HEADS = pytest.mark.parametrize("Hq,Hkv,D", [(2, 2, 64), (8, 2, 128)])
CASES = ["causal", "w1", "w65", "w200", "doc", "qrange"]
QRANGE = (128, 384)


def close(a, b, atol, rtol, what=""):
    assert torch.isfinite(a).all(), f"{what}: non-finite values in the kernel output"
    a = a.float()
    b = b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).float().mean().item()
    print(f"{what}: worst error/tolerance {float((err / tol).max()):.3f}")
    assert bad == 0.0, f"{what}: {bad*100:.3f}% elements out of tolerance, max err {err.max().item():.4g}"


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    C = ext()
    assert C.arch() == "gfx950"


def seed_obj(v=42):
    s = StepSeed(v, 0, device=DEV)
    s.next()
    return s


def split(t, Hq, Hkv, D):
    return t[:, :Hq * D], t[:, Hq * D:(Hq + Hkv) * D], t[:, (Hq + Hkv) * D:]


def rows(x, qb, qe):
    return x.view(B, T, -1)[:, qb:qe].reshape(B * (qe - qb), -1).contiguous()


@functools.lru_cache(maxsize=None)
def inputs(Hq, Hkv, D, dtype, qmul=1, planted=False):
    """(q, k, v, do) of one shape, N(0, 1) in the 16-bit format, shared (read-only) by every case that runs it.
    ``qmul``: q times a power of two (exact).  ``planted``: column 0 of every query head is +-128 and of every key
    head +-64 with random signs, so that every score is sign * 8192 / sqrt(D) plus the N(0, 64^2) rest (qmul = 64):
    at least 200 in magnitude, far past any saturation."""
    g = torch.Generator(device=DEV).manual_seed(B * 1000003 + T * 1009 + Hq * 101 + Hkv * 11 + D)
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, device=DEV, generator=g).to(dtype)
    do = torch.randn(B * T, Hq * D, device=DEV, generator=g).to(dtype)
    q, k, v = (t.contiguous() for t in split(qkv, Hq, Hkv, D))
    q = q * qmul
    if planted:
        sq = torch.randint(0, 2, (B * T, Hq), device=DEV, generator=g).to(dtype) * 2 - 1
        sk = torch.randint(0, 2, (B * T, Hkv), device=DEV, generator=g).to(dtype) * 2 - 1
        q.view(B * T, Hq, D)[:, :, 0] = 128 * sq
        k.view(B * T, Hkv, D)[:, :, 0] = 64 * sk
    return q, k, v, do


@functools.lru_cache(maxsize=None)
def mask_kw(case):
    """The attention arguments of a case; the document bounds come from a seeded packed table."""
    if case == "causal":
        return {}
    if case.startswith("w"):
        return {"window": int(case[1:])}
    if case == "qrange":
        return {"q_range": QRANGE}
    ds = SyntheticDataset(256, T, size=B, seed=7, doc_len=96)
    return {"bounds": F_.doc_bounds(ds.data[:B].to(DEV), ds.eos_id, 0)}


def operands(case, Hq, Hkv, D, dtype, **kw):
    q, k, v, do = inputs(Hq, Hkv, D, dtype, **kw)
    if case == "qrange":
        q, do = rows(q, *QRANGE), rows(do, *QRANGE)
    return q, k, v, do


def run_kernels(q, k, v, do, Hq, Hkv, D, case, **cap):
    """(o, lse, dq, dk, dv) through F_.attn_fwd / F_.attn_bwd; the gradients start as NaN: every element must be
    written."""
    scale = 1.0 / math.sqrt(D)
    o, lse, _ = F_.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.0, seed_obj(), SITE, **cap, **mask_kw(case))
    dq = torch.full_like(q, float("nan"))
    dk = torch.full_like(k, float("nan"))
    dv = torch.full_like(v, float("nan"))
    assert F_.attn_bwd(q, k, v, o, do, lse, None, dq, dk, dv, B, T, Hq, Hkv, scale, True, 0.0, seed_obj(), SITE,
                       **cap, **mask_kw(case)) is None
    return o, lse, dq, dk, dv


def against_ref(q, k, v, do, Hq, Hkv, D, case, cap, what):
    """The five comparisons of tests/test_attn_sinks_gpu.py; returns the kernel's and the reference's (o, lse)."""
    kw = mask_kw(case)
    scale = 1.0 / math.sqrt(D)
    Tq = q.shape[0] // B
    o, lse, dq, dk, dv = run_kernels(q, k, v, do, Hq, Hkv, D, case, softcap=cap)
    assert o.dtype == q.dtype and o.shape == (B * Tq, Hq * D) and lse.shape == (B, Hq, Tq) and lse.dtype == F32
    sd = seed_obj()
    ro, rlse = ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.0, sd, SITE, softcap=cap, **kw)
    close(lse, rlse, 8e-3, 1e-3, f"{what} lse")
    close(o, ro, 2e-2, 3e-2, f"{what} O")
    rdq, rdk, rdv = torch.empty_like(dq), torch.empty_like(dk), torch.empty_like(dv)
    ref.attn_bwd(q, k, v, o, do, lse, rdq, rdk, rdv, B, T, Hq, Hkv, scale, True, 0.0, sd, SITE, softcap=cap, **kw)
    for name, a, b in zip("qkv", (dq, dk, dv), (rdq, rdk, rdv)):
        close(a, b, 5e-2, 5e-2, f"{what} d{name}")
    return o, lse, ro, rlse


def visible_scores(q, k, Hq, Hkv, D, case):
    """The raw scores x of the visible pairs, from the reference alone."""
    kw = dict(mask_kw(case))
    qb, qe = kw.pop("q_range", (0, T))
    s = ref._attn_probs(q, k, B, T, Hq, Hkv, D, 1.0 / math.sqrt(D), True, kw.get("window", 0), kw.get("bounds"), qb, qe)
    return s[torch.isfinite(s)]


# ------------------------------------------------------------------------------------------- kernels against ref
@FORMATS
@HEADS
@pytest.mark.parametrize("case", CASES)
def test_gemma_cap_against_ref(case, Hq, Hkv, D, dtype):
    """cap = 50 on N(0, 1) scores: forward, dQ, dK, dV of every mask kind and the query range."""
    q, k, v, do = operands(case, Hq, Hkv, D, dtype)
    against_ref(q, k, v, do, Hq, Hkv, D, case, 50.0, f"cap50 {case} {dtype} D={D}")


@FORMATS
@HEADS
@pytest.mark.parametrize("case", ["causal", "w65", "doc"])
def test_saturating_cap_against_ref(case, Hq, Hkv, D, dtype):
    """cap = 2 with q times 4: x ~ N(0, 4^2), about 60 % of the visible scores lie past the cap."""
    q, k, v, do = operands(case, Hq, Hkv, D, dtype, qmul=4)
    x = visible_scores(q, k, Hq, Hkv, D, case)
    share = float((x.abs() > 2.0).float().mean())
    print(f"share of visible scores with |x| > cap: {share:.3f}")
    assert share >= 0.25, share
    _, lse, _, _ = against_ref(q, k, v, do, Hq, Hkv, D, case, 2.0, f"cap2 {case} {dtype} D={D}")
    # the cap did its work: the uncapped lse of these scores is far away
    _, plain = ref.attn_fwd(q, k, v, B, T, Hq, Hkv, 1.0 / math.sqrt(D), True, 0.0, seed_obj(), SITE, **mask_kw(case))
    assert float((plain - lse).abs().max()) > 1.0


@FORMATS
@HEADS
@pytest.mark.parametrize("planted", [False, True], ids=["random", "all_saturated"])
@pytest.mark.parametrize("case", ["causal", "w65", "doc"])
def test_overflowing_tanh_argument(case, planted, Hq, Hkv, D, dtype):
    """cap = 2 with q times 64: x / cap runs into the hundreds, the exp2 of the tanh evaluation overflows to inf for
    large positive scores and underflows to 0 for large negative ones.  Every output is finite and within the
    tolerances of the reference.  ``all_saturated`` plants one dominant column (``inputs``) so that EVERY visible
    score is past +-100 cap: there the forward must equal the softmax over scores that are exactly +-cap."""
    q, k, v, do = operands(case, Hq, Hkv, D, dtype, qmul=64, planted=planted)
    x = visible_scores(q, k, Hq, Hkv, D, case)
    # 2 log2(e) x / cap beyond +-128 (|x| > 88.8) is where exp2 leaves fp32: a good share on both sides
    assert float((x > 89.0).float().mean()) > 0.05 and float((x < -89.0).float().mean()) > 0.05
    what = f"overflow {case} {dtype} D={D} planted={planted}"
    o, lse, ro, rlse = against_ref(q, k, v, do, Hq, Hkv, D, case, 2.0, what)
    if not planted:
        return
    assert float(x.abs().min()) > 100.0 * 2.0, float(x.abs().min())
    kw = dict(mask_kw(case))
    qb, qe = kw.pop("q_range", (0, T))
    s = ref._attn_probs(q, k, B, T, Hq, Hkv, D, 1.0 / math.sqrt(D), True, kw.get("window", 0), kw.get("bounds"), qb, qe)
    z = torch.where(torch.isfinite(s), 2.0 * torch.sign(s), s)          # all +-cap, the masked ones stay -inf
    zl = torch.logsumexp(z, -1)
    G = Hq // Hkv
    vh = v.float().view(B, T, Hkv, D).transpose(1, 2).repeat_interleave(G, 1)
    zo = (torch.exp(z - zl[..., None]) @ vh).transpose(1, 2).reshape(B * T, Hq * D)
    close(lse, zl, 8e-3, 1e-3, f"{what} lse against +-cap")
    close(o, zo, 2e-2, 3e-2, f"{what} O against +-cap")


# ------------------------------------------------------------------------------------------- off is off
@FORMATS
@HEADS
@pytest.mark.parametrize("case", ["causal", "w65"])
def test_softcap_zero_is_the_plain_call_bit_for_bit(case, Hq, Hkv, D, dtype):
    q, k, v, do = operands(case, Hq, Hkv, D, dtype)
    plain = run_kernels(q, k, v, do, Hq, Hkv, D, case)
    zero = run_kernels(q, k, v, do, Hq, Hkv, D, case, softcap=0.0)
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), plain, zero):
        assert torch.isfinite(a).all(), name
        assert same_bits(a, b), name


def _count_cap_launches(monkeypatch):
    """Wraps the extension's attention entry points; returns the list that collects every call's softcap."""
    C = ext()
    seen = []

    def wrap(name, pos):
        fn = getattr(C, name)

        def inner(*a, **kw):
            seen.append((name, kw.get("softcap", a[pos] if len(a) > pos else 0.0)))
            return fn(*a, **kw)
        monkeypatch.setattr(C, name, inner)
    wrap("attn_fwd", 16)            # positional index of softcap in the bindings' signatures
    wrap("attn_bwd_part", 21)
    return seen


def test_bindings_refuse_bad_operands():
    C = ext()
    Hq, Hkv, D = 2, 2, 64
    q, k, v, do = inputs(Hq, Hkv, D, BF16)
    scale = 1.0 / math.sqrt(D)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="softcap must be"):
            C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, softcap=bad)
    with pytest.raises(RuntimeError, match="causal"):
        C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, False, 0.0, softcap=50.0)
    mask = C.attn_mask(B, T, Hq, 0.1, seed_obj().device_tensor, SITE, q)
    with pytest.raises(RuntimeError, match="p = 0"):
        C.attn_fwd(q, k, v, mask, B, T, Hq, Hkv, scale, True, 0.1, softcap=50.0)
    with pytest.raises(RuntimeError, match="sink"):
        C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, sink=torch.zeros(Hq, device=DEV, dtype=BF16),
                   softcap=50.0)
    lse = torch.zeros(B, Hq, T, device=DEV)
    with pytest.raises(RuntimeError, match="causal"):
        C.attn_bwd_part(1, q, k, v, do, lse, lse.clone(), None, torch.empty_like(q), None, B, T, Hq, Hkv, scale, False,
                        0.0, softcap=50.0)
    with pytest.raises(ValueError, match="causal"):
        F_.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, False, 0.0, seed_obj(), SITE, softcap=50.0)
    with pytest.raises(ValueError, match="sink"):
        F_.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.0, seed_obj(), SITE,
                    sink=torch.zeros(Hq, device=DEV, dtype=BF16), softcap=50.0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- whole model
T_MODEL = 128


def _cfg(cap, **kw):
    return ModelConfig(**dict(get_model_config("mtiny", T_MODEL).to_dict(), attn_softcap=cap, **kw))


def _scaled_up(cfg, mul=6.0):
    """One initialisation with the query and key projections times ``mul``: at the initialisation's scale the scores
    are far below either cap, and a cap that bends nothing would check nothing."""
    torch.manual_seed(0)
    m = build_model(cfg)
    qk_rows = (cfg.n_head + cfg.kv_heads) * cfg.head_dim
    with torch.no_grad():
        for layer in m.model.layers:
            layer.self_attn.qkv_proj.weight[:qk_rows].mul_(mul)
    return m


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


def _one_step(base, kind, idx, tgt, head_chunk=None):
    m = copy.deepcopy(base) if kind == "cpu" else copy.deepcopy(base).to(DEV, BF16)
    m.rt = ParamRuntime()
    if kind != "cpu":
        m.activation_recompute = kind
    if head_chunk:
        m.head_chunk = head_chunk
    i, t = (idx, tgt) if kind == "cpu" else (idx.to(DEV), tgt.to(DEV))
    loss = m(i, t)[1]
    loss.backward()
    return loss.detach(), {n: p.grad for n, p in m.named_parameters()}


def _batch(cfg):
    idx = torch.randint(0, cfg.vocab_size, (2, T_MODEL), generator=torch.Generator().manual_seed(3))
    return idx, idx.roll(-1, 1)


def _model_close(cpu, gpu, what):
    (l_cpu, g_cpu), (l_gpu, g_gpu) = cpu, gpu
    print(f"{what}: loss cpu {l_cpu.item():.6f} gpu {l_gpu.item():.6f}")
    assert math.isfinite(l_gpu.item())
    assert abs(l_cpu.item() - l_gpu.item()) < 1e-2 * abs(l_cpu.item())
    for n, g in g_cpu.items():
        if g is None:           # an expert without a token on the CPU path
            continue
        assert torch.isfinite(g_gpu[n]).all(), n
        r = rel(g_gpu[n], g)
        assert r < 6e-2, (what, n, r)


@pytest.fixture(scope="module", params=[50.0, 2.0], ids=["cap50", "cap2"])
def model_runs(request):
    """One initialisation per cap; the CPU reference run and the GPU runs per recompute mode, each computed once."""
    cfg = _cfg(request.param)
    base = _scaled_up(cfg)
    idx, tgt = _batch(cfg)
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = _one_step(base, kind, idx, tgt)
        return cache[kind]
    get.cap, get.base, get.batch = request.param, base, (idx, tgt)
    return get


def test_model_matches_cpu_reference(model_runs):
    """Loss and every parameter gradient against the CPU reference path (ops/ref.py with the cap), at the tolerances of
    tests/test_attn_sinks_gpu.py; the CPU path without the cap gives another loss, so the cap is in the comparison."""
    _model_close(model_runs("cpu"), model_runs("off"), f"cap {model_runs.cap}")
    off = copy.deepcopy(model_runs.base)
    off.cfg.attn_softcap = 0.0
    l_off, _ = _one_step(off, "cpu", *model_runs.batch)
    assert abs(l_off.item() - model_runs("cpu")[0].item()) > (1e-5 if model_runs.cap == 50.0 else 1e-3)


@pytest.mark.parametrize("mode", ["selective", "full"])
def test_model_recompute_equals_off_bit_for_bit(model_runs, mode):
    l0, g0 = model_runs("off")
    l1, g1 = model_runs(mode)
    assert torch.equal(l0, l1), (l0.item(), l1.item())
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_flag_off_model_launches_no_cap_kernel(monkeypatch):
    seen = _count_cap_launches(monkeypatch)
    cfg = _cfg(0.0)
    idx, tgt = _batch(cfg)
    _one_step(_scaled_up(cfg), "off", idx, tgt)
    assert len(seen) == 3 * cfg.n_layer and all(c == 0.0 for _, c in seen), seen
    del seen[:]
    cfg = _cfg(50.0)
    _one_step(_scaled_up(cfg), "off", idx, tgt)
    assert len(seen) == 3 * cfg.n_layer and all(c == 50.0 for _, c in seen), seen


def _pick_routers(model, cfg, idx):
    """The procedure of tests/test_moe_gpu.py::_margin_case on this model: a top-k choice is discontinuous, and a bf16
    run compares with an fp32 run only while no token's choice flips.  Layer by layer, among 20000 draws of the init
    scheme's std 0.02, take the router whose smallest gap between the K-th and (K+1)-th logit over the rows (float64
    run) is largest.  Returns the smallest gap."""
    gen = torch.Generator().manual_seed(9)
    m64 = copy.deepcopy(model).double()
    seen = []
    real = ref.moe_route

    def spy(h, wr, K):
        seen.append(h.detach().clone())
        return real(h, wr, K)
    gaps = []
    for layer in range(cfg.n_layer):
        seen.clear()
        ref.moe_route = spy
        try:
            m64(idx, idx)
        finally:
            ref.moe_route = real
        cands = (0.02 * torch.randn(20000, cfg.n_experts, cfg.n_embd, generator=gen)).double()
        srt = torch.sort(torch.einsum("nd,ced->cne", seen[layer], cands), -1, descending=True).values
        K = cfg.moe_top_k
        gap, best = (srt[..., K - 1] - srt[..., K]).min(1).values.max(0)
        gaps.append(float(gap))
        with torch.no_grad():
            m64.model.layers[layer].mlp.router.weight.copy_(cands[best])
            model.model.layers[layer].mlp.router.weight.copy_(cands[best])
    return min(gaps)


@pytest.mark.parametrize("kw,chunk", [(dict(qk_norm=True), None),
                                      (dict(n_experts=4, moe_top_k=2, moe_dropless=True), None),
                                      (dict(), 64)], ids=["qknorm", "moe_dropless", "head_chunk64"])
def test_composition_one_step(kw, chunk):
    """One mtiny step under cap 2 with --qk-norm, --moe-experts 4 --moe-dropless, --head-chunk 64: finite, and the CPU
    path's loss and gradients within the model tolerances.  The MoE case runs 128 rows with routers chosen for a
    margin (``_pick_routers``) and first checks that the device chose the CPU run's experts token by token: with the
    init's routers one flipped choice put post_attention_layernorm's gradient at 6.1e-2 of the 6e-2 allowed."""
    cfg = _cfg(2.0, **kw)
    base = _scaled_up(cfg, 1.0 if kw.get("qk_norm") else 6.0)      # QK-norm sets the scores' scale itself
    idx, tgt = _batch(cfg)
    if not cfg.n_experts:
        _model_close(_one_step(base, "cpu", idx, tgt, chunk), _one_step(base, "off", idx, tgt, chunk),
                     f"composition {kw} chunk={chunk}")
        return
    idx = idx[:1]
    tgt = idx.roll(-1, 1)
    gap = _pick_routers(base, cfg, idx)
    print(f"smallest gap between the K-th and (K+1)-th router logit {gap:.3e}")
    # tests/test_moe_gpu.py: the device's router logits differ from the float64 run's by at most LOGIT_DIFF = 5e-3
    # there, and a gap above twice the difference rules a flip out; the token-by-token check below is the guard
    assert gap >= 2 * 5.0e-3, gap
    seen = {"cpu": [], "cuda": []}
    real_f = F_.moe_route

    def spy(h, wr, K):
        out = real_f(h, wr, K)
        seen[h.device.type].append(out[0].cpu().sort(1).values)
        return out
    F_.moe_route = spy
    try:
        cpu, gpu = _one_step(base, "cpu", idx, tgt), _one_step(base, "off", idx, tgt)
    finally:
        F_.moe_route = real_f
    assert len(seen["cpu"]) == len(seen["cuda"]) == cfg.n_layer
    for layer, (c, g) in enumerate(zip(seen["cpu"], seen["cuda"])):
        assert torch.equal(c, g), f"routing flipped in layer {layer}"
    _model_close(cpu, gpu, f"composition {kw}")


def _train(graphed, accum=2, windows=2):
    torch.manual_seed(0)
    cfg = _cfg(2.0)
    with torch.device(DEV):
        model = build_model(cfg)
    eng = make_engine(model, engine_config("zero3", accum, "reference"), "cuda:0")
    eng.train()
    g = torch.Generator(device=DEV).manual_seed(1)
    runner = GraphedStep(eng) if graphed else None
    losses = []
    for _ in range(accum * windows):
        idx = torch.randint(0, cfg.vocab_size, (2, T_MODEL), device=DEV, generator=g)
        if runner is None:
            loss = eng(idx, idx.roll(-1, 1))[1]
            eng.backward(loss)
            eng.step()
        else:
            loss = runner(idx, idx.roll(-1, 1))
        losses.append(loss.item())
    if runner is not None:
        assert len(runner.graphs) == eng.accum and not runner.disabled
    sd = {k: v.detach().clone() for k, v in eng.full_state_dict().items()}
    del eng, model, runner
    torch.cuda.empty_cache()
    return losses, sd


def test_graph_replay_equals_eager():
    """Two accumulation windows of two micro-steps under ZeRO-3 and the cap: the replayed graphs train the eager steps'
    model bit for bit."""
    l0, s0 = _train(False)
    l1, s1 = _train(True)
    assert all(l == l for l in l0) and l0 == l1, (l0, l1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k


# ------------------------------------------------------------------------------------------- two ranks
TOL = dict(loss_tol=1e-3, upd_tol=0.02, cos_min=0.9998, param_tol=0.03)      # tests/test_attn_sinks_gpu.py


@pytest.mark.parametrize("case,layout", [("cp_zero3", "zigzag"), ("cp_zero3_window", "contiguous")])
def test_world2_cp2_zero3_equals_world1_gpu(tmp_path, case, layout):
    """Two ranks sharing the GPU (gloo, host-staged buffers) as one context-parallel group under ZeRO-3 against the
    one-rank whole-row run, mtiny under cap 2 at 512 positions: zigzag (two query ranges per rank), and contiguous
    with a sliding window."""
    args = ("--seq-len", "512", "--windows", "2", "--cases", case, "--attn-softcap", "2")
    ws1 = run(tmp_path / "ws1.pt", 1, "cuda", extra=args, timeout=300)
    ws2 = run(tmp_path / "ws2.pt", 2, "cuda", extra=args + ("--context-parallel", "2", "--cp-layout", layout),
              env_extra={"DLTB_COMM": "host"}, timeout=300)
    bad = compare(ws1, ws2, **TOL)
    assert not bad, bad
