"""The mixture-of-experts kernels of csrc/moe.hip on the MI355X: routing and slot assignment bit for bit against
ops/ref.py on inputs whose dot products are exact, every kernel against the float64 reference with bounds derived from
the number formats, determinism, and the routed model under HIP-graph replay, under every strategy, on two ranks and
under context parallelism.  (The hand-written backward against autograd: tests/test_moe_cpu.py, in float64.)"""
import copy
import json
import math
import os

import pytest
import torch

import dltb
from dltb.models import build_model, get_model_config
from dltb.models import mistral
from dltb.models.config import ModelConfig
from dltb.ops import functional as F_
from dltb.ops import ref
from dltb.parallel import GraphedStep, ParamRuntime, engine_config, make_engine
from multirank_util import compare, run

pytestmark = pytest.mark.gpu
DEV = "cuda"
U32 = 2.0 ** -24                     # fp32 unit roundoff
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
TOL = dict(loss_tol=1e-3, upd_tol=0.02, cos_min=0.9998, param_tol=0.03)      # tests/test_context_parallel_gpu.py


# ------------------------------------------------------------------------------------------- bounds
def half_ulp(v, dtype):
    """Half a unit in the last place of ``dtype`` at magnitude ``v`` (float64 tensor), subnormal spacing below."""
    p, emin = (8, -126) if dtype == torch.bfloat16 else (11, -14)
    e = torch.floor(torch.log2(v.clamp(min=2.0 ** emin)))
    return torch.pow(2.0, e - p)


def bound(want, mag, n, dtype):
    """|got - want| for got = one rounding to ``dtype`` of an fp32 value built by at most ``n`` fp32 operations on
    terms of summed magnitude ``mag``: any order of summation is within (n + 1) u32 mag of the exact value, and the
    final rounding adds half an ulp at the (error-widened) magnitude."""
    acc = (n + 1) * U32 * mag
    return acc + half_ulp(want.abs() + acc, dtype)


def check(got, want, mag, n, dtype, what):
    err = (got.double().cpu() - want).abs()
    b = bound(want, mag, n, dtype)
    worst = (err / b).max().item()
    print(f"{what}: max err / bound = {worst:.3f}")
    assert worst <= 1.0, (what, worst)


# ------------------------------------------------------------------------------------------- routing is exact
def _grid(shape, gen):
    """Integers in [-8, 8] times 2^-3: every product is a multiple of 2^-6 below 1 and every partial sum of 128 of
    them stays below 2^7, so a dot product is exact in fp32 in any order."""
    return torch.randint(-8, 9, shape, generator=gen).double() / 8.0


@pytest.fixture(scope="module")
def grid_inputs():
    gen = torch.Generator().manual_seed(11)
    out = {}
    for E in (8, 5):
        h, wr = _grid((200, 128), gen), _grid((E, 128), gen)
        wr[E - 2] = wr[1]           # two experts with the same row: a tie in every token row, wherever the pair ranks
        out[E] = (h, wr)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("E,K", [(8, 2), (8, 1), (8, 4), (5, 2), (5, 1), (5, 4)])
def test_routing_is_exact(grid_inputs, E, K, dtype):
    h64, wr64 = grid_inputs[E]
    N = 200
    C = ref.moe_capacity(N, E, K, 1.25)
    expert, gate, logits = ref.moe_route(h64, wr64, K)
    # the grid does produce ties at the selection boundary and rows without any
    srt = torch.sort(logits, -1, descending=True).values
    tie = srt[:, K - 1] == srt[:, K] if K < E else torch.zeros(N, dtype=torch.bool)
    inner = (srt[:, :K - 1] == srt[:, 1:K]).any(1) if K > 1 else torch.zeros(N, dtype=torch.bool)
    assert tie.any() and (~tie).any() and (K == 1 or inner.any())
    slot, src, src_k, counts = ref.moe_assign(expert, E, C)
    h, wr = h64.to(DEV, dtype), wr64.to(DEV, dtype)
    assert torch.equal(h.double().cpu(), h64) and torch.equal(wr.double().cpu(), wr64)
    g_expert, g_gate, g_logits = F_.moe_route(h, wr, K)
    g_slot, g_src, g_src_k, g_counts = F_.moe_assign(g_expert, E, C)
    torch.cuda.synchronize()
    assert torch.equal(g_logits.double().cpu(), logits)
    assert torch.equal(g_expert.cpu(), expert)
    assert torch.equal(g_slot.cpu(), slot) and torch.equal(g_src.cpu(), src)
    assert torch.equal(g_src_k.cpu(), src_k) and torch.equal(g_counts.cpu(), counts)
    assert int(counts.sum()) == N * K
    # gates: K exp() results, K - 1 adds and a divide in fp32
    rel = ((g_gate.double().cpu() - gate) / gate).abs().max().item()
    print(f"gate max rel err {rel:.3e}")
    assert rel <= 8 * U32


@pytest.mark.parametrize("N,K,E", [(1, 1, 2), (63, 1, 64), (64, 4, 64), (65, 2, 3), (1030, 4, 7), (4100, 2, 64)])
def test_assign_sizes(N, K, E):
    """Slot assignment alone over the sizes at which its kernels change shape: less than one wave of assignments,
    exactly one, one more, several blocks, more waves than the scan's 16 segments; 64 experts."""
    gen = torch.Generator().manual_seed(N)
    expert = torch.stack([torch.randperm(E, generator=gen)[:K] for _ in range(N)]).to(torch.int32)
    expert[: N // 2, 0] = 0
    if K > 1:
        expert[: N // 2, 1:] = torch.stack([1 + torch.randperm(E - 1, generator=gen)[:K - 1]
                                            for _ in range(N // 2)]).to(torch.int32)
    C = ref.moe_capacity(N, E, K, 1.0)
    want = ref.moe_assign(expert, E, C)
    got = F_.moe_assign(expert.to(DEV), E, C)
    for w, g, name in zip(want, got, ("slot", "src", "src_k", "counts")):
        assert torch.equal(g.cpu(), w), name


# ------------------------------------------------------------------------------------------- capacity edges
def _layer_model(E, K, factor, dtype, d=128, f=256):
    cfg = ModelConfig(arch="mistral", vocab_size=64, n_embd=d, n_head=2, n_kv_head=1, n_layer=1, ffn_hidden=f,
                      block_size=256, dropout=0.0, causal=True, tie_embeddings=False, n_experts=E, moe_top_k=K,
                      moe_capacity_factor=factor)
    torch.manual_seed(2)
    model = mistral.MistralLM(cfg).to(DEV, dtype)
    model.rt = ParamRuntime()
    return cfg, model


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_capacity_edge_everything_to_expert_0(dtype):
    E, K, N, d = 8, 1, 200, 128
    cfg, model = _layer_model(E, K, 1.25, dtype)
    C = ref.moe_capacity(N, E, K, 1.25)
    assert C == 32
    gen = torch.Generator().manual_seed(5)
    h = (torch.randint(1, 9, (N, d), generator=gen).double() / 8.0).to(DEV, dtype)       # positive rows
    unit = model.unit_blocks[0]
    ws = model.rt.acquire(unit)
    with torch.no_grad():
        for e in range(E):
            ws[4][e].fill_(1.0 - e / 8.0)              # logits strictly descending in e: expert 0 first, no tie
    m, saved = mistral._moe_fwd(model, 0, h, ws[4:])
    expert, gate, slot, src, xe, ye, gus, hhs, C_ = saved
    assert C_ == C and (expert == 0).all()
    assert src[:C].tolist() == list(range(C)) and (src[C:] == -1).all()            # exactly C kept, in token order
    assert slot[:C, 0].tolist() == list(range(C)) and (slot[C:] == -1).all()
    assert model.moe_counts(DEV)[0].tolist() == [N] + [0] * (E - 1)
    assert torch.equal(xe[:C], h[:C]) and (xe[C:] == 0).all()
    assert (m[C:] == 0).all() and (m[:C] != 0).any()
    s = [(torch.full_like(w, float("nan")), False) for w in ws]                    # accumulate = False on NaN slots
    dm = torch.randn(N, d, generator=gen).to(DEV, dtype)
    dh = mistral._moe_bwd(model, unit, dm, h, ws, s, saved)
    torch.cuda.synchronize()
    assert torch.isfinite(dh).all()
    for j in (5, 6):
        assert torch.isfinite(s[j][0]).all() and (s[j][0] != 0).any(), j          # expert 0 has a gradient
    for e in range(1, E):
        for j in (5 + 2 * e, 6 + 2 * e):
            assert (s[j][0] == 0).all(), (e, j)                                    # exact zeros, not stale memory
    assert torch.isfinite(s[4][0]).all()
    assert (s[4][0] == 0).all()        # K = 1: the only gate is 1 whatever the logits, so the router gets no gradient


# ------------------------------------------------------------------------------------------- kernels against float64
@pytest.fixture(scope="module")
def kcase():
    """N = 200, d = 128, E = 8, K = 2, C = 64 with drops; random data, read-only."""
    gen = torch.Generator().manual_seed(21)
    N, d, E, K = 200, 128, 8, 2
    h = torch.randn(N, d, generator=gen) + 0.5
    wr = 0.3 * torch.randn(E, d, generator=gen)
    wr[0] += 0.15                                       # rows of mean 0.5: expert 0 is crowded and overflows
    C = ref.moe_capacity(N, E, K, 1.0)
    return dict(N=N, d=d, E=E, K=K, C=C, h=h, wr=wr, ye=torch.randn(E * C, d, generator=gen),
                dm=torch.randn(N, d, generator=gen), dxe=torch.randn(E * C, d, generator=gen),
                dxe_grid=_grid((E * C, d), gen))


def _routed(kcase, dtype):
    h, wr = kcase["h"].to(DEV, dtype), kcase["wr"].to(DEV, dtype)
    expert, gate, _ = F_.moe_route(h, wr, kcase["K"])
    slot, src, src_k, counts = F_.moe_assign(expert, kcase["E"], kcase["C"])
    assert (slot < 0).any() and (src < 0).any() and int(counts.max()) > kcase["C"]
    return h, wr, expert, gate, slot, src


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_kernels_against_float64(kcase, dtype):
    N, d, E, K, C = (kcase[k] for k in ("N", "d", "E", "K", "C"))
    h, wr, expert, gate, slot, src = _routed(kcase, dtype)
    c = lambda t: t.cpu()
    f64 = lambda t: t.double().cpu()
    # dispatch: exact copies, exact zero rows
    xe = F_.moe_dispatch(h, src)
    assert torch.equal(c(xe), ref.moe_dispatch(c(h), c(src)))
    assert (xe[src < 0] == 0).all()
    # combine: K fused multiply-adds in fp32, one rounding
    ye = kcase["ye"].to(DEV, dtype)
    m = F_.moe_combine(ye, slot, gate)
    want = ref.moe_combine(f64(ye), c(slot), f64(gate))
    mag = ref.moe_combine(f64(ye).abs(), c(slot), f64(gate))
    check(m, want, mag, K, dtype, "combine")
    assert (m[(slot < 0).all(1)] == 0).all()
    # combine backward
    dm = kcase["dm"].to(DEV, dtype)
    dye, dgate, dlogits = F_.moe_combine_bwd(dm, ye, slot, src, expert, gate, E)
    w_dye, w_dgate, _ = ref.moe_combine_bwd(f64(dm), f64(ye), c(slot), c(src), c(expert), f64(gate), E)
    check(dye, w_dye, w_dye.abs(), 1, dtype, "dye")                     # one fp32 product, one rounding
    assert (dye[src < 0] == 0).all()
    # dgate: an fp32 dot product of d terms (any order), kept in fp32
    mag_g = ref.moe_combine_bwd(f64(dm).abs(), f64(ye).abs(), c(slot), c(src), c(expert), f64(gate), E)[1]
    err = (f64(dgate) - w_dgate).abs()
    assert (err <= (d + 1) * U32 * mag_g).all(), (err / ((d + 1) * U32 * mag_g).clamp(min=1e-300)).max()
    assert (dgate[slot < 0] == 0).all()
    # dlogits: the softmax backward of the kernel's own dgate: K products and adds, one product more, in fp32
    g64, dg64 = f64(gate), f64(dgate)
    t = (g64 * dg64).sum(-1, keepdim=True)
    w_dl = torch.zeros(N, E, dtype=torch.float64).scatter_(1, c(expert).long(), g64 * (dg64 - t))
    mag_l = torch.zeros(N, E, dtype=torch.float64).scatter_(1, c(expert).long(),
                                                            g64 * (dg64.abs() + (g64 * dg64.abs()).sum(-1, keepdim=True)))
    assert ((f64(dlogits) - w_dl).abs() <= (2 * K + 3) * U32 * mag_l).all()
    chosen = torch.zeros(N, E, dtype=torch.bool).scatter_(1, c(expert).long(), True)
    assert (c(dlogits)[~chosen] == 0).all()
    # dispatch backward, gather part alone (zero router gradient): sums of grid values are exact
    dxe_g = kcase["dxe_grid"].to(DEV, dtype)
    zero_l = torch.zeros(N, E, device=DEV)
    dh_g = F_.moe_dispatch_bwd(dxe_g, slot, zero_l, wr)
    assert torch.equal(f64(dh_g), ref.moe_dispatch_bwd(kcase["dxe_grid"], c(slot), torch.zeros(N, E).double(), f64(wr)))
    # ... and whole: K adds and at most E fused multiply-adds in fp32, one rounding
    dxe = kcase["dxe"].to(DEV, dtype)
    dh = F_.moe_dispatch_bwd(dxe, slot, dlogits, wr)
    want = ref.moe_dispatch_bwd(f64(dxe), c(slot), f64(dlogits), f64(wr))
    mag = ref.moe_dispatch_bwd(f64(dxe).abs(), c(slot), f64(dlogits).abs(), f64(wr).abs())
    check(dh, want, mag, K + E, dtype, "dispatch_bwd")
    # router weight gradient: a sum over N rows in a fixed but unspecified order, into NaN (overwrite), then accumulated
    dwr = torch.full_like(wr, float("nan"))
    F_.moe_router_wgrad(dlogits, h, dwr, False)
    want = f64(dlogits).t() @ f64(h)
    mag = f64(dlogits).abs().t() @ f64(h).abs()
    check(dwr, want, mag, N, dtype, "router_wgrad")
    first = dwr.clone()
    F_.moe_router_wgrad(dlogits, h, dwr, True)
    check(dwr, want + f64(first), mag + f64(first).abs(), N + 1, dtype, "router_wgrad accumulate")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_kernels_are_deterministic(kcase, dtype):
    def once():
        h, wr, expert, gate, slot, src = _routed(kcase, dtype)
        E = kcase["E"]
        ye, dm, dxe = (kcase[k].to(DEV, dtype) for k in ("ye", "dm", "dxe"))
        xe = F_.moe_dispatch(h, src)
        m = F_.moe_combine(ye, slot, gate)
        dye, dgate, dlogits = F_.moe_combine_bwd(dm, ye, slot, src, expert, gate, E)
        dh = F_.moe_dispatch_bwd(dxe, slot, dlogits, wr)
        dwr = torch.empty_like(wr)
        F_.moe_router_wgrad(dlogits, h, dwr, False)
        return [t.cpu() for t in (expert, gate, slot, src, xe, m, dye, dgate, dlogits, dh, dwr)]

    a, b = once(), once()
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), i


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,E", [(64, 64), (128, 32), (576, 16), (1088, 64)])
def test_dispatch_bwd_more_experts_than_chunk_lanes(d, E, dtype):
    """The router term of dh with every dlogit non-zero, at widths where fewer lanes hold a 16-byte chunk than there
    are experts (d / 8 < E), and at widths that are no multiple of 512, below and above it (the last pass over the
    chunks then runs with part of the wave)."""
    gen = torch.Generator().manual_seed(d + E)
    N, K, C = 37, 2, 16
    rows = E * C
    dxe = torch.randn(rows, d, generator=gen).to(dtype)
    wr = torch.randn(E, d, generator=gen).to(dtype)
    dlogits = torch.randn(N, E, generator=gen)
    slot = torch.randint(-1, rows, (N, K), generator=gen).to(torch.int32)
    got = F_.moe_dispatch_bwd(dxe.to(DEV), slot.to(DEV), dlogits.to(DEV), wr.to(DEV))
    want = ref.moe_dispatch_bwd(dxe.double(), slot, dlogits.double(), wr.double())
    mag = ref.moe_dispatch_bwd(dxe.double().abs(), slot, dlogits.double().abs(), wr.double().abs())
    check(got, want, mag, K + E, dtype, f"dispatch_bwd d={d} E={E}")
    only = ref.moe_dispatch_bwd(dxe.double(), slot, torch.zeros(N, E).double(), wr.double())
    assert float((want - only).abs().min(0).values.max()) > 0           # the router term reaches every column


# ------------------------------------------------------------------------------------------- one layer against float64
def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("E,K", [(8, 2), (32, 4)])
def test_layer_forward_backward_against_float64(E, K, dtype):
    """``_moe_fwd`` / ``_moe_bwd`` as the GPU runs them (the seven kernels, the E slab GEMMs, the gradient slots
    4, 5 + 2e, 6 + 2e) against the same functions on the float64 CPU path.  The rows and the router lie on a dyadic
    grid, so the logits are exact on both sides and the routing is equal by construction (asserted): any difference
    is arithmetic.  N = 200, d = 128, f = 256, capacity factor 1.0 (drops); E = 32 > d / 8.  Tolerance: the relative
    L2 bound of tests/test_mistral_gpu.py."""
    N, d = 200, 128
    cfg, model = _layer_model(E, K, 1.0, dtype)
    gen = torch.Generator().manual_seed(31 + E)
    h64 = _grid((N, d), gen)
    wr64 = _grid((E, d), gen) / 16.0                    # logits of spread 0.3, still exact: multiples of 2^-10 below 8
    wr64[E - 2] = wr64[1]                               # ties in every row
    h64[:, 0] = 1.0                                     # ... and two crowded experts, so that late tokens lose both
    wr64[0, 0] += 1.0
    wr64[2, 0] += 0.75
    dm64 = torch.randn(N, d, generator=gen).to(dtype).double()
    with torch.no_grad():
        model.model.layers[0].mlp.router.weight.copy_(wr64)
        for ex in model.model.layers[0].mlp.experts:   # larger experts: outputs and gradients of order 1
            ex.gate_up_proj.weight.mul_(8.0)
            ex.down_proj.weight.mul_(8.0)
    m64 = copy.deepcopy(model).cpu().double()
    m64.rt = ParamRuntime()
    assert torch.equal(m64.model.layers[0].mlp.router.weight, wr64)

    def run_layer(mod, h, dm):
        unit = mod.unit_blocks[0]
        ws = mod.rt.acquire(unit)
        m, saved = mistral._moe_fwd(mod, 0, h, ws[4:])
        s = [(torch.full_like(w, float("nan")), False) for w in ws]
        dh = mistral._moe_bwd(mod, unit, dm, h, ws, s, saved)
        return m, dh, [t for t, _ in s[4:]], saved

    m_g, dh_g, grads_g, saved_g = run_layer(model, h64.to(DEV, dtype), dm64.to(DEV, dtype))
    m_c, dh_c, grads_c, saved_c = run_layer(m64, h64, dm64)
    for i in (0, 2, 3):                                 # expert, slot, src: the routing taken from the device
        assert torch.equal(saved_g[i].cpu(), saved_c[i]), i
    assert (saved_c[2] < 0).any()                                        # drops
    assert K > 2 or (saved_c[2] < 0).all(1).any()                        # K = 2: a token that lost every choice
    assert rel(m_g, m_c) < 6e-2 and rel(dh_g, dh_c) < 6e-2, (rel(m_g, m_c), rel(dh_g, dh_c))
    names = ["router"] + [f"experts.{e}.{w}" for e in range(E) for w in ("gate_up", "down")]
    worst = 0.0
    for n, a, b in zip(names, grads_g, grads_c):
        assert float(b.abs().max()) > 0 or float(a.float().abs().max()) == 0, n
        r = rel(a, b)
        worst = max(worst, r)
        assert r < 6e-2, (n, r)
    print(f"E={E} K={K}: m {rel(m_g, m_c):.2e} dh {rel(dh_g, dh_c):.2e} worst gradient {worst:.2e}")


# ------------------------------------------------------------------------------------------- model level
# The largest |GPU router logit - float64 router logit| over both layers of the case below (bf16, MI355X) measured
# 4.1e-3 on 2026-10-20; the test prints the current value and fails above LOGIT_DIFF.  The logits have a spread of 0.2.
# The best of 20000 router draws per layer gives a smallest 2nd-to-3rd logit gap of 1.3e-2: 3.2 times the measured
# difference, not the 8 times first aimed at (3.3e-2), which no draw of the init scheme reaches at 128 rows (gap and
# difference both scale with the router's std).  A choice flips only if two logits move towards each other by the gap,
# so a gap above twice the difference already rules a flip out; the test asks for 2.5 times LOGIT_DIFF, and then
# checks the device's chosen experts against the float64 run's token by token, failing on any flip, before it
# compares anything else.
LOGIT_DIFF = 5.0e-3
GAP_FACTOR = 2.5


def _margin_case():
    """mtiny, E = 4, K = 2, 128 token rows as T = 128, B = 1 (the GPU attention kernels need T % 128 == 0, so the
    rows of T = 64, B = 2 are laid out as one sequence).  Routers are chosen on the CPU, layer by layer, among random
    draws of the init scheme's std 0.02: the draw whose smallest gap between the K-th and (K+1)-th logit over the
    layer's 128 rows (float64 reference run) is largest."""
    cfg = get_model_config("mtiny", 128)
    cfg.n_experts, cfg.moe_top_k, cfg.moe_capacity_factor = 4, 2, 1.0
    cfg.validate()
    torch.manual_seed(0)
    model = build_model(cfg)
    gen = torch.Generator().manual_seed(9)
    idx = torch.randint(0, cfg.vocab_size, (1, 128), generator=gen)
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
        h2 = seen[layer]
        cands = (0.02 * torch.randn(20000, 4, cfg.n_embd, generator=gen)).double()
        srt = torch.sort(torch.einsum("nd,ced->cne", h2, cands), -1, descending=True).values
        gap, best = (srt[..., 1] - srt[..., 2]).min(1).values.max(0)
        gaps.append(float(gap))
        with torch.no_grad():
            m64.model.layers[layer].mlp.router.weight.copy_(cands[best])
            model.model.layers[layer].mlp.router.weight.copy_(cands[best])
    return cfg, model, m64, idx, min(gaps)


def test_model_against_cpu_reference():
    cfg, m_cpu, m64, idx, gap = _margin_case()
    print(f"smallest gap between the 2nd and 3rd logit {gap:.3e}, required {GAP_FACTOR * LOGIT_DIFF:.3e}")
    assert gap >= GAP_FACTOR * LOGIT_DIFF, gap         # a changed init fails here, not in the comparison below
    m_gpu = copy.deepcopy(m_cpu).to(DEV, torch.bfloat16)
    m_cpu.rt, m_gpu.rt = ParamRuntime(), ParamRuntime()
    seen = {"cpu": [], "cuda": []}
    real_f = F_.moe_route

    def spy(h, wr, K):
        out = real_f(h, wr, K)
        seen[h.device.type].append((out[0].cpu(), out[2].detach().double().cpu()))
        return out

    tgt = idx.roll(-1, 1)
    F_.moe_route = spy
    try:
        m64(idx, tgt)
        want = list(seen["cpu"])
        seen["cpu"].clear()
        _, l_cpu = m_cpu(idx, tgt)
        _, l_gpu = m_gpu(idx.to(DEV), tgt.to(DEV))
    finally:
        F_.moe_route = real_f
    assert len(want) == len(seen["cuda"]) == len(seen["cpu"]) == cfg.n_layer
    diff = max(float((g[1] - w[1]).abs().max()) for g, w in zip(seen["cuda"], want))
    print(f"largest GPU-vs-float64 router logit difference {diff:.3e}")
    assert diff <= LOGIT_DIFF, diff
    # the chosen SET per token must be the float64 run's (the margin is between the K-th and (K+1)-th logit; the two
    # chosen logits may swap places: a token's slot in an expert does not depend on the choice's position k)
    for layer, (g, c, w) in enumerate(zip(seen["cuda"], seen["cpu"], want)):
        chosen = [t[0].sort(1).values for t in (g, c, w)]
        assert torch.equal(chosen[0], chosen[2]) and torch.equal(chosen[1], chosen[2]), f"routing flipped in layer {layer}"
    assert abs(l_cpu.item() - l_gpu.item()) < 1e-2 * abs(l_cpu.item())
    l_cpu.backward()
    l_gpu.backward()
    gp = dict(m_gpu.named_parameters())
    for n, p in m_cpu.named_parameters():
        r = rel(gp[n].grad, p.grad)
        assert r < 6e-2, (n, r)
    assert torch.equal(m_gpu.moe_counts(DEV).cpu(), m_cpu.moe_counts("cpu"))


# ------------------------------------------------------------------------------------------- graphs and strategies
def _train(strategy, graphed, dtype=None, steps=6, accum=2, T=128, same_batch=False):
    torch.manual_seed(0)
    cfg = get_model_config("mtiny", T)
    cfg.n_experts = 4
    cfg.validate()
    with torch.device(DEV):
        model = build_model(cfg)
    kw = {} if dtype is None else {"compute_dtype": dtype}
    eng = make_engine(model, engine_config(strategy, accum, "reference", **kw), "cuda:0")
    eng.train()
    g = torch.Generator(device=DEV).manual_seed(1)
    runner = GraphedStep(eng) if graphed else None
    losses, counts = [], []
    idx = None
    for _ in range(steps):
        if idx is None or not same_batch:
            idx = torch.randint(0, cfg.vocab_size, (2, T), device=DEV, generator=g)  # a new batch: routing changes
        if runner is None:
            loss = eng(idx, idx)[1]
            eng.backward(loss)
            eng.step()
        else:
            loss = runner(idx, idx)
        losses.append(loss.item())
        counts.append(model.moe_counts(DEV).cpu().clone())
    if runner is not None:
        assert len(runner.graphs) == eng.accum and not runner.disabled
    return losses, eng.full_state_dict(), counts


def test_graph_replay_is_eager_bit_for_bit():
    l0, s0, c0 = _train("zero3", False)
    l1, s1, c1 = _train("zero3", True)          # one eager window, then three windows' worth of replays
    assert l0 == l1, (l0, l1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    for a, b in zip(c0, c1):
        assert torch.equal(a, b)
    assert not all(torch.equal(c0[0], c) for c in c0[1:])      # the routing did change between the batches


def test_strategies_train_the_same_model():
    """zero2 and zero3 at world 1 hold the same bf16 model and run the same kernels in the same order: bitwise equal
    losses and parameters after two windows.  ddp and fsdp scale the loss and the update differently (the
    reference's semantics per strategy), and no test of the dense model compares them with the ZeRO engines; they
    are held to what tests/test_mistral_gpu.py asks of an engine: finite losses that fall on a repeated batch."""
    l2, s2, _ = _train("zero2", False, steps=4)
    l3, s3, _ = _train("zero3", False, steps=4)
    assert all(math.isfinite(v) for v in l2) and l2 == l3, (l2, l3)
    for k in s2:
        assert torch.equal(s2[k], s3[k]), k
    moe = [k for k in s2 if ".mlp.experts." in k or ".mlp.router." in k]
    assert len(moe) == 18
    for strategy in ("ddp", "fsdp", "zero3"):
        l, s, _ = _train(strategy, False, steps=6, same_batch=True)
        assert all(math.isfinite(v) for v in l), (strategy, l)
        assert l[-1] < l[0], (strategy, l)
        assert all(torch.isfinite(s[k].float()).all() for k in moe), strategy


def test_fp16_build_trains():
    l, s, _ = _train("ddp", False, dtype=torch.float16, steps=4)
    assert all(math.isfinite(v) for v in l), l
    assert all(torch.isfinite(t.float()).all() for t in s.values())


def test_world2_host_staged_zero3_lazy(tmp_path):
    args = ("--seq-len", "128", "--windows", "2", "--cases", "zero3_mistral", "--moe-experts", "4",
            "--moe-capacity-factor", "2.0")
    one = run(tmp_path / "w1.pt", 1, "cuda", extra=args)
    two = run(tmp_path / "w2.pt", 2, "cuda", extra=args, env_extra={"DLTB_COMM": "host", "DLTB_COMM_LAZY": "1"})
    # F = E / K: nothing drops, so the split of the rows over the ranks cannot change which assignments are kept
    bad = compare(one, two, **TOL)
    assert not bad, bad


def test_context_parallel_doc_mask_head_chunk_together(tmp_path):
    args = ("--seq-len", "512", "--windows", "2", "--cases", "cp_zero3", "--moe-experts", "4",
            "--moe-capacity-factor", "2.0", "--doc-len", "16", "--head-chunk", "32")
    one = run(tmp_path / "cp1.pt", 1, "cuda", extra=args)
    two = run(tmp_path / "cp2.pt", 2, "cuda", extra=args + ("--context-parallel", "2"),
              env_extra={"DLTB_COMM": "host"})
    bad = compare(one, two, **TOL)
    assert not bad, bad


def test_strict_kernels_stays_clean(tmp_path):
    from dltb.harness import main
    os.environ.pop("WORLD_SIZE", None)
    res = tmp_path / "res"
    assert main(["--strategy", "zero3", "--tier", "M7B_narrow", "--seq-len", "128", "--steps", "2", "--warmup-steps",
                 "1", "--per-device-batch", "1", "--grad-accum", "1", "--results-dir", str(res), "--log-every", "0",
                 "--moe-experts", "8", "--strict-kernels"]) == 0
    ext = [f for f in os.listdir(res) if f.endswith(".extended.json")]
    side = json.loads((res / ext[0]).read_text())
    assert side["torch_gemm_fallbacks"] is None and side["strict_kernels"] is True
    assert side["moe"]["experts"] == 8 and side["moe"]["capacity"] == 48
    assert all(sum(c) == 2 * 128 for c in side["moe"]["counts"]) and len(side["moe"]["counts"]) == 32
