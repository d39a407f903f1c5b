"""Learned attention sinks on the MI355X: the SINK forward instantiations of csrc/attention.hip and the sink-gradient
kernel of csrc/attn_sink.hip against dltb.ops.ref and float64, the exact equalities a very negative sink must give,
the whole model against the CPU reference path, recompute modes, HIP-graph replay, and ZeRO-3 with context
parallelism on two host-staged ranks.  The CPU definitions: tests/test_attn_sinks_cpu.py.

Shapes, comparison helper and tolerances of the attention quantities: tests/test_attention_window_gpu.py (those of
test_kernels_gpu.py::test_attention): lse 8e-3 / 1e-3, O 2e-2 / 3e-2, dq / dk / dv 5e-2 / 5e-2, no element outside.
B = 2, T = 512 is four query blocks and eight key tiles; (2, 2, 64) takes the three-way key-split merge in front of the
sink epilogue and (8, 2, 128) the head-split dK/dV path.

Bound of the sink-gradient kernel (``sink_bound``).  No tolerance is taken from what the kernel returns; the constants
are those of tests/test_qknorm_gpu.py: U = 2^-24 per fp32 rounding, MARGIN = 2 on the fp32 part, H = 2^-20 assumed for
one approximated function (here expf), ``half_ulp`` for the one rounding of a slot to 16 bits.  The kernel forms, for
head h and the (b, t) rows of workgroup g, part[g, h] = 0 - sum_i e_i d_i with e_i = expf(x_i), x_i = s_h - lse_i:

    x_i:        one subtraction, |dx| <= U |x_i|, which moves exp(x_i) by the factor exp(dx): relative |x_i| U
    e_i:        expf                                                            -> relative H
    e_i d_i:    one multiply                                                    -> relative U
    term error: |e_i d_i| ((|x_i| + 1) U + H)
    the sum:    a lane adds its ceil(rpw / 64) terms in order (rpw = ceil(B Tq / G) rows per workgroup,
                G = min(ceil(B Tq / 256), 256)), then 6 butterfly rounds; 0 - acc is exact
                chain = ceil(rpw / 64) + 6, on the magnitudes sum_i |e_i d_i|
    partials:   MARGIN (sum_i term error + chain U sum_i |e_i d_i|), the G rows added in float64 by the test
    slot:       colreduce_multi adds the G rows (at most one add per row) and 1 for the old value, then rounds once:
                half_ulp(want + old) + MARGIN (sum_i term error + (chain + G + 1) U (sum_i |e_i d_i| + |old|))

In the attention test delta is the dQ kernel's own: D exact products (two 16-bit factors) summed in fp32, at most
D adds: |d delta_i| <= D U sum_d |dO O|, which enters the bound as e_i times that.
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
from qknorm_ref import MARGIN, U
from rowwise_ref import half_ulp

pytestmark = pytest.mark.gpu
DEV = "cuda"
SITE = 11
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
FORMATS = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
H = 2.0 ** -20
B, T = 2, 512
HEADS = pytest.mark.parametrize("Hq,Hkv,D", [(2, 2, 64), (8, 2, 128)])
CASES = ["causal", "w1", "w65", "w200", "doc", "qrange"]
MASKS = pytest.mark.parametrize("case", CASES)
QRANGE = (128, 384)


def close(a, b, atol, rtol, what=""):
    assert torch.isfinite(a).all(), f"{what}: non-finite values in the kernel output"
    a = a.float()
    b = b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).float().mean().item()
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
def inputs(Hq, Hkv, D, dtype):
    """(qkv, do, sink) of one shape, shared (read-only) by every case that runs it; the sinks are N(0, 2^2)."""
    g = torch.Generator(device=DEV).manual_seed(B * 1000003 + T * 1009 + Hq * 101 + Hkv * 11 + D)
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, device=DEV, generator=g).to(dtype)
    do = torch.randn(B * T, Hq * D, device=DEV, generator=g).to(dtype)
    sink = (2.0 * torch.randn(Hq, device=DEV, generator=g)).to(dtype)
    return qkv, do, sink


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


def operands(case, Hq, Hkv, D, dtype):
    qkv, do, sink = inputs(Hq, Hkv, D, dtype)
    q, k, v = split(qkv, Hq, Hkv, D)
    if case == "qrange":
        q, do = rows(q, *QRANGE), rows(do, *QRANGE)
    return q, k, v, do, sink


def forward(case, Hq, Hkv, D, dtype, sink):
    q, k, v, do, _ = operands(case, Hq, Hkv, D, dtype)
    o, lse, _ = F_.attn_fwd(q, k, v, B, T, Hq, Hkv, 1.0 / math.sqrt(D), True, 0.0, seed_obj(), SITE, sink=sink,
                            **mask_kw(case))
    return o, lse


def backward(case, Hq, Hkv, D, dtype, o, lse, sink):
    """(dq, dk, dv, dsink partials) through F_.attn_bwd with the kernels' own o and lse."""
    q, k, v, do, _ = operands(case, Hq, Hkv, D, dtype)
    dq = torch.full_like(q, float("nan"))               # every element must be written
    dk = torch.full_like(k, float("nan")).contiguous()
    dv = torch.full_like(v, float("nan")).contiguous()
    part = F_.attn_bwd(q, k, v, o, do, lse, None, dq, dk, dv, B, T, Hq, Hkv, 1.0 / math.sqrt(D), True, 0.0, seed_obj(),
                       SITE, sink=sink, **mask_kw(case))
    return dq, dk, dv, part


def sink_chain(Bk, Tq):
    """(G, chain) of the sink-gradient kernel for Bk rows of Tq queries (module docstring)."""
    R = Bk * Tq
    G = min(-(-R // 256), 256)
    rpw = -(-R // G)
    return G, -(-rpw // 64) + 6


def sink_bound(lse, delta, sink, ddelta=None):
    """(want [Hq], term-error sum [Hq], magnitude sum [Hq]) in float64 for fp32 lse / delta [B, Hq, Tq]."""
    x = sink.double().view(1, -1, 1) - lse.double()
    e = torch.exp(x)
    t = e * delta.double()
    terr = t.abs() * ((x.abs() + 1.0) * U + H)
    if ddelta is not None:
        terr = terr + e * ddelta
    return -t.sum((0, 2)), terr.sum((0, 2)), t.abs().sum((0, 2))


def check(what, got, want, bound):
    got, want = got.double(), want.double()
    assert got.shape == want.shape, what
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound, torch.zeros_like(err))
    print(f"{what}: worst error/bound {float(ratio.max()) if ratio.numel() else 0.0:.3f} ({got.numel()} elements)")
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    nbad = int((err > bound).sum())
    assert nbad == 0, f"{what}: {nbad} of {got.numel()} elements outside their bound, worst {float(ratio.max()):.3f}"


# ------------------------------------------------------------------------------------------- kernels against ref
@FORMATS
@HEADS
@MASKS
def test_kernels_against_ref_with_random_sinks(case, Hq, Hkv, D, dtype):
    q, k, v, do, sink = operands(case, Hq, Hkv, D, dtype)
    kw = mask_kw(case)
    scale = 1.0 / math.sqrt(D)
    Tq = q.shape[0] // B
    o, lse = forward(case, Hq, Hkv, D, dtype, sink)
    assert o.dtype == dtype and o.shape == (B * Tq, Hq * D) and lse.shape == (B, Hq, Tq) and lse.dtype == F32
    sd = seed_obj()
    ro, rlse = ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.0, sd, SITE, sink=sink, **kw)
    close(lse, rlse, 8e-3, 1e-3, "lse")
    close(o, ro, 2e-2, 3e-2, "O")
    # the sink took a visible share: without it lse is lower by more than the tolerance somewhere
    _, plain = ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.0, sd, SITE, **kw)
    assert float((rlse - plain).max()) > 0.1
    dq, dk, dv, part = backward(case, Hq, Hkv, D, dtype, o, lse, sink)
    rdq, rdk, rdv = torch.empty_like(dq), torch.empty_like(dk), torch.empty_like(dv)
    rds = ref.attn_bwd(q, k, v, o, do, lse, rdq, rdk, rdv, B, T, Hq, Hkv, scale, True, 0.0, sd, SITE, sink=sink, **kw)
    for name, a, b in zip("qkv", (dq, dk, dv), (rdq, rdk, rdv)):
        close(a, b, 5e-2, 5e-2, "d" + name)
    # the sink gradient: float64 of the formula on the kernel's lse and the exact delta of (dO, O)
    G, chain = sink_chain(B, Tq)
    assert tuple(part.shape) == (G, Hq) and part.dtype == F32
    prod = (do.double() * o.double()).view(B, Tq, Hq, D)
    delta64 = prod.sum(-1).transpose(1, 2)
    ddelta = D * U * prod.abs().sum(-1).transpose(1, 2)
    want, terr, mag = sink_bound(lse, delta64, sink, ddelta)
    check(f"dsink {case} {dtype} Hq={Hq}", part.double().sum(0), want, MARGIN * (terr + chain * U * mag))
    assert tuple(rds.shape) == (1, Hq) and float(want.abs().min()) > 0


# ------------------------------------------------------------------------------------------- exactness
@FORMATS
@HEADS
@MASKS
def test_very_negative_sink_is_the_sinkless_call_bit_for_bit(case, Hq, Hkv, D, dtype):
    """exp2 of the sink underflows to 0: a = exp2(0) = 1, l + 0, 1 / l -- o and lse are the sink-less kernel's."""
    sink = torch.full((Hq,), -30000.0, device=DEV, dtype=dtype)
    o0, lse0 = forward(case, Hq, Hkv, D, dtype, None)
    o1, lse1 = forward(case, Hq, Hkv, D, dtype, sink)
    assert torch.isfinite(o1).all() and torch.isfinite(lse1).all()
    assert same_bits(o0, o1), "o"
    assert same_bits(lse0, lse1), "lse"
    *_, part = backward(case, Hq, Hkv, D, dtype, o1, lse1, sink)
    assert bool((part == 0).all()), "dsink partials are not exact zeros"


@FORMATS
@HEADS
@MASKS
def test_large_sink(case, Hq, Hkv, D, dtype):
    """Every sink at +50: nearly all of each row's probability goes to the sink."""
    _, _, v, _, _ = operands(case, Hq, Hkv, D, dtype)
    sink = torch.full((Hq,), 50.0, device=DEV, dtype=dtype)
    o, lse = forward(case, Hq, Hkv, D, dtype, sink)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    assert float(o.float().abs().max()) < math.exp(-30.0) * float(v.float().abs().max())
    close(lse, torch.full_like(lse, 50.0), 8e-3, 1e-3, "lse")


# ------------------------------------------------------------------------------------------- sink-gradient kernel
@FORMATS
@pytest.mark.parametrize("Hq", [2, 5, 8])        # 2, 5: colreduce_multi's dword path; 5: a partly filled head group
@pytest.mark.parametrize("Bk,Tq", [(1, 128), (3, 640)])
def test_sink_gradient_kernel_against_float64(Bk, Tq, Hq, dtype):
    """(1, 128): one workgroup of 128 rows.  (3, 640): 1920 rows in 8 workgroups of 240, which cross batch rows."""
    C = ext()
    g = torch.Generator(DEV).manual_seed(17 * Tq + Hq)
    lse = 3.0 + 2.0 * torch.randn(Bk, Hq, Tq, device=DEV, generator=g)
    delta = torch.randn(Bk, Hq, Tq, device=DEV, generator=g)
    sink = (2.0 * torch.randn(Hq, device=DEV, generator=g)).to(dtype)
    G, chain = sink_chain(Bk, Tq)
    assert C.attn_sink_partials(Bk, Tq) == G == F_.attn_sink_partials(lse, Bk, Tq)
    part = C.attn_sink_bwd(lse, delta, sink)
    assert tuple(part.shape) == (G, Hq) and part.dtype == F32
    want, terr, mag = sink_bound(lse, delta, sink)
    what = f"attn_sink_bwd {dtype} B={Bk} Tq={Tq} Hq={Hq}"
    check(f"{what} partials", part.double().sum(0), want, MARGIN * (terr + chain * U * mag))
    slot0 = torch.randn(Hq, device=DEV, generator=g).to(dtype)
    for accumulate in (False, True):
        slot = slot0.clone()
        red = F_.GradReducer()
        p = F_.attn_sink_bwd(lse, delta, sink)
        assert same_bits(p, part), "repeated call"
        F_.reduce_partials(red, p, slot, accumulate)
        red.flush()
        prev = slot0.double() if accumulate else torch.zeros_like(want)
        b = half_ulp(want + prev, dtype) + MARGIN * (terr + (chain + G + 1) * U * (mag + prev.abs()))
        check(f"{what} slot acc={accumulate}", slot, want + prev, b)
    # two calls into one partial matrix (the context-parallel ranges): each writes its own rows, bit for bit
    big = torch.full((2 * G + 1, Hq), float("nan"), dtype=F32, device=DEV)
    for j in range(2):
        C.attn_sink_bwd(lse, delta, sink, big, j * G)
    assert same_bits(big[:G], part) and same_bits(big[G:2 * G], part)
    assert bool(torch.isnan(big[2 * G]).all()), "rows past the call's range were written"
    rows_ = F_.attn_sink_bwd(lse, delta, sink, big, G)
    assert same_bits(rows_, part)


def test_bindings_refuse_bad_operands():
    C = ext()
    Hq, Hkv, D = 2, 2, 64
    qkv, do, sink = inputs(Hq, Hkv, D, BF16)
    q, k, v = split(qkv, Hq, Hkv, D)
    scale = 1.0 / math.sqrt(D)
    with pytest.raises(RuntimeError, match="causal"):
        C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, False, 0.0, sink=sink)
    mask = C.attn_mask(B, T, Hq, 0.1, seed_obj().device_tensor, SITE, q)
    with pytest.raises(RuntimeError, match="p = 0"):
        C.attn_fwd(q, k, v, mask, B, T, Hq, Hkv, scale, True, 0.1, sink=sink)
    with pytest.raises(RuntimeError, match="Hq"):
        C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, sink=torch.zeros(Hq + 1, device=DEV, dtype=BF16))
    with pytest.raises(RuntimeError, match="dtype"):
        C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, sink=sink.to(F16))
    with pytest.raises(RuntimeError, match="dtype"):
        C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, sink=sink.float())
    with pytest.raises(ValueError, match="causal"):
        F_.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, False, 0.0, seed_obj(), SITE, sink=sink)
    with pytest.raises(ValueError, match="dropout"):
        F_.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.1, seed_obj(), SITE, sink=sink)
    lse = torch.zeros(B, Hq, T, device=DEV)
    with pytest.raises(RuntimeError, match="Hq"):
        C.attn_sink_bwd(lse, lse, torch.zeros(Hq + 1, device=DEV, dtype=BF16))
    with pytest.raises(RuntimeError, match="lse's shape"):
        C.attn_sink_bwd(lse, lse[:, :, :128].contiguous(), sink)
    G = C.attn_sink_partials(B, T)
    with pytest.raises(RuntimeError, match="partial rows out of range"):
        C.attn_sink_bwd(lse, lse, sink, torch.empty(G, Hq, device=DEV), 1)
    with pytest.raises(RuntimeError, match="part_out must be"):
        C.attn_sink_bwd(lse, lse, sink, torch.empty(G, Hq + 2, device=DEV), 0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- whole model
T_MODEL = 128


def _cfg(**kw):
    return ModelConfig(**dict(get_model_config("mtiny", T_MODEL).to_dict(), attn_sinks=True, **kw))


def _perturbed(cfg):
    torch.manual_seed(0)
    m = build_model(cfg)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for layer in m.model.layers:
            layer.self_attn.sinks.add_(torch.randn(cfg.n_head, generator=g))
    return m


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


@pytest.fixture(scope="module")
def model_runs():
    """One initialisation; the CPU reference run and the GPU runs per recompute mode, each computed once."""
    cfg = _cfg()
    base = _perturbed(cfg)
    idx = torch.randint(0, cfg.vocab_size, (2, T_MODEL), generator=torch.Generator().manual_seed(3))
    tgt = idx.roll(-1, 1)
    cache = {}

    def get(kind):
        if kind not in cache:
            m = copy.deepcopy(base) if kind == "cpu" else copy.deepcopy(base).to(DEV, BF16)
            m.rt = ParamRuntime()
            if kind != "cpu":
                m.activation_recompute = kind
            i, t = (idx, tgt) if kind == "cpu" else (idx.to(DEV), tgt.to(DEV))
            loss = m(i, t)[1]
            loss.backward()
            cache[kind] = (loss.detach(), {n: p.grad for n, p in m.named_parameters()})
        return cache[kind]
    return get


def test_model_matches_cpu_reference(model_runs):
    """The tolerances of tests/test_mistral_gpu.py for the same comparison."""
    l_cpu, g_cpu = model_runs("cpu")
    l_gpu, g_gpu = model_runs("off")
    assert abs(l_cpu.item() - l_gpu.item()) < 1e-2 * abs(l_cpu.item())
    assert sum(g.numel() for n, g in g_cpu.items() if n.endswith("sinks")) == 4
    for n, g in g_cpu.items():
        assert torch.isfinite(g_gpu[n]).all(), n
        r = rel(g_gpu[n], g)
        assert r < 6e-2, (n, r)


@pytest.mark.parametrize("mode", ["selective", "full"])
def test_model_recompute_equals_off_bit_for_bit(model_runs, mode):
    l0, g0 = model_runs("off")
    l1, g1 = model_runs(mode)
    assert torch.equal(l0, l1), (l0.item(), l1.item())
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def _train(graphed, moe, qk, accum=2, windows=2):
    torch.manual_seed(0)
    kw = dict(n_experts=4, moe_top_k=2, moe_dropless=True) if moe else {}
    cfg = _cfg(qk_norm=qk, **kw)
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


@pytest.mark.parametrize("qk", [False, True], ids=["", "qknorm"])
@pytest.mark.parametrize("moe", [False, True], ids=["dense", "moe_dropless"])
def test_graph_replay_equals_eager(moe, qk):
    """Two accumulation windows of two micro-steps under ZeRO-3: the replayed graphs train the eager steps' model bit
    for bit, dense and with --moe-experts 4 --moe-dropless, also together with --qk-norm."""
    l0, s0 = _train(False, moe, qk)
    l1, s1 = _train(True, moe, qk)
    assert all(l == l for l in l0) and l0 == l1, (l0, l1)
    names = [k for k in s0 if k.endswith("sinks")]
    assert len(names) == 2
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    assert all(bool((s0[k] != 0).any()) for k in names), "the sinks were not trained"


# ------------------------------------------------------------------------------------------- two ranks
TOL = dict(loss_tol=1e-3, upd_tol=0.02, cos_min=0.9998, param_tol=0.03)      # tests/test_context_parallel_gpu.py


def test_world2_cp2_zero3_equals_world1_gpu(tmp_path):
    """Two ranks sharing the GPU (gloo, host-staged buffers) as one context-parallel group under ZeRO-3 against the
    one-rank whole-row run, mtiny with sinks at 512 positions (zigzag: two ranges per rank, whose sink-gradient
    partials fill one matrix)."""
    args = ("--seq-len", "512", "--windows", "2", "--cases", "cp_zero3", "--attn-sinks")
    ws1 = run(tmp_path / "ws1.pt", 1, "cuda", extra=args, timeout=300)
    ws2 = run(tmp_path / "ws2.pt", 2, "cuda", extra=args + ("--context-parallel", "2"),
              env_extra={"DLTB_COMM": "host"}, timeout=300)
    bad = compare(ws1, ws2, **TOL)
    assert not bad, bad
    r1, r2 = ws1["cp_zero3"], ws2["cp_zero3"]
    names = [n for n in r1["init"] if n.endswith("sinks")]
    assert len(names) == 2
    for n in names:         # compare() looks at large updates only: the sinks within its param_tol here
        u1, u2 = r1["final"][n] - r1["init"][n], r2["final"][n] - r2["init"][n]
        assert float(u1.norm()) > 0, n
        assert float((u1 - u2).norm()) <= TOL["param_tol"] * float(u1.norm()), n
