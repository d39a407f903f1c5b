"""QK-norm fused with RoPE on the MI355X (csrc/qknorm.hip): the two kernels against the float64 references of
tests/qknorm_ref.py in both 16-bit formats, the whole model against the CPU reference path, the bit-for-bit
equalities (recompute modes, HIP-graph replay, MoE), and ZeRO-3 with context parallelism on two host-staged ranks.
The CPU definitions: tests/test_qknorm_cpu.py.

No tolerance is taken from what a kernel returns.  The bounds follow tests/test_rowwise_gpu.py (U = 2^-24 per fp32
rounding, MARGIN = 2 on the fp32 part, H = 2^-20 assumed for the hardware rsqrt; ``half_ulp`` for the one rounding to
16 bits) and are evaluated by ``fwd_bound`` / ``bwd_bounds`` of tests/qknorm_ref.py, whose formulas
tests/test_qknorm_cpu.py's docstring derives.  What is specific to the kernels is the length of their sums; a head
spans L = D / 16 lanes of 16 elements each:

    var = mean(x^2):   16 squares and 16 adds in a lane, log2(L) butterfly rounds, (the 1 / D factor is a power of two),
                       the eps add                                           -> n_var = 33 + log2(L)
    mean(gw xh):       16 adds in a lane and log2(L) butterfly rounds        -> n_dot = 16 + log2(L)
    weight gradients:  a thread adds its share of the workgroup's (row, head) items, ceil(rpw heads L / 256) at most
                       (rpw = ceil(N / G) rows per workgroup, G = min(ceil(N / 8), 1024) workgroups), then
                       log2(64 / L) shuffle rounds over the wave and 3 adds over the four waves; colreduce_multi adds
                       the G partial rows (at most one add per row, in whatever order) and 1 for the old value:
                       chain = ceil(rpw heads L / 256) + log2(64 / L) + 3 + G + 1, as ``colsum_bound``'s chain, on
                       the magnitudes sum|g xh| + |old|; each term g xh carries its own error (``bwd_bounds``).
"""
import copy
import math

import pytest
import torch

import dltb  # noqa: F401
from dltb.models import build_model, get_model_config
from dltb.models.config import ModelConfig
from dltb.ops import functional as F_
from dltb.ops import ref
from dltb.ops._ext import ext
from dltb.parallel import GraphedStep, ParamRuntime, engine_config, make_engine

from multirank_util import compare, run
from qknorm_ref import MARGIN, U, bwd_bounds, fwd_bound, qknorm_rope64, qknorm_rope_bwd64
from rowwise_ref import half_ulp

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
FORMATS = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
H = 2.0 ** -20          # one hardware approximation, relative (assumed: tests/test_rowwise_gpu.py)
EPS = 1e-5
SHAPES = pytest.mark.parametrize("N,T", [(1, 1), (7 * 43, 43)])
HEADS = pytest.mark.parametrize("Hq,Hkv", [(2, 1), (8, 2)])
DIMS = pytest.mark.parametrize("D", [64, 128])


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def check(what, got, want, bound):
    got, want = got.double(), want.double()
    assert got.shape == want.shape, what
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound, torch.zeros_like(err))
    print(f"{what}: worst error/bound {float(ratio.max()) if ratio.numel() else 0.0:.3f} ({got.numel()} elements)")
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    nbad = int((err > bound).sum())
    assert nbad == 0, f"{what}: {nbad} of {got.numel()} elements outside their bound, worst {float(ratio.max()):.3f}"


def inputs(dtype, N, Hq, Hkv, D, pad, seed):
    """A [N, (Hq + 2 Hkv) D + pad] buffer whose first (Hq + 2 Hkv) D columns are the strided qkv view; head rows as
    in tests/test_qknorm_cpu.py: two all-zero head rows, in fp16 two scaled to 2^14."""
    g = torch.Generator(DEV).manual_seed(seed)
    heads = Hq + Hkv
    W = (Hq + 2 * Hkv) * D
    buf = torch.randn(N, W + pad, device=DEV, generator=g)
    x = buf[:, :heads * D].view(N, heads, D)
    if N > 4:
        x[1, 0] = 0.0
        x[2, heads - 1] = 0.0
        if dtype == F16:
            x[3, 0] *= 2.0 ** 14 / float(x[3, 0].abs().max())
            x[4, heads - 1] *= 2.0 ** 14 / float(x[4, heads - 1].abs().max())
    wq = (1.0 + 0.5 * torch.randn(D, device=DEV, generator=g)).to(dtype)
    wk = (1.0 + 0.5 * torch.randn(D, device=DEV, generator=g)).to(dtype)
    dbuf = torch.randn(N, W + pad, device=DEV, generator=g).to(dtype)
    return buf.to(dtype), dbuf, wq, wk, W


def tables(T, D, sub):
    """The kernel's fp32 tables for T positions; ``sub``: rows [T, 2 T) of a table for 2 T positions, as context
    parallelism passes a range's rows (a view into the position-indexed table)."""
    if not sub:
        return ref.rope_tables(T, D, 10000.0, DEV)
    cos, sin = ref.rope_tables(2 * T, D, 10000.0, DEV)
    return cos[T:], sin[T:]


# ------------------------------------------------------------------------------------------- 7. forward kernel
@FORMATS
@SHAPES
@HEADS
@DIMS
@pytest.mark.parametrize("sub", [False, True], ids=["", "subrange"])
def test_forward_against_float64(dtype, D, Hq, Hkv, N, T, sub):
    C = ext()
    heads, L = Hq + Hkv, D // 16
    buf, _, wq, wk, W = inputs(dtype, N, Hq, Hkv, D, 24, 11 * D + Hq + N)
    cos, sin = tables(T, D, sub)
    before = buf.clone()
    qkv = buf[:, :W]
    assert N == 1 or not qkv.is_contiguous()
    x = before[:, :heads * D].reshape(N, heads, D)
    raw = C.qknorm_rope_fwd(qkv, wq, wk, cos, sin, T, Hq, Hkv, D, EPS)
    assert raw.is_contiguous() and same_bits(raw, before[:, :heads * D].contiguous()), "raw is not the input"
    assert same_bits(buf[:, heads * D:], before[:, heads * D:]), "bytes outside the q|k columns were written"
    got = buf[:, :heads * D].reshape(N, heads, D)
    want, _ = qknorm_rope64(x, wq, wk, cos, sin, T, Hq, EPS)
    n_var = 33 + int(math.log2(L))
    check(f"qknorm_rope_fwd {dtype} D={D} Hq={Hq} N={N} sub={sub}", got, want,
          fwd_bound(dtype, x, wq, wk, cos, sin, T, Hq, EPS, want, n_var, H))
    if N > 4:
        assert bool((got[1, 0] == 0).all()) and bool((got[2, heads - 1] == 0).all())     # rstd = 1 / sqrt(eps), y = 0
    buf2 = before.clone()
    raw2 = C.qknorm_rope_fwd(buf2[:, :W], wq, wk, cos, sin, T, Hq, Hkv, D, EPS)
    assert same_bits(buf2, buf) and same_bits(raw2, raw), "repeated call"
    # the functional wrapper is this kernel
    buf3 = before.clone()
    raw3 = F_.qknorm_rope_fwd(buf3[:, :W], wq, wk, cos, sin, T, Hq, Hkv, D, EPS)
    assert same_bits(buf3, buf) and same_bits(raw3, raw)


def test_bindings_refuse_bad_operands():
    C = ext()
    N, T, Hq, Hkv, D = 4, 4, 2, 1, 64
    buf, dbuf, wq, wk, W = inputs(BF16, N, Hq, Hkv, D, 0, 1)
    cos, sin = tables(T, D, False)
    raw = C.qknorm_rope_fwd(buf.clone(), wq, wk, cos, sin, T, Hq, Hkv, D, EPS)
    with pytest.raises(RuntimeError, match="D must be 64 or 128"):
        C.qknorm_rope_fwd(buf, wq[:32], wk[:32], cos, sin, T, Hq, Hkv, 32, EPS)
    with pytest.raises(RuntimeError, match="weight size"):
        C.qknorm_rope_fwd(buf, wq[:32], wk, cos, sin, T, Hq, Hkv, D, EPS)
    with pytest.raises(RuntimeError, match="table size"):
        C.qknorm_rope_fwd(buf, wq, wk, cos[:2], sin, T, Hq, Hkv, D, EPS)
    with pytest.raises(RuntimeError, match="exceeds row"):
        C.qknorm_rope_fwd(buf[:, :128], wq, wk, cos, sin, T, Hq, Hkv, D, EPS)
    with pytest.raises(RuntimeError, match="rows % T"):
        C.qknorm_rope_fwd(buf[:3], wq, wk, cos, sin, T, Hq, Hkv, D, EPS)
    with pytest.raises(RuntimeError, match="all be bf16 or all fp16"):
        C.qknorm_rope_fwd(buf, wq.to(F16), wk, cos, sin, T, Hq, Hkv, D, EPS)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        C.qknorm_rope_fwd(torch.zeros(N, W + 8, dtype=BF16, device=DEV)[:, 4:4 + W], wq, wk, cos, sin, T, Hq, Hkv, D,
                          EPS)
    with pytest.raises(RuntimeError, match="raw shape"):
        C.qknorm_rope_bwd_(dbuf, raw[:, :64].contiguous(), wq, wk, cos, sin, T, Hq, Hkv, D, EPS)
    part = torch.empty(2, C.qknorm_partials(N), D, dtype=F32, device=DEV)
    with pytest.raises(RuntimeError, match="partial rows out of range"):
        C.qknorm_rope_bwd_(dbuf, raw, wq, wk, cos, sin, T, Hq, Hkv, D, EPS, part, 1)
    with pytest.raises(RuntimeError, match="part_out must be"):
        C.qknorm_rope_bwd_(dbuf, raw, wq, wk, cos, sin, T, Hq, Hkv, D, EPS, part[:, :, :32], 0)


# ------------------------------------------------------------------------------------------- 8. backward kernel
def check_backward(dtype, D, Hq, Hkv, N, T):
    C = ext()
    heads, L = Hq + Hkv, D // 16
    buf, dbuf, wq, wk, W = inputs(dtype, N, Hq, Hkv, D, 24, 13 * D + Hq + N)
    cos, sin = tables(T, D, False)
    x = buf[:, :heads * D].reshape(N, heads, D)
    raw = buf[:, :heads * D].contiguous()
    dbefore = dbuf.clone()
    dy = dbefore[:, :heads * D].reshape(N, heads, D)
    part = C.qknorm_rope_bwd_(dbuf[:, :W], raw, wq, wk, cos, sin, T, Hq, Hkv, D, EPS)
    G = min(-(-N // 8), 1024)
    assert C.qknorm_partials(N) == G and tuple(part.shape) == (2, G, D) and part.dtype == F32
    assert same_bits(dbuf[:, heads * D:], dbefore[:, heads * D:]), "bytes outside the q|k columns of dqkv were written"
    want_dx, want_dwq, want_dwk = qknorm_rope_bwd64(dy, x, wq, wk, cos, sin, T, Hq, EPS)
    n_var, n_dot = 33 + int(math.log2(L)), 16 + int(math.log2(L))
    bdx, term, mags = bwd_bounds(dtype, dy, x, wq, wk, cos, sin, T, Hq, EPS, want_dx, n_var, n_dot, H)
    what = f"qknorm_rope_bwd {dtype} D={D} Hq={Hq} N={N}"
    check(f"{what} dx", dbuf[:, :heads * D].reshape(N, heads, D), want_dx, bdx)
    rpw = -(-N // G)
    chain = -(-rpw * heads * L // 256) + int(math.log2(64 // L)) + 3
    sums = ((0, want_dwq, slice(0, Hq), "dwq"), (1, want_dwk, slice(Hq, heads), "dwk"))
    for k, want, sl, name in sums:          # the fp32 partials, summed in float64 here
        b = term[:, sl].sum((0, 1)) + MARGIN * chain * U * mags[:, sl].sum((0, 1))
        check(f"{what} {name} partials", part[k].double().sum(0), want, b)
    slots0 = [torch.randn(D, device=DEV, generator=torch.Generator(DEV).manual_seed(5 + k)).to(dtype) for k in (0, 1)]
    for accumulate in (False, True):
        slots = [s.clone() for s in slots0]
        red = F_.GradReducer()
        pq, pk = F_.qknorm_rope_bwd_(dbefore.clone()[:, :W], raw, wq, wk, cos, sin, T, Hq, Hkv, D, EPS)
        F_.reduce_partials(red, pq, slots[0], accumulate)
        F_.reduce_partials(red, pk, slots[1], accumulate)
        red.flush()
        assert same_bits(pq, part[0]) and same_bits(pk, part[1]), "repeated call"
        for k, want, sl, name in sums:
            prev = slots0[k].double() if accumulate else torch.zeros_like(want)
            b = half_ulp(want + prev, dtype) + term[:, sl].sum((0, 1)) \
                + MARGIN * (chain + G + 1) * U * (mags[:, sl].sum((0, 1)) + prev.abs())
            check(f"{what} {name} slot acc={accumulate}", slots[k], want + prev, b)
    d2 = dbefore.clone()
    part2 = C.qknorm_rope_bwd_(d2[:, :W], raw, wq, wk, cos, sin, T, Hq, Hkv, D, EPS)
    assert same_bits(d2, dbuf) and same_bits(part2, part), "repeated call"
    # two calls into one partial matrix (the context-parallel ranges): each writes its own rows, bit for bit
    big = torch.full((2, 2 * G + 1, D), float("nan"), dtype=F32, device=DEV)
    for j in range(2):
        C.qknorm_rope_bwd_(dbefore.clone()[:, :W], raw, wq, wk, cos, sin, T, Hq, Hkv, D, EPS, big, j * G)
    for k in (0, 1):
        assert same_bits(big[k, :G], part[k]) and same_bits(big[k, G:2 * G], part[k])
        assert bool(torch.isnan(big[k, 2 * G]).all()), "rows past the call's range were written"


@FORMATS
@SHAPES
@HEADS
@DIMS
def test_backward_against_float64(dtype, D, Hq, Hkv, N, T):
    """dx and the weight gradients through GradReducer, overwriting and accumulating onto a non-zero slot.  N = 301:
    38 workgroups of 8 rows (the last with 5)."""
    check_backward(dtype, D, Hq, Hkv, N, T)


@FORMATS
def test_backward_past_the_workgroup_cap(dtype):
    """N = 8200 > 8 * 1024: the workgroup count stops at 1024, a workgroup takes 9 rows, and the workgroups from 912
    on own no row and write zero partials."""
    check_backward(dtype, 64, 2, 1, 8200, 8200)


# ------------------------------------------------------------------------------------------- 9 / 10. whole model
T_MODEL = 128


def _qk_cfg(**kw):
    return ModelConfig(**dict(get_model_config("mtiny", T_MODEL).to_dict(), qk_norm=True, **kw))


def _perturbed(cfg):
    torch.manual_seed(0)
    m = build_model(cfg)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for layer in m.model.layers:
            layer.self_attn.q_norm.weight.add_(0.3 * torch.randn(cfg.head_dim, generator=g))
            layer.self_attn.k_norm.weight.add_(0.3 * torch.randn(cfg.head_dim, generator=g))
    return m


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


@pytest.fixture(scope="module")
def model_runs():
    """One initialisation; the CPU reference run and the GPU runs per recompute mode, each computed once."""
    cfg = _qk_cfg()
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
    assert sum("q_norm" in n or "k_norm" in n for n in g_cpu) == 4
    for n, g in g_cpu.items():
        r = rel(g_gpu[n], g)
        assert r < 6e-2, (n, r)


@pytest.mark.parametrize("mode", ["selective", "full"])
def test_model_recompute_equals_off_bit_for_bit(model_runs, mode):
    l0, g0 = model_runs("off")
    l1, g1 = model_runs(mode)
    assert torch.equal(l0, l1), (l0.item(), l1.item())
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def _train(graphed, moe, accum=2, windows=2):
    torch.manual_seed(0)
    cfg = _qk_cfg(**(dict(n_experts=4, moe_top_k=2, moe_dropless=True) if moe else {}))
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


@pytest.mark.parametrize("moe", [False, True], ids=["dense", "moe_dropless"])
def test_graph_replay_equals_eager(moe):
    """Two accumulation windows of two micro-steps under ZeRO-3, recompute off: the replayed graphs train the eager
    steps' model bit for bit; with --moe-experts 4 --moe-dropless the flag-on model runs and does the same."""
    l0, s0 = _train(False, moe)
    l1, s1 = _train(True, moe)
    assert all(l == l for l in l0) and l0 == l1, (l0, l1)
    names = [k for k in s0 if "q_norm" in k or "k_norm" in k]
    assert len(names) == 4
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    assert any(not bool((s0[k] == 1).all()) for k in names), "the QK-norm weights were not trained"


# ------------------------------------------------------------------------------------------- 11. two ranks
TOL = dict(loss_tol=1e-3, upd_tol=0.02, cos_min=0.9998, param_tol=0.03)      # tests/test_context_parallel_gpu.py


def test_world2_cp2_zero3_equals_world1_gpu(tmp_path):
    """Two ranks sharing the GPU (gloo, host-staged buffers) as one context-parallel group under ZeRO-3 against the
    one-rank whole-row run, mtiny with QK-norm at 512 positions (zigzag: two ranges per rank)."""
    args = ("--seq-len", "512", "--windows", "2", "--cases", "cp_zero3", "--qk-norm")
    ws1 = run(tmp_path / "ws1.pt", 1, "cuda", extra=args, timeout=300)
    ws2 = run(tmp_path / "ws2.pt", 2, "cuda", extra=args + ("--context-parallel", "2"),
              env_extra={"DLTB_COMM": "host"}, timeout=300)
    bad = compare(ws1, ws2, **TOL)
    assert not bad, bad
    r1, r2 = ws1["cp_zero3"], ws2["cp_zero3"]
    names = [n for n in r1["init"] if "q_norm" in n or "k_norm" in n]
    assert len(names) == 4
    for n in names:         # compare() looks at large updates only: the new weights within its param_tol here
        u1, u2 = r1["final"][n] - r1["init"][n], r2["final"][n] - r2["init"][n]
        assert float(u1.norm()) > 0, n
        assert float((u1 - u2).norm()) <= TOL["param_tol"] * float(u1.norm()), n
