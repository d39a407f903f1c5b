"""Row-scaled FP8 linear layers on the GPU (csrc/gemm_fp8.hip) against the contract of ops/ref.py: the quantiser bit for
bit, the GEMM bit for bit on integer operands and within a derived bound on random ones, the two linears, and a
two-layer model (d 256, T 256) with ``fp8_linear``."""
import pytest
import torch

import dltb  # noqa: F401
from dltb.models import build_model, get_model_config
from dltb.models.config import ModelConfig
from dltb.ops import functional as F_
from dltb.ops import ref
from dltb.parallel import GraphedStep, ParamRuntime, engine_config, make_engine

pytestmark = pytest.mark.gpu
DEV, BF16, F16 = "cuda", torch.bfloat16, torch.float16
T = 256


def _special(K, dtype):
    """Zero row; amax exactly 448 * 2^e and one ulp above; +-2^100 (bf16); a subnormal row; an inf row; a NaN row."""
    big = 2.0 ** 100 if dtype == BF16 else 2.0 ** 15
    ramp = torch.linspace(-0.9, 0.9, K)
    rows = [ramp * 0, ramp * 448 * 2.0 ** -7, ramp * 450 * 2.0 ** -7, ramp * big, ramp * 2.0 ** (-130 if dtype == BF16 else -20),
            ramp.clone(), ramp.clone()]
    for r, peak in zip(rows[1:5], (448 * 2.0 ** -7, 450 * 2.0 ** -7, -big, 2.0 ** (-130 if dtype == BF16 else -20))):
        r[K // 3] = peak
    rows[5][K - 1], rows[6][1] = float("inf"), float("nan")
    return torch.stack(rows).to(dtype)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("R,K", [(1, 128), (3, 4096), (130, 14336), (16, 28672)])
def test_quantiser_equals_the_reference_bit_for_bit(R, K, dtype):
    g = torch.Generator().manual_seed(R + K)
    span = 30 if dtype == BF16 else 6
    x = (torch.randn(R, K, generator=g) * 2.0 ** torch.randint(-span, span, (R, 1), generator=g)).to(dtype)
    x = torch.cat([x, _special(K, dtype)])
    q, s = F_.fp8_quant_rows(x.to(DEV))
    wq, ws = ref.fp8_quant_rows(x)
    assert torch.equal(s.cpu().view(torch.int32), ws.view(torch.int32))
    assert torch.equal(q.cpu(), wq)
    xb = torch.stack([x, x.flip(0)]).to(DEV)                  # the batched form: two matrices, one launch
    qb, sb = F_.fp8_quant_rows(xb)
    assert torch.equal(qb[0], q) and torch.equal(sb[1].view(torch.int32), s.flip(0).view(torch.int32))


def _int_operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    qa, qb = (torch.randint(-4, 5, (n, K), generator=g).float().to(torch.float8_e4m3fn).view(torch.uint8) for n in (M, N))
    sa, sb = (2.0 ** torch.randint(-3, 4, (n,), generator=g).float() for n in (M, N))
    return qa, sa, qb, sb


# one k-step; an odd count of k-steps over several tiles; ring wrap (depth + 1 k-steps: 4 + 1 at 128 x 128, 3 + 1 at
# 256 x 128); each tile config with more than one tile in both directions
@pytest.mark.parametrize("M,N,K,cfg,dtype", [(128, 128, 128, -1, BF16), (256, 384, 640, 0, BF16), (384, 128, 640, 0, BF16),
                                             (512, 256, 512, 1, BF16), (256, 384, 640, 1, F16)])
def test_gemm_is_exact_on_integer_operands(M, N, K, cfg, dtype):
    qa, sa, qb, sb = _int_operands(M, N, K, M + N + K)
    want = (ref.fp8_dec(qa).double() @ ref.fp8_dec(qb).double().t()) * sa.double()[:, None] * sb.double()[None]
    got = F_.gemm_fp8_nt(qa.to(DEV), sa.to(DEV), qb.to(DEV), sb.to(DEV), dtype, cfg)
    assert got.dtype == dtype and torch.equal(got.cpu(), want.to(dtype))


def test_gemm_on_random_codes_within_the_derived_bound():
    """Per element 2^-8 |ref| (the bf16 rounding) + K 2^-23 sum_k |a| |b| sa sb (fp32 accumulation of exact products)."""
    M = N = 256
    K = 4096
    g = torch.Generator().manual_seed(1)
    (qa, sa), (qb, sb) = (ref.fp8_quant_rows(torch.randn(n, K, generator=g).to(BF16)) for n in (M, N))
    a, b = ref.fp8_dec(qa).double() * sa.double()[:, None], ref.fp8_dec(qb).double() * sb.double()[:, None]
    want, mags = a @ b.t(), a.abs() @ b.abs().t()
    got = F_.gemm_fp8_nt(qa.to(DEV), sa.to(DEV), qb.to(DEV), sb.to(DEV)).cpu().double()
    excess = ((got - want).abs() - (2.0 ** -8 * want.abs() + K * 2.0 ** -23 * mags)).max().item()
    print(f"largest error minus bound: {excess:.3e}")
    assert excess <= 0


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
def test_linears_against_the_reference_and_fallback(dtype):
    g = torch.Generator().manual_seed(2)
    x, w, dy = (torch.randn(*s, generator=g).to(dtype) for s in ((256, 256), (384, 256), (256, 384)))
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    n0 = F_.fp8_gemm_calls
    for got, got_q, want in ((F_.linear_fp8_fwd(xd, wd), F_.linear_fp8_fwd(xd, wd, F_.fp8_quant_rows(wd)),
                              ref.linear_fp8_fwd(x, w)),
                             (F_.linear_fp8_dgrad(dyd, wd), F_.linear_fp8_dgrad(dyd, wd, F_.fp8_quant_rows(wd.t().contiguous())),
                              ref.linear_fp8_dgrad(dy, w))):
        assert torch.equal(got, got_q)                         # supplied and freshly made weight codes
        # same codes on both sides (the quantiser is bit-exact); the sums differ in fp32 order only
        assert (got.cpu().float() - want.float()).abs().max() <= 2.0 ** -7 * want.float().abs().max()
    assert F_.fp8_gemm_calls == n0 + 4
    x192, w192 = xd[:, :192].contiguous(), wd[:, :192].contiguous()       # K = 192: the 16-bit path
    assert torch.equal(F_.linear_fp8_fwd(x192, w192), F_.linear_fwd(x192, w192)) and F_.fp8_gemm_calls == n0 + 4


def _cfg(**kw):
    base = dict(get_model_config("mtiny", T).to_dict(), n_embd=256, n_head=4, n_kv_head=2, ffn_hidden=512)
    return ModelConfig(**dict(base, **kw))


_RUNS = {}


def model_run(kind, **kw):
    """Loss and gradients of one bf16 step of the two-layer model: ``cpu`` (ref.py) or a GPU recompute mode."""
    if (kind, tuple(sorted(kw.items()))) not in _RUNS:
        cfg = _cfg(**kw)
        torch.manual_seed(0)
        m = build_model(cfg)
        idx = torch.randint(0, cfg.vocab_size, (2, T), generator=torch.Generator().manual_seed(3))
        m = m.to(BF16)
        if kind != "cpu":
            m, idx = m.to(DEV), idx.to(DEV)
            m.activation_recompute = kind
        m.rt = ParamRuntime()
        loss = m(idx, idx.roll(-1, 1))[1]
        loss.backward()
        _RUNS[(kind, tuple(sorted(kw.items())))] = (loss.detach(), {n: p.grad for n, p in m.named_parameters()})
    return _RUNS[(kind, tuple(sorted(kw.items())))]


def test_model_matches_the_cpu_reference_step():
    """The comparison and tolerances of the model equivalence tests (tests/test_sandwich_norm_gpu.py: loss 1e-2,
    every gradient 6e-2 relative).  The ref.py CPU step runs in bf16, the step's own format, so both sides round where
    the kernels round and quantise the same values: an E4M3 code is a discrete choice, and against the fp32 CPU step
    (which those tests use) a bf16 rounding of an activation moves about 3 % of the codes by a whole E4M3 step.  At
    this shape the fp32 and the bf16 CPU steps themselves are 0.057 .. 0.093 apart on the gradients (0.064 on the head's,
    which no FP8 product reaches), and the GPU step measured 0.0725 against the fp32 one on the embedding."""
    (l_cpu, g_cpu), (l_gpu, g_gpu) = model_run("cpu", fp8_linear=True), model_run("off", fp8_linear=True)
    assert F_.fp8_gemm_calls >= 16                             # 2 layers x 4 products x (forward + data gradient)
    print(f"loss cpu {l_cpu.item():.6f} gpu {l_gpu.item():.6f}")
    assert abs(l_cpu.item() - l_gpu.item()) < 1e-2 * abs(l_cpu.item())
    for n, g in g_cpu.items():
        r = ((g_gpu[n].float().cpu() - g).norm() / g.norm().clamp(min=1e-12)).item()
        print(f"{n}: {r:.4f}")
        assert r < 6e-2, (n, r)


def test_recompute_full_equals_off_and_flag_off_is_the_default_run():
    (l0, g0), (l1, g1) = model_run("off", fp8_linear=True), model_run("full", fp8_linear=True)
    assert torch.equal(l0, l1) and all(torch.equal(g0[n], g1[n]) for n in g0)
    n0 = F_.fp8_gemm_calls
    (ld, _), (lf, _) = model_run("off"), model_run("off", fp8_linear=False)
    assert torch.equal(ld, lf) and F_.fp8_gemm_calls == n0 and not torch.equal(ld, l0)


def _train(graphed):
    torch.manual_seed(0)
    cfg = _cfg(fp8_linear=True)
    with torch.device(DEV):
        model = build_model(cfg)
    eng = make_engine(model, engine_config("zero3", 2, "reference", compute_dtype=BF16), "cuda:0")
    eng.train()
    g = torch.Generator(device=DEV).manual_seed(1)
    runner = GraphedStep(eng) if graphed else None
    losses = []
    for _ in range(6):                                          # three windows of two micro-steps
        idx = torch.randint(0, cfg.vocab_size, (2, T), device=DEV, generator=g)
        if runner is None:
            loss = eng(idx, idx.roll(-1, 1))[1]
            eng.backward(loss)
            eng.step()
        else:
            loss = runner(idx, idx.roll(-1, 1))
        losses.append(loss.item())
    assert runner is None or (len(runner.graphs) == eng.accum and not runner.disabled)
    mats = ((512, 256), (256, 256), (1024, 256), (256, 512))    # qkv, o, gate|up, down: codes of W and W^T + their scales
    assert eng.weight_q_cache_bytes() == cfg.n_layer * sum(2 * n * k + 4 * (n + k) for n, k in mats)
    return losses, {k: v.detach().clone() for k, v in eng.full_state_dict().items()}


def test_graph_replay_equals_eager_across_optimizer_steps():
    """The replayed graphs train the eager model bit for bit over three optimizer steps, so the cached weight codes
    are refreshed inside the graphs as they are eagerly."""
    (l0, s0), (l1, s1) = _train(False), _train(True)
    assert all(l == l for l in l0) and l0 == l1, (l0, l1)
    assert all(torch.equal(s0[k], s1[k]) for k in s0)
