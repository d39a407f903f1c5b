"""Dropless mixture-of-experts routing on the MI355X: the packed assignment bit for bit against ops/ref.py, the two
grouped GEMMs of csrc/gemm_grouped.hip against float64 with the format-derived bound of tests/test_moe_gpu.py (empty
groups, a tail, every pipeline depth), the layer at its edges and against float64 beside the capacity layer at factor
E / K, a HIP-graph step replayed on a batch with another routing, and every strategy against the capacity model.
(The hand-written backward against autograd: tests/test_moe_dropless_cpu.py, in float64.)"""
import copy

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
RING_ROWS = 4 * 64                   # the grouped kernels' LDS ring: 4 stages of 64 k-elements


# ------------------------------------------------------------------------------------------- bounds (test_moe_gpu.py)
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


def _grid(shape, gen):
    """Integers in [-8, 8] times 2^-3 (exact in both formats; dot products of 128 of them are exact in fp32)."""
    return torch.randint(-8, 9, shape, generator=gen).double() / 8.0


# ------------------------------------------------------------------------------------------- assignment
@pytest.mark.parametrize("N,K,E", [(1, 1, 2), (63, 1, 64), (64, 4, 64), (65, 2, 3), (1030, 4, 7), (4100, 2, 64)])
def test_assign_dropless_sizes(N, K, E):
    """The sizes of tests/test_moe_gpu.py::test_assign_sizes, with its crowded expert 0: bit for bit."""
    gen = torch.Generator().manual_seed(N)
    expert = torch.stack([torch.randperm(E, generator=gen)[:K] for _ in range(N)]).to(torch.int32)
    expert[: N // 2, 0] = 0
    if K > 1:
        expert[: N // 2, 1:] = torch.stack([1 + torch.randperm(E - 1, generator=gen)[:K - 1]
                                            for _ in range(N // 2)]).to(torch.int32)
    want = ref.moe_assign_dropless(expert, E)
    got = F_.moe_assign_dropless(expert.to(DEV), E)
    assert got[1].shape[0] == ref.moe_dropless_rows(N, E, K)
    for w, g, name in zip(want, got, ("slot", "src", "src_k", "counts", "offsets")):
        assert g.dtype == torch.int32 and torch.equal(g.cpu(), w), name
    counts_out = torch.full((E,), -7, dtype=torch.int32, device=DEV)
    again = F_.moe_assign_dropless(expert.to(DEV), E, counts_out)
    assert again[3] is counts_out and torch.equal(counts_out.cpu(), want[3])


@pytest.mark.parametrize("name,E", [("all_to_one", 8), ("one_each", 64)])
def test_assign_dropless_adversarial(name, E):
    expert = torch.zeros(200, 1, dtype=torch.int32) if name == "all_to_one" \
        else torch.arange(64, dtype=torch.int32).view(64, 1)
    want = ref.moe_assign_dropless(expert, E)
    got = F_.moe_assign_dropless(expert.to(DEV), E)
    for w, g in zip(want, got):
        assert torch.equal(g.cpu(), w)
    assert int(got[4][E]) <= got[1].shape[0]


# ------------------------------------------------------------------------------------------- grouped NT
NT_OFFSETS = [0, 0, 128, 384, 384, 384]      # 0, 128, 256 rows, then two adjacent empty groups; a tail of 128 rows


@pytest.fixture(scope="module")
def nt_inputs():
    gen = torch.Generator().manual_seed(41)
    R, E = 512, 5
    return {(K, N): (torch.randn(R, K, generator=gen), [torch.randn(N, K, generator=gen) for _ in range(E)])
            for K in (64, 256, 576) for N in (128, 512)}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [128, 512])
@pytest.mark.parametrize("K", [64, 256, 576])        # 1, 4 and 9 k-steps: a ring that never fills, fills, wraps
def test_gemm_grouped_nt(nt_inputs, K, N, dtype):
    a32, bs32 = nt_inputs[(K, N)]
    a, bs = a32.to(DEV, dtype), [b.to(DEV, dtype) for b in bs32]
    offsets = torch.tensor(NT_OFFSETS, dtype=torch.int32)
    out = torch.full((a.shape[0], N), float("nan"), dtype=dtype, device=DEV)  # a sentinel everywhere
    got = F_.gemm_grouped_nt(a, offsets.to(DEV), bs, out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    a64, bs64 = a.double().cpu(), [b.double().cpu() for b in bs]
    want = ref.gemm_grouped_nt(a64, offsets, bs64)
    mag = ref.gemm_grouped_nt(a64.abs(), offsets, [b.abs() for b in bs64])
    check(got, want, mag, K, dtype, f"grouped NT K={K} N={N}")
    assert (got[NT_OFFSETS[-1]:] == 0).all() and (a[NT_OFFSETS[-1]:] != 0).any()      # the tail: exact zeros
    assert torch.isfinite(got).all()                                            # no sentinel left anywhere
    fresh = F_.gemm_grouped_nt(a, offsets.to(DEV), bs)                          # a new output: bitwise the same
    assert torch.equal(fresh.view(torch.int16), got.view(torch.int16))


INT_OFFSETS = [0, 128, 128, 384]             # 128, 0 and 256 rows; a tail of 128 rows
INT_ROWS = INT_OFFSETS[-1] + 128


def _ints(shape, gen, dtype):
    return torch.randint(-1, 2, shape, generator=gen).to(DEV, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gemm_grouped_nt_exact_on_small_integers(dtype):
    """Entries in {-1, 0, 1}: every fp32 sum is exact in any order, so each segment must equal its fp32 product bit
    for bit at 1 and 9 k-steps (a stage read early or a k-slice paired wrongly cannot hide in a bound)."""
    gen = torch.Generator().manual_seed(47)
    offsets = torch.tensor(INT_OFFSETS, dtype=torch.int32, device=DEV)
    for K in (64, 576):
        a = _ints((INT_ROWS, K), gen, dtype)
        bs = [_ints((128, K), gen, dtype) for _ in INT_OFFSETS[1:]]
        out = torch.full((INT_ROWS, 128), float("nan"), dtype=dtype, device=DEV)
        F_.gemm_grouped_nt(a, offsets, bs, out)
        want = torch.zeros_like(out)                                              # the tail: exact zeros
        for e, b in enumerate(bs):
            rows = slice(INT_OFFSETS[e], INT_OFFSETS[e + 1])
            want[rows] = (a[rows].float() @ b.float().t()).to(dtype)
        assert (a[INT_OFFSETS[-1]:] != 0).any() and torch.equal(out, want), f"K {K}"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("empty_accumulates", [False, True])
def test_gemm_grouped_tn_exact_on_small_integers(dtype, empty_accumulates):
    """As above for the weight gradients: an accumulating group of 2 k-steps, an empty one (exact zeros, or its slot
    untouched when accumulating) and an overwriting group of 4; the tail rows hold NaN and belong to nobody."""
    gen = torch.Generator().manual_seed(53)
    offsets = torch.tensor(INT_OFFSETS, dtype=torch.int32, device=DEV)
    dy, x = _ints((INT_ROWS, 128), gen, dtype), _ints((INT_ROWS, 128), gen, dtype)
    dy[INT_OFFSETS[-1]:] = float("nan")
    old = [_ints((128, 128), gen, dtype) for _ in INT_OFFSETS[1:]]
    acc = [True, empty_accumulates, False]
    dws = [o.clone() for o in old]
    F_.gemm_grouped_tn(dy, x, offsets, dws, acc)
    for e, flag in enumerate(acc):
        rows = slice(INT_OFFSETS[e], INT_OFFSETS[e + 1])
        want = dy[rows].float().t() @ x[rows].float() + (old[e].float() if flag else 0.0)
        assert torch.equal(dws[e], want.to(dtype)), f"group {e}, accumulate {flag}"


def test_gemm_grouped_nt_refuses_what_it_cannot_run():
    off = torch.tensor([0, 128], dtype=torch.int32, device=DEV)
    mk = lambda r, c: torch.zeros(r, c, dtype=torch.bfloat16, device=DEV)
    for a, b in ((mk(128, 32), mk(128, 32)), (mk(64, 64), mk(128, 64)), (mk(128, 64), mk(64, 64))):
        with pytest.raises(RuntimeError, match="gemm_grouped_nt"):
            F_.gemm_grouped_nt(a, off, [b])
    with pytest.raises(RuntimeError):
        F_.gemm_grouped_nt(mk(128, 64), off, [mk(128, 64).half()])            # mixed formats
    with pytest.raises(RuntimeError):
        F_.gemm_grouped_nt(mk(128, 64), off, [mk(128, 64), mk(128, 64)])      # one b per segment


# ------------------------------------------------------------------------------------------- grouped TN
TN_LENGTHS = [0, 0, 128, 256, 512, 1152]      # k-steps 0, 0, 2, 4, 8, 18: empty, below / at / above the ring's depth
TN_ACC = [True, False, False, True, False, True]


@pytest.fixture(scope="module")
def tn_inputs():
    gen = torch.Generator().manual_seed(43)
    R = sum(TN_LENGTHS) + 128                                                  # a tail the kernel must not read
    M, N = 256, 128
    return (torch.randn(R, M, generator=gen), torch.randn(R, N, generator=gen),
            [torch.randn(M, N, generator=gen) for _ in TN_LENGTHS])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gemm_grouped_tn(tn_inputs, dtype):
    assert max(TN_LENGTHS) > RING_ROWS and 2 * 64 in TN_LENGTHS and RING_ROWS in TN_LENGTHS
    dy32, x32, old32 = tn_inputs
    dy, x = dy32.to(DEV, dtype), x32.to(DEV, dtype)
    off = [0]
    for n in TN_LENGTHS:
        off.append(off[-1] + n)
    offsets = torch.tensor(off, dtype=torch.int32)
    dy[off[-1]:] = float("nan")                                                # the tail belongs to nobody
    old = [o.to(DEV, dtype) for o in old32]

    def once():
        dws = [o.clone() for o in old]
        F_.gemm_grouped_tn(dy, x, offsets.to(DEV), dws, TN_ACC)
        torch.cuda.synchronize()
        return dws

    dws = once()
    dy64, x64 = dy.double().cpu(), x.double().cpu()
    for e, (n, acc) in enumerate(zip(TN_LENGTHS, TN_ACC)):
        rows = slice(off[e], off[e + 1])
        if n == 0:
            if acc:
                assert torch.equal(dws[e], old[e]), "an empty group under accumulate must leave its slot"
            else:
                assert (dws[e] == 0).all(), "an empty group writes exact zeros"
            continue
        want = dy64[rows].t() @ x64[rows]
        mag = dy64[rows].abs().t() @ x64[rows].abs()
        ops = n
        if acc:
            o64 = old[e].double().cpu()
            want, mag, ops = want + o64, mag + o64.abs(), n + 1
        check(dws[e], want, mag, ops, dtype, f"grouped TN group {e} ({n} rows, accumulate {acc})")
    for a, b in zip(dws, once()):                                              # a fixed summation order
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# ------------------------------------------------------------------------------------------- the layer
def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


def _layer_model(E, K, dtype, dropless=True, d=128, f=256):
    kw = dict(moe_dropless=True) if dropless else dict(moe_capacity_factor=E / K)
    cfg = ModelConfig(arch="mistral", vocab_size=64, n_embd=d, n_head=2, n_kv_head=1, n_layer=1, ffn_hidden=f,
                      block_size=512, dropout=0.0, causal=True, tie_embeddings=False, n_experts=E, moe_top_k=K, **kw)
    torch.manual_seed(2)
    model = mistral.MistralLM(cfg).to(DEV, dtype)
    model.rt = ParamRuntime()
    with torch.no_grad():
        for ex in model.model.layers[0].mlp.experts:    # larger experts: outputs and gradients of order 1
            ex.gate_up_proj.weight.mul_(8.0)
            ex.down_proj.weight.mul_(8.0)
    return cfg, model


def _run_layer(mod, h, dm):
    unit = mod.unit_blocks[0]
    ws = mod.rt.acquire(unit)
    m, saved = mistral._moe_fwd(mod, 0, h, ws[4:])
    s = [(torch.full_like(w, float("nan")), False) for w in ws]
    dh = mistral._moe_bwd(mod, unit, dm, h, ws, s, saved)
    return m, dh, [t for t, _ in s[4:]], saved


def _f64_twin(model):
    m64 = copy.deepcopy(model).cpu().double()
    m64.rt = ParamRuntime()
    return m64


ROUNDS = 6       # roundings to the storage format on the longest path of the layer: gu, hh, ye, m forward (xe is a
#                  copy); dye, dhh, dgu, dxe, dh backward, with gu's own rounding under dgu -- at most 6 in a row


def chain_limit(dtype, cancel=1):
    """Relative L2 limit of a layer output against the float64 run.  One rounding to the format moves every element
    by at most 2^-p of itself (p = 8 bf16, 11 fp16), so the tensor by at most 2^-p in relative L2; to first order the
    roundings of a chain add up, each carried on by stages that map a perturbation like the signal.  ``cancel``: 2 for
    the router gradient, whose softmax backward g_k (dgate_k - sum_j g_j dgate_j) is a difference of terms of equal
    size.  The fp32 accumulation (u = 2^-24) is below 1 % of either figure.  Set before any measurement."""
    p = 8 if dtype == torch.bfloat16 else 11
    return cancel * ROUNDS * 2.0 ** -p


def _check_chain(m_g, dh_g, grads_g, m_c, dh_c, grads_c, E, dtype, what):
    lim = chain_limit(dtype)
    rm, rd = rel(m_g, m_c), rel(dh_g, dh_c)
    print(f"{what}: chain rel L2 m {rm:.2e} dh {rd:.2e} (limit {lim:.2e})")
    assert rm < lim and rd < lim, (what, rm, rd, lim)
    names = ["router"] + [f"experts.{e}.{w}" for e in range(E) for w in ("gate_up", "down")]
    worst = 0.0
    for n, a, b in zip(names, grads_g, grads_c):
        assert torch.isfinite(a).all(), n
        if float(b.abs().max()) == 0:
            assert float(a.float().abs().max()) == 0, (what, n)                 # exact zeros, not stale memory
            continue
        r, l = rel(a, b), chain_limit(dtype, 2 if n == "router" else 1)
        worst = max(worst, r / l)
        assert r < l, (what, n, r, l)
    print(f"{what}: worst gradient rel L2 / limit = {worst:.3f}")


def _check_layer(model, got, want, h, dm, E, dtype, what):
    """The layer's output, data gradient and 1 + 2 E weight gradients against the float64 run of the same functions
    (:func:`chain_limit`), and each of its six grouped products against float64 of its own device inputs with the
    single-rounding bound: the two forward ones from the saved tensors, the four backward ones from the backward's
    intermediates rebuilt here with the layer's own calls (dye, dhh, dgu, dxe; every kernel is deterministic, and the
    rebuilt chain must end in the layer's dh bit for bit)."""
    m_g, dh_g, grads_g, saved_g = got
    m_c, dh_c, grads_c, saved_c = want
    for i in (0, 2, 3):                                  # expert, slot, src: equal by construction (exact logits)
        assert torch.equal(saved_g[i].cpu(), saved_c[i]), i
    assert torch.equal(saved_g[8].cpu(), saved_c[8])     # offsets
    _check_chain(m_g, dh_g, grads_g, m_c, dh_c, grads_c, E, dtype, what)
    expert, gate, slot, src, xe, ye, gu, hh, offsets = saved_g[:9]
    unit = model.unit_blocks[0]
    ws = model.rt.acquire(unit)
    f64 = lambda t: t.double().cpu()
    off = offsets.cpu()
    bounds = off.tolist()
    ju, jd = [5 + 2 * e for e in range(E)], [6 + 2 * e for e in range(E)]

    def nt(a, c, bs64, what2):
        a64 = f64(a)
        want_c = ref.gemm_grouped_nt(a64, off, bs64)
        mag = ref.gemm_grouped_nt(a64.abs(), off, [b.abs() for b in bs64])
        check(c, want_c, mag, a.shape[1], dtype, f"{what}: {what2}")

    def tn(dy, x, dws, what2):
        dy64, x64 = f64(dy), f64(x)
        worst = 0.0
        for e, dw in enumerate(dws):
            rows = slice(bounds[e], bounds[e + 1])
            if rows.stop == rows.start:
                assert (dw == 0).all(), (what, what2, e)
                continue
            want_w = dy64[rows].t() @ x64[rows]
            mag = dy64[rows].abs().t() @ x64[rows].abs()
            b = bound(want_w, mag, rows.stop - rows.start, dtype)
            worst = max(worst, ((f64(dw) - want_w).abs() / b).max().item())
        print(f"{what}: {what2}: max err / bound = {worst:.3f}")
        assert worst <= 1.0, (what, what2, worst)

    # forward
    nt(xe, gu, [f64(ws[j]) for j in ju], "gate|up product")
    nt(hh, ye, [f64(ws[j]) for j in jd], "down product")
    # backward, rebuilt with the layer's calls
    dye, _, dlogits = F_.moe_combine_bwd(dm, ye, slot, src, expert, gate, E)
    tn(dye, hh, [grads_g[2 + 2 * e] for e in range(E)], "down weight gradients (TN)")
    wdt = mistral._moe_weights_t(model.rt, unit, ws, jd)
    for t, j in zip(wdt, jd):
        assert torch.equal(t, ws[j].t())                 # the W^T the product runs on (cached or the scratch copies)
    dhh = F_.gemm_grouped_nt(dye, offsets, wdt)
    nt(dye, dhh, [f64(ws[j]).t() for j in jd], "dhh = dye Wd (NT on W^T)")
    dgu = F_.swiglu_bwd(dhh, gu)
    tn(dgu, xe, [grads_g[1 + 2 * e] for e in range(E)], "gate|up weight gradients (TN)")
    wgt = mistral._moe_weights_t(model.rt, unit, ws, ju)
    dxe = F_.gemm_grouped_nt(dgu, offsets, wgt)
    nt(dgu, dxe, [f64(ws[j]).t() for j in ju], "dxe = dgu Wgu (NT on W^T)")
    dh_again = F_.moe_dispatch_bwd(dxe, slot, dlogits, ws[4])
    assert torch.equal(dh_again.view(torch.int16), dh_g.view(torch.int16)), "the rebuilt chain is not the layer's"


def _edge(model, h64, dm64, dtype, E, what):
    m64 = _f64_twin(model)
    h, dm = h64.to(DEV, dtype), dm64.to(DEV, dtype)
    got = _run_layer(model, h, dm)
    want = _run_layer(m64, h64, dm64)
    _check_layer(model, got, want, h, dm, E, dtype, what)
    return got, want


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layer_edge_everything_to_expert_0(dtype):
    E, K, N, d = 8, 1, 200, 128
    cfg, model = _layer_model(E, K, dtype)
    gen = torch.Generator().manual_seed(5)
    h64 = torch.randint(1, 9, (N, d), generator=gen).double() / 8.0           # positive rows
    with torch.no_grad():
        wr = model.model.layers[0].mlp.router.weight
        for e in range(E):
            wr[e].fill_(1.0 - e / 8.0)                   # logits strictly descending in e: expert 0 first, no tie
    dm64 = torch.randn(N, d, generator=gen).to(dtype).double()
    got, _ = _edge(model, h64, dm64, dtype, E, "all to expert 0")
    saved = got[3]
    assert (saved[0] == 0).all() and saved[8].tolist() == [0] + [256] * E
    assert saved[4].shape[0] == 256 + 128 * E
    assert model.moe_counts(DEV)[0].tolist() == [N] + [0] * (E - 1)
    assert (got[0] != 0).any(1).all()                    # nobody dropped: every token has an output
    for e in range(1, E):
        assert (got[2][1 + 2 * e] == 0).all() and (got[2][2 + 2 * e] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layer_edge_64_experts_mostly_empty(dtype):
    E, K, N, d = 64, 2, 65, 128
    cfg, model = _layer_model(E, K, dtype)
    gen = torch.Generator().manual_seed(6)
    h64 = _grid((N, d), gen)
    h64[:, 0] = 1.0
    wr64 = _grid((E, d), gen) / 64.0                     # logits of the rest: |.| < 0.5 in practice, exact in fp32
    for e, v in ((3, 2.0), (17, 1.75), (40, 1.5)):       # three experts far above the rest: the top 2 come from them
        wr64[e, 0] = v
    with torch.no_grad():
        model.model.layers[0].mlp.router.weight.copy_(wr64)
    dm64 = torch.randn(N, d, generator=gen).to(dtype).double()
    got, _ = _edge(model, h64, dm64, dtype, E, "E 64, N 65")
    counts = model.moe_counts(DEV)[0]
    assert int((counts == 0).sum()) >= 61 and int(counts.sum()) == N * K


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layer_edge_counts_128_127_129(dtype):
    E, K, N, d = 4, 1, 384, 128
    cfg, model = _layer_model(E, K, dtype)
    gen = torch.Generator().manual_seed(7)
    tgt = torch.cat([torch.zeros(128), torch.ones(127), torch.full((129,), 2.0)]).long()[torch.randperm(N, generator=gen)]
    h64 = _grid((N, d), gen)
    h64[:, :4] = 0.0
    h64[torch.arange(N), tgt] = 4.0                      # logit 4 for the target, 0 for the others: exact
    wr64 = torch.zeros(E, d, dtype=torch.float64)
    wr64[:, :4] = torch.eye(4, dtype=torch.float64)
    with torch.no_grad():
        model.model.layers[0].mlp.router.weight.copy_(wr64)
    dm64 = torch.randn(N, d, generator=gen).to(dtype).double()
    got, _ = _edge(model, h64, dm64, dtype, E, "counts 128 / 127 / 129")
    assert model.moe_counts(DEV)[0].tolist() == [128, 127, 129, 0]
    assert got[3][8].tolist() == [0, 128, 256, 512, 512]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layer_and_capacity_layer_against_float64(dtype):
    """The dropless layer and the capacity layer at factor E / K on the same weights, each against the float64 run
    (never against each other): N = 200, E = 8, K = 2, ties and two crowded experts."""
    E, K, N, d = 8, 2, 200, 128
    cfg, model = _layer_model(E, K, dtype)
    gen = torch.Generator().manual_seed(39)
    h64 = _grid((N, d), gen)
    wr64 = _grid((E, d), gen) / 16.0
    wr64[E - 2] = wr64[1]
    h64[:, 0] = 1.0
    wr64[0, 0] += 1.0
    wr64[2, 0] += 0.75
    with torch.no_grad():
        model.model.layers[0].mlp.router.weight.copy_(wr64)
    dm64 = torch.randn(N, d, generator=gen).to(dtype).double()
    _, want = _edge(model, h64, dm64, dtype, E, "dropless")
    _, cap = _layer_model(E, K, dtype, dropless=False)
    cap.load_state_dict(model.state_dict())
    m_g, dh_g, grads_g, saved_g = _run_layer(cap, h64.to(DEV, dtype), dm64.to(DEV, dtype))
    assert (saved_g[2] >= 0).all() and torch.equal(saved_g[0].cpu(), want[3][0])      # no drops, the same routing
    m_c, dh_c, grads_c, _ = want
    _check_chain(m_g, dh_g, grads_g, m_c, dh_c, grads_c, E, dtype, "capacity at E / K")


# ------------------------------------------------------------------------------------------- graphs and strategies
def _train(strategy, graphed, steps=6, accum=2, T=128):
    torch.manual_seed(0)
    cfg = get_model_config("mtiny", T)
    cfg.n_experts, cfg.moe_top_k, cfg.moe_dropless = 4, 2, True
    cfg.validate()
    with torch.device(DEV):
        model = build_model(cfg)
    eng = make_engine(model, engine_config(strategy, accum, "reference"), "cuda:0")
    eng.train()
    g = torch.Generator(device=DEV).manual_seed(1)
    runner = GraphedStep(eng) if graphed else None
    losses, counts = [], []
    for _ in range(steps):
        idx = torch.randint(0, cfg.vocab_size, (2, T), device=DEV, generator=g)      # a new batch: routing changes
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


def test_graph_replay_on_another_routing_is_eager_bit_for_bit():
    """Graphs captured on the first window's batches are replayed on batches with other counts per expert: equal to
    the eager steps only if the kernels read the offsets on the device."""
    l0, s0, c0 = _train("zero3", False)
    l1, s1, c1 = _train("zero3", True)
    assert l0 == l1, (l0, l1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    for a, b in zip(c0, c1):
        assert torch.equal(a, b)
    assert len({tuple(c.flatten().tolist()) for c in c0}) == len(c0)     # every step saw other counts: the replays too


def test_strategies_against_the_capacity_model(tmp_path):
    """zero2, zero3, ddp and fsdp at world 1, and zero3 on two host-staged ranks, with --moe-dropless against the
    capacity model at factor E / K = 2 (nothing drops, so both compute the same function up to GEMM rounding)."""
    base = ("--seq-len", "128", "--windows", "2", "--moe-experts", "4")
    cases = "cp_ddp,cp_fsdp,cp_zero2,cp_zero3,zero3_mistral"
    cap = run(tmp_path / "cap.pt", 1, "cuda", extra=base + ("--cases", cases, "--moe-capacity-factor", "2.0"))
    one = run(tmp_path / "w1.pt", 1, "cuda", extra=base + ("--cases", cases, "--moe-dropless"))
    bad = compare(cap, one, **TOL)
    assert not bad, bad
    two = run(tmp_path / "w2.pt", 2, "cuda", extra=base + ("--cases", "zero3_mistral", "--moe-dropless"),
              env_extra={"DLTB_COMM": "host", "DLTB_COMM_LAZY": "1"})
    bad = compare({"zero3_mistral": cap["zero3_mistral"]}, two, **TOL)
    assert not bad, bad
