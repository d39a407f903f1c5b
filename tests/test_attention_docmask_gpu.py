"""Document-masked causal attention for packed sequences on the MI355X: the ``attn_doc_bounds`` kernel against
``ref.doc_bounds`` (exact), and the bounds-driven forward / dQ / dK/dV kernels against the fp32 reference of
dltb.ops.ref, which shares the dropout hash with the kernels.

A token equal to the EOS id ends a document and belongs to it; query i sees keys ``lo[i] <= j <= i``.  Layouts
are given as the document end positions of a row.  Method, ``close`` (finite first, zero elements out of
tolerance) and tolerances are those of tests/test_attention_window_gpu.py.

The "no EOS is bitwise causal" cases hold for these inputs, not by construction: the bounds kernels keep the
windowed kernels' per-row lazy rescale of the running max, the causal kernels rescale a whole wave at once,
and the two agree bit for bit as long as no row's max moves by more than 2^8 after its first tile -- which
N(0, 1) scores never do.  Against the windowed kernels the arithmetic is the same statement by statement.
"""
import copy
import functools
import math

import pytest
import torch

import dltb
from dltb.models import build_model, get_model_config
from dltb.ops import functional as F_
from dltb.ops import ref
from dltb.ops._ext import ext
from dltb.ops.rng import StepSeed
from dltb.parallel import GraphedStep, ParamRuntime, engine_config, make_engine

pytestmark = pytest.mark.gpu
DEV = "cuda"
SITE = 11
EOS = 255
VOCAB = 256


def close(a, b, atol, rtol, what=""):
    assert torch.isfinite(a).all(), f"{what}: non-finite values in the kernel output"
    a = a.float()
    b = b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).float().mean().item()
    assert bad == 0.0, f"{what}: {bad*100:.3f}% elements out of tolerance, max err {err.max().item():.4g}"


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


@functools.lru_cache(maxsize=None)
def inputs(B, T, Hq, Hkv, D, dtype=torch.bfloat16):
    """(qkv, do) of one shape, shared (read-only) by every case that runs it."""
    g = torch.Generator(device=DEV).manual_seed(B * 1000003 + T * 1009 + Hq * 101 + Hkv * 11 + D)
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, device=DEV, generator=g).to(dtype)
    do = torch.randn(B * T, Hq * D, device=DEV, generator=g).to(dtype)
    return qkv, do


def tokens(T, rows, seed=0):
    """int64 [len(rows), T] on the CPU: random non-EOS tokens with EOS at each row's document end positions."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, EOS, (len(rows), T), generator=g, dtype=torch.int64)
    for b, ends in enumerate(rows):
        for e in ends:
            idx[b, e] = EOS
    return idx


def bounds_of(T, rows, window=0):
    """Device bounds of the layout from the kernel, checked exactly against ref.doc_bounds."""
    idx = tokens(T, rows)
    got = ext().attn_doc_bounds(idx.to(DEV), EOS, window)
    want = ref.doc_bounds(idx, EOS, window)
    assert got.dtype == torch.int32 and tuple(got.shape) == (2, len(rows), T)
    assert torch.equal(got.cpu(), want)
    return got


def run_kernels(qkv, do, B, T, Hq, Hkv, D, p, sd, fused, bounds=None, window=0):
    """(o, lse, dq, dk, dv) of the HIP kernels; ``fused``: the model's path (dQ pass forms delta itself)."""
    C = ext()
    q, k, v = split(qkv, Hq, Hkv, D)
    scale = 1.0 / math.sqrt(D)
    amask = C.attn_mask(B, T, Hq, p, sd.device_tensor, SITE, q) if p else None
    o, lse = C.attn_fwd(q, k, v, amask, B, T, Hq, Hkv, scale, True, p, window=window, bounds=bounds)
    dqkv = torch.full_like(qkv, float("nan"))          # every element must be written
    if fused:
        F_.attn_bwd(q, k, v, o, do, lse, amask, *split(dqkv, Hq, Hkv, D), B, T, Hq, Hkv, scale, True, p, sd, SITE,
                    window=window, bounds=bounds)
    else:
        C.attn_bwd(q, k, v, o, do, lse, amask, *split(dqkv, Hq, Hkv, D), B, T, Hq, Hkv, scale, True, p,
                   window=window, bounds=bounds)
    return (o, lse) + split(dqkv, Hq, Hkv, D)


def check_against_ref(B, T, Hq, Hkv, D, p, rows, window=0, dtype=torch.bfloat16):
    assert len(rows) == B
    qkv, do = inputs(B, T, Hq, Hkv, D, dtype)
    q, k, v = split(qkv, Hq, Hkv, D)
    scale = 1.0 / math.sqrt(D)
    sd = seed_obj()
    bounds = bounds_of(T, rows, window)
    o, lse, dq, dk, dv = run_kernels(qkv, do, B, T, Hq, Hkv, D, p, sd, fused=False, bounds=bounds)
    assert o.dtype == dtype
    ro, rlse = ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, p, sd, SITE, bounds=bounds)
    # tolerances of test_kernels_gpu.py::test_attention for the same quantities
    close(lse, rlse, 8e-3, 1e-3, "lse")
    close(o, ro, 2e-2, 3e-2, "O")
    rdqkv = torch.empty_like(qkv)
    ref.attn_bwd(q, k, v, o, do, lse, *split(rdqkv, Hq, Hkv, D), B, T, Hq, Hkv, scale, True, p, sd, SITE,
                 bounds=bounds)
    for name, a, b in zip("qkv", (dq, dk, dv), split(rdqkv, Hq, Hkv, D)):
        close(a, b, 5e-2, 5e-2, "d" + name)
    fo, flse, fdq, fdk, fdv = run_kernels(qkv, do, B, T, Hq, Hkv, D, p, sd, fused=True, bounds=bounds)
    for name, a, b in zip("qkv", (fdq, fdk, fdv), split(rdqkv, Hq, Hkv, D)):
        close(a, b, 5e-2, 5e-2, "fused-delta d" + name)


# ------------------------------------------------------------------------------ bounds kernel
@pytest.mark.parametrize("window", [0, 100])
@pytest.mark.parametrize("T", [1, 100, 512, 2048])
def test_doc_bounds_kernel_is_exact(T, window):
    """B = 3 with a different layout per row: random document ends, none, and every token an EOS; T = 1, a T
    below the 256 threads of the row's workgroup, and chunks of 2 and 8 tokens per thread."""
    g = torch.Generator().manual_seed(T)
    idx = torch.randint(0, EOS, (3, T), generator=g, dtype=torch.int64)
    idx[0, torch.rand(T, generator=g) < 0.05] = EOS
    idx[2, :] = EOS
    if T > 1:
        idx[0, 0] = EOS
        idx[0, T - 1] = EOS
    got = ext().attn_doc_bounds(idx.to(DEV), EOS, window)
    want = ref.doc_bounds(idx, EOS, window)
    assert got.dtype == torch.int32 and tuple(got.shape) == (2, 3, T)
    assert torch.equal(got.cpu(), want)


# ------------------------------------------------------------------------------ layout sweep
# T = 512 is four query blocks of 128 and eight key tiles of 64.  Document ends of a row:
LAYOUTS = {
    "none": [],
    "len1": list(range(512)),           # every tile is an edge tile, every row of every wave starts a document,
                                        # and each wave sees one tile: the other key splits have none
    "e63": [63], "e64": [64], "e65": [65], "e127": [127], "e128": [128], "e129": [129],   # around tile / block edges
    "e300": [300],                      # mid-wave
    "e0": [0], "e511": [511],
    "run3": list(range(130, 256, 3)),   # 3-token documents filling tiles 2-3, then one long document: blocks
                                        # with many edge tiles and splits without a visible tile
    "pairs": [31, 32, 33, 95, 96, 97],
}
NAMES = list(LAYOUTS)


def rows_for(name):
    """Batch row 0 has the layout, row 1 another one of the list."""
    return [LAYOUTS[name], LAYOUTS[NAMES[(NAMES.index(name) + 5) % len(NAMES)]]]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("Hq,Hkv,D", [(2, 2, 64), (8, 2, 128)])      # (8, 2, 128): the head-split dK/dV path
@pytest.mark.parametrize("name", NAMES)
def test_docmask_layout_sweep(name, Hq, Hkv, D, p):
    check_against_ref(2, 512, Hq, Hkv, D, p, rows_for(name))


@pytest.mark.parametrize("Hq,Hkv,D", [(2, 2, 64), (8, 2, 128)])
def test_docmask_length_one_documents_are_exact(Hq, Hkv, D):
    """Every row sees only its own key: P = 1, so O is the row's V of its KV head bit for bit and lse the scaled
    diagonal score."""
    B, T = 2, 512
    qkv, do = inputs(B, T, Hq, Hkv, D)
    q, k, v = split(qkv, Hq, Hkv, D)
    bounds = bounds_of(T, [LAYOUTS["len1"]] * B)
    o, lse = ext().attn_fwd(q, k, v, None, B, T, Hq, Hkv, 1.0 / math.sqrt(D), True, 0.0, bounds=bounds)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    want = v.reshape(B * T, Hkv, D).repeat_interleave(Hq // Hkv, 1).reshape(B * T, Hq * D)
    assert torch.equal(o, want)
    kk = k.reshape(B * T, Hkv, D).repeat_interleave(Hq // Hkv, 1).float()
    diag = (q.reshape(B * T, Hq, D).float() * kk).sum(-1) / math.sqrt(D)          # [B*T, Hq]
    close(lse, diag.view(B, T, Hq).transpose(1, 2), 8e-3, 1e-3, "lse")


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("window", [0, 100])
@pytest.mark.parametrize("Hq,Hkv,D", [(2, 2, 64), (8, 2, 128)])
def test_docmask_without_eos_is_bitwise_causal_or_windowed(window, Hq, Hkv, D, p):
    """D = 128 with dropout is the dQ instantiation that runs unsplit and sums even and odd key tiles apart, to
    give the bits of the two-split causal / windowed kernels (csrc/attention.hip dq_ks_doc)."""
    B, T = 2, 512
    qkv, do = inputs(B, T, Hq, Hkv, D)
    sd = seed_obj()
    base = run_kernels(qkv, do, B, T, Hq, Hkv, D, p, sd, fused=False, window=window)
    got = run_kernels(qkv, do, B, T, Hq, Hkv, D, p, sd, fused=False, bounds=bounds_of(T, [[], []], window))
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), got, base):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), name


@pytest.mark.parametrize("p", [0.1, 0.0])
def test_docmask_composes_with_window_long_t_d64(p):
    """T = 1024 at D = 64 is where the causal dQ pass changes its split count (the bounds pass does not)."""
    check_against_ref(1, 1024, 4, 4, 64, p, [[200, 700]], window=100)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("Hq,Hkv,D", [(4, 2, 64), (4, 2, 128)])
def test_docmask_exact_locality(Hq, Hkv, D, p):
    """Boundary {299}: rows 300.. and rows ..299 are different documents, and nothing crosses the boundary."""
    B, T, e = 1, 512, 299
    qkv, do = inputs(B, T, Hq, Hkv, D)
    sd = seed_obj()
    bounds = bounds_of(T, [[e]])
    o, lse, dq, dk, dv = run_kernels(qkv, do, B, T, Hq, Hkv, D, p, sd, fused=False, bounds=bounds)
    g = torch.Generator(device=DEV).manual_seed(5)
    # K and V rows 0 .. 299 replaced: rows 300.. of o, lse, dq keep every bit
    qkv2 = qkv.clone()
    qkv2[:e + 1, Hq * D:] = torch.randn(e + 1, 2 * Hkv * D, device=DEV, generator=g).to(qkv.dtype)
    o2, lse2, dq2, _, _ = run_kernels(qkv2, do, B, T, Hq, Hkv, D, p, sd, fused=False, bounds=bounds)
    for x in (o, lse, dq, dk, dv, o2, lse2, dq2):
        assert torch.isfinite(x).all()
    assert torch.equal(o[e + 1:], o2[e + 1:])
    assert torch.equal(lse[..., e + 1:], lse2[..., e + 1:])
    assert torch.equal(dq[e + 1:], dq2[e + 1:])
    # Q and dO rows 300.. replaced (their o, lse follow): dk, dv of rows 0 .. 299 keep every bit
    qkv3, do3 = qkv.clone(), do.clone()
    qkv3[e + 1:, :Hq * D] = torch.randn(T - e - 1, Hq * D, device=DEV, generator=g).to(qkv.dtype)
    do3[e + 1:] = torch.randn(T - e - 1, Hq * D, device=DEV, generator=g).to(do.dtype)
    _, _, _, dk3, dv3 = run_kernels(qkv3, do3, B, T, Hq, Hkv, D, p, sd, fused=False, bounds=bounds)
    assert torch.isfinite(dk3).all() and torch.isfinite(dv3).all()
    assert torch.equal(dk[:e + 1], dk3[:e + 1])
    assert torch.equal(dv[:e + 1], dv3[:e + 1])
    # row 299 is the first document's last: it does see key 0
    qkv4 = qkv.clone()
    qkv4[0, Hq * D:] = qkv2[0, Hq * D:]
    o4 = run_kernels(qkv4, do, B, T, Hq, Hkv, D, p, sd, fused=False, bounds=bounds)[0]
    assert not torch.equal(o[e], o4[e])
    assert torch.equal(o[e + 1:], o4[e + 1:])


def test_docmask_fp16_build():
    """fp16 tensors select the fp16 objects of the same kernels (tests/test_fp16_gpu.py)."""
    check_against_ref(2, 512, 8, 2, 128, 0.1, rows_for("run3"), dtype=torch.float16)


def test_docmask_refusals():
    C = ext()
    B, T, Hq, Hkv, D = 2, 512, 2, 2, 64
    qkv, do = inputs(B, T, Hq, Hkv, D)
    q, k, v = split(qkv, Hq, Hkv, D)
    scale = 1.0 / math.sqrt(D)
    o, lse = C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0)
    g = split(torch.empty_like(qkv), Hq, Hkv, D)
    delta = torch.empty_like(lse)
    bounds = bounds_of(T, [[100], [200]])
    with pytest.raises(RuntimeError, match="causal"):
        C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, False, 0.0, bounds=bounds)
    with pytest.raises(RuntimeError, match="causal"):
        C.attn_bwd(q, k, v, o, do, lse, None, *g, B, T, Hq, Hkv, scale, False, 0.0, bounds=bounds)
    with pytest.raises(RuntimeError, match="causal"):
        C.attn_bwd_part(1, q, k, v, do, lse, delta, None, g[0], None, B, T, Hq, Hkv, scale, False, 0.0,
                        bounds=bounds)
    with pytest.raises(RuntimeError, match="either bounds or window"):
        C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, window=64, bounds=bounds)
    with pytest.raises(RuntimeError, match="either bounds or window"):
        C.attn_bwd(q, k, v, o, do, lse, None, *g, B, T, Hq, Hkv, scale, True, 0.0, window=64, bounds=bounds)
    for bad in (bounds[:1], bounds[:, :1], bounds[:, :, :256], bounds.reshape(2, B * T)):      # wrong shape
        with pytest.raises(RuntimeError, match=r"\[2, B, T\]"):
            C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, bounds=bad)
    with pytest.raises(RuntimeError, match=r"\[2, B, T\]"):
        C.attn_bwd_part(0, q, k, v, do, lse, delta, None, g[1], g[2], B, T, Hq, Hkv, scale, True, 0.0,
                        bounds=bounds[:, :1])
    with pytest.raises(RuntimeError, match="int32"):                                            # wrong dtype
        C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, bounds=bounds.long())
    with pytest.raises(RuntimeError, match="int32"):
        C.attn_bwd(q, k, v, o, do, lse, None, *g, B, T, Hq, Hkv, scale, True, 0.0, bounds=bounds.float())
    with pytest.raises(RuntimeError, match="device"):
        C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, bounds=bounds.cpu())
    with pytest.raises(ValueError, match="causal"):
        F_.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, False, 0.0, seed_obj(), SITE, bounds=bounds)
    with pytest.raises(ValueError, match="either bounds or window"):
        F_.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.0, seed_obj(), SITE, window=64, bounds=bounds)
    with pytest.raises(RuntimeError, match="int64"):
        C.attn_doc_bounds(torch.zeros(2, 8, dtype=torch.int32, device=DEV), 1, 0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ model
def _doc_model_cfg():
    cfg = get_model_config("mtiny", 256)
    cfg.doc_eos_id = EOS
    cfg.validate()
    return cfg


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


def test_docmask_mistral_hip_matches_cpu_reference():
    """Method and tolerances of tests/test_attention_window_gpu.py::test_window_mistral_hip_matches_cpu_reference;
    the two batch rows have different boundaries."""
    torch.manual_seed(0)
    cfg = _doc_model_cfg()
    m_cpu = build_model(cfg)
    m_gpu = copy.deepcopy(m_cpu).to("cuda", torch.bfloat16)
    m_cpu.rt, m_gpu.rt = ParamRuntime(), ParamRuntime()
    idx = tokens(256, [[40, 41, 130, 200], [63, 64, 191]], seed=3)
    tgt = idx.roll(-1, 1)
    _, l_cpu = m_cpu(idx, tgt)
    _, l_gpu = m_gpu(idx.cuda(), tgt.cuda())
    assert math.isfinite(l_gpu.item())
    assert abs(l_cpu.item() - l_gpu.item()) < 1e-2 * abs(l_cpu.item())
    l_cpu.backward()
    l_gpu.backward()
    gp = dict(m_gpu.named_parameters())
    for n, p in m_cpu.named_parameters():
        assert torch.isfinite(gp[n].grad).all(), n
        r = rel(gp[n].grad, p.grad)
        assert r < 6e-2, (n, r)


def test_docmask_mistral_zero3_step():
    torch.manual_seed(0)
    cfg = _doc_model_cfg()
    with torch.device("cuda"):
        model = build_model(cfg)
    eng = make_engine(model, engine_config("zero3", 1, "reference"), "cuda:0")
    eng.train()
    idx = tokens(256, [[17, 100, 101, 229]], seed=4).cuda()
    loss = eng(idx, idx.roll(-1, 1))[1]
    eng.backward(loss)
    eng.step()
    torch.cuda.synchronize()
    assert math.isfinite(loss.item())


def _graph_engine():
    torch.manual_seed(0)
    cfg = _doc_model_cfg()
    with torch.device("cuda"):
        model = build_model(cfg)
        with torch.no_grad():           # 0.02-std weights barely attend: make the mask matter to the loss
            for p in model.parameters():
                if p.dim() == 2:
                    p.mul_(8.0)
    eng = make_engine(model, engine_config("zero3", 1, "reference"), "cuda:0")
    eng.train()
    return eng


def test_docmask_graph_replay_follows_the_tokens(monkeypatch):
    """A captured micro-step recomputes the bounds from its static idx buffer: after the capture a batch with other
    boundaries gives the loss of a twin eager engine on that batch (tolerance of tests/test_graphs_gpu.py), not
    the loss that the captured batch's boundaries would give."""
    T = 256
    batches = [tokens(T, [ends], seed=10 + i).cuda()
               for i, ends in enumerate([[50], [30, 31, 140], [30, 31, 140], [64, 200, 201, 202]])]

    def eager(stale_from=None):
        eng = _graph_engine()
        out = []
        for i, idx in enumerate(batches):
            if stale_from is not None and i == len(batches) - 1:
                import dltb.models.mistral as mm
                stale = F_.doc_bounds(batches[stale_from], EOS, 0)
                monkeypatch.setattr(mm.F_, "doc_bounds", lambda *a, **k: stale)
            loss = eng(idx, idx.roll(-1, 1))[1]
            eng.backward(loss)
            eng.step()
            out.append(loss.item())
        monkeypatch.undo()
        return out

    want = eager()
    eng = _graph_engine()
    runner = GraphedStep(eng)
    got = [runner(idx, idx.roll(-1, 1)).item() for idx in batches]
    assert not runner.disabled and len(runner.graphs) == eng.accum      # batches 1.. were replays
    for a, b in zip(got, want):
        assert math.isfinite(a) and abs(a - b) < 1e-3 * abs(b), (got, want)
    stale = eager(stale_from=1)[-1]      # the last batch under the boundaries of the batch the capture saw
    assert got[-1] != stale
    assert abs(got[-1] - stale) > abs(got[-1] - want[-1]), (got[-1], want[-1], stale)
