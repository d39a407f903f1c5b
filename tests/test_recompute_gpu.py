"""Activation recomputation (``--activation-recompute``) on the MI355X.

The two new kernels against the launches they replace, bit for bit (they evaluate the same fp32 expressions on
the same inputs and round once, like them); then the Mistral-shape model, the sharded engines, HIP-graph replay
and context parallelism under ``selective`` / ``full`` against ``off``.  A re-run forward uses the forward's own
kernels on the forward's own inputs and all randomness is hash-seeded, so wherever two ``off`` runs agree bit for
bit (tests/test_graphs_gpu.py::test_graph_replay_mistral relies on that) a recompute run must agree with them bit
for bit too; should a library GEMM ever reduce in a run-dependent order, the fallback is the tolerance
tests/test_mistral_gpu.py holds the same model to against the CPU reference (1e-2 loss, 6e-2 gradients)."""
import copy

import pytest
import torch

import dltb
from dltb.models import build_model, get_model_config
from dltb.ops import functional as F_
from dltb.ops._ext import ext
from dltb.parallel import GraphedStep, ParamRuntime, engine_config, make_engine
from multirank_util import compare, run

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
MODES = ["selective", "full"]


def _rand(*shape, dtype, scale=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, device="cuda", generator=g) * scale).to(dtype)


# ------------------------------------------------------------------------------------------- swiglu_bwd_h
# (1, 8): one vector; (3, 1032): F no multiple of a wave's 512 columns; (257, 1024): an odd row count over several
# blocks; (128, 14336): the Mistral-7B width; (300, 14336): 537 600 vectors, more than the 2048 x 256 threads of one
# grid pass, so the grid-stride loop runs a second, partial pass
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("N,F", [(1, 8), (3, 1032), (257, 1024), (128, 14336), (300, 14336)])
def test_swiglu_bwd_h_is_the_two_kernels(N, F, dtype):
    C = ext()
    gu = _rand(N, 2 * F, dtype=dtype, scale=6.0, seed=1)            # |gate| up to ~20 and beyond: sigmoid saturates
    gu[0, :8] = torch.tensor([-30.0, -20.0, -8.0, -0.0, 0.0, 8.0, 20.0, 30.0], device="cuda").to(dtype)
    dh = _rand(N, F, dtype=dtype, seed=2)
    assert gu[:, :F].abs().max().item() >= 20.0
    dgu, h = F_.swiglu_bwd_h(dh, gu)
    assert h.shape == (N, F) and dgu.shape == (N, 2 * F) and h.dtype == dgu.dtype == dtype
    assert torch.equal(h, C.swiglu_fwd(gu))
    assert torch.equal(dgu, C.swiglu_bwd(dh, gu))
    assert torch.isfinite(h.float()).all() and torch.isfinite(dgu.float()).all()


def test_swiglu_bwd_h_refuses_bad_operands():
    C = ext()
    gu, dh = _rand(4, 32, dtype=torch.bfloat16), _rand(4, 16, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        C.swiglu_bwd_h(dh[:, :8], gu)                                  # not contiguous / wrong width
    with pytest.raises(RuntimeError):
        C.swiglu_bwd_h(_rand(4, 8, dtype=torch.bfloat16), gu)
    with pytest.raises(RuntimeError):
        C.swiglu_bwd_h(dh.half(), gu)                                  # one 16-bit format per call


# ------------------------------------------------------------------------------------------- norm_apply
# every NV instantiation of norm_fwd (csrc/norm.hip nv_for: 1, 2, 3, 4, 6, 8 vectors per lane; 5 and 7 round up)
# with a partly filled last vector group, mtiny's 128, TinyGPT's 1024 and Mistral-7B's 4096
NORM_D = [8, 128, 512, 520, 1024, 1536, 2048, 2560, 3072, 3584, 4096]


def _norm_case(N, d, rms, dtype, res):
    x = _rand(N, d, dtype=dtype, scale=2.0, seed=3) + 0.5
    r = _rand(N, d, dtype=dtype, seed=4) if res else None
    w = (1 + 0.2 * _rand(d, dtype=torch.float32, seed=5)).to(dtype)
    b = None if rms else (0.3 * _rand(d, dtype=torch.float32, seed=6)).to(dtype)
    s, y, mean, rstd = F_.norm_fwd(x, r, w, b, 1e-5, rms)
    return (s if res else x), w, b, mean, rstd, y


@pytest.mark.parametrize("d", NORM_D)
@pytest.mark.parametrize("rms", [True, False], ids=["rms_nobias", "ln_bias"])
def test_norm_apply_is_norm_fwd_y(rms, d):
    """RMSNorm has no bias (norm_fwd ignores b) and LayerNorm needs one: those are the two bias cases.  Both with
    and without the fused residual add, whose rounded sum is the s that norm_apply reads."""
    for N in (1, 5, 300):
        for res in (False, True):
            s, w, b, mean, rstd, y = _norm_case(N, d, rms, torch.bfloat16, res)
            got = F_.norm_apply(s, w, b, mean, rstd, rms)
            assert got.shape == y.shape and torch.equal(got, y), (N, res)


@pytest.mark.parametrize("rms", [True, False], ids=["rms", "ln"])
def test_norm_apply_fp16_and_3d(rms):
    s, w, b, mean, rstd, y = _norm_case(300, 1024, rms, torch.float16, True)
    assert torch.equal(F_.norm_apply(s, w, b, mean, rstd, rms), y)
    assert torch.equal(F_.norm_apply(s.view(3, 100, 1024), w, b, mean, rstd, rms), y.view(3, 100, 1024))


def test_norm_apply_strided_y_out():
    s, w, b, mean, rstd, y = _norm_case(300, 128, True, torch.bfloat16, False)
    buf = torch.full((300, 3 * 128), 7.0, device="cuda", dtype=torch.bfloat16)
    out = buf[:, 128:256]                                              # a column block: row stride 384
    got = F_.norm_apply(s, w, b, mean, rstd, True, y_out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(out, y)
    assert (buf[:, :128] == 7.0).all() and (buf[:, 256:] == 7.0).all()    # nothing beside the view was written


def test_norm_apply_refuses_bad_operands():
    C = ext()
    s, w, b, mean, rstd, y = _norm_case(5, 128, False, torch.bfloat16, False)
    with pytest.raises(RuntimeError):
        C.norm_apply(s, w, None, mean, rstd, False)                   # LayerNorm without its bias
    with pytest.raises(RuntimeError):
        C.norm_apply(s, w, b, None, rstd, False)                      # ... or its means
    with pytest.raises(RuntimeError):
        C.norm_apply(s, w, b, mean, rstd[:4], False)                  # one statistic per row
    with pytest.raises(RuntimeError):
        C.norm_apply(s, w[:64], b, mean, rstd, False)
    with pytest.raises(RuntimeError):
        C.norm_apply(s, w, b, mean, rstd, False, torch.empty(5, 136, device="cuda", dtype=torch.bfloat16)[:, 4:132])
    with pytest.raises(RuntimeError):
        C.norm_apply(s, w, b, mean, rstd, False, torch.empty(4, 128, device="cuda", dtype=torch.bfloat16))


# ------------------------------------------------------------------------------------------- model
def _m7b_slice(T=256, layers=2):
    """Full Mistral-7B width (d4096, 32q/8kv heads x 128, ffn 14336) with fewer layers."""
    c = get_model_config("M7B", T)
    c.n_layer = layers
    return c


def _model_cfg(kind):
    if kind == "m7b":
        return _m7b_slice(256, 1)
    cfg = get_model_config("mtiny", 256)
    cfg.n_layer = 2
    if kind == "mtiny_window_doc":
        cfg.sliding_window = 96
        cfg.doc_eos_id = cfg.vocab_size - 1
        cfg.validate()
    return cfg


def _batch(cfg):
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, cfg.vocab_size, (2, 256), generator=g)
    if cfg.doc_eos_id is not None:
        idx[:, [40, 41, 130, 255]] = cfg.doc_eos_id
    return idx, idx.roll(-1, 1)


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


class _ModelRuns:
    """One initialisation per model kind; every run starts from a copy of it.  The two ``off`` runs and, only if
    they disagree, the CPU reference are computed once and shared."""

    def __init__(self):
        self.cache = {}

    def base(self, kind):
        if ("base", kind) not in self.cache:
            torch.manual_seed(0)
            cfg = _model_cfg(kind)
            self.cache[("base", kind)] = (cfg, build_model(cfg))
        return self.cache[("base", kind)]

    def gpu(self, kind, mode, tag=0):
        key = (kind, mode, tag)
        if key not in self.cache:
            cfg, m_cpu = self.base(kind)
            if ("gpu_base", kind) not in self.cache:
                self.cache[("gpu_base", kind)] = copy.deepcopy(m_cpu).to("cuda", torch.bfloat16)
            m = copy.deepcopy(self.cache[("gpu_base", kind)])
            m.rt = ParamRuntime()
            m.activation_recompute = mode
            idx, tgt = _batch(cfg)
            _, loss = m(idx.cuda(), tgt.cuda())
            loss.backward()
            torch.cuda.synchronize()
            self.cache[key] = (loss.detach(), {n: p.grad for n, p in m.named_parameters()})
        return self.cache[key]

    def cpu(self, kind):
        if ("cpu", kind) not in self.cache:
            cfg, m_cpu = self.base(kind)
            m = copy.deepcopy(m_cpu)
            m.rt = ParamRuntime()
            idx, tgt = _batch(cfg)
            _, loss = m(idx, tgt)
            loss.backward()
            self.cache[("cpu", kind)] = (loss.detach(), {n: p.grad for n, p in m.named_parameters()})
        return self.cache[("cpu", kind)]

    def deterministic(self, kind):
        (l0, g0), (l1, g1) = self.gpu(kind, "off", 0), self.gpu(kind, "off", 1)
        return torch.equal(l0, l1) and all(torch.equal(g0[n], g1[n]) for n in g0)


@pytest.fixture(scope="module")
def model_runs():
    return _ModelRuns()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["mtiny", "mtiny_window_doc", "m7b"])
def test_model_recompute_equals_off(model_runs, kind, mode):
    loss, grads = model_runs.gpu(kind, mode)
    if model_runs.deterministic(kind):
        l0, g0 = model_runs.gpu(kind, "off", 0)
        assert torch.equal(loss, l0), (loss.item(), l0.item())
        for n in g0:
            assert torch.equal(grads[n], g0[n]), n
    else:
        l_cpu, g_cpu = model_runs.cpu(kind)
        assert abs(l_cpu.item() - loss.item()) < 1e-2 * abs(l_cpu.item())
        for n, g in g_cpu.items():
            r = rel(grads[n], g)
            assert r < 6e-2, (n, r)


# ------------------------------------------------------------------------------------------- engines
def _engine_run(strategy, mode, graphed=False, tier="m7b"):
    """test_mistral_engine_steps' model (tier m7b) or test_graph_replay_mistral's (mtiny): a 2-micro-step
    accumulation window (4 for the graph test, like its original), six steps (16)."""
    torch.manual_seed(0)
    if tier == "m7b":
        cfg, T, accum, steps = _m7b_slice(512, 2), 512, 2, 6
    else:
        cfg, T, accum, steps = get_model_config("mtiny", 256), 256, 4, 16
        cfg.n_layer = 2
    with torch.device("cuda"):
        model = build_model(cfg)
    model.activation_recompute = mode
    eng = make_engine(model, engine_config(strategy, accum, "reference"), "cuda:0")
    eng.train()
    g = torch.Generator(device="cuda").manual_seed(1)
    runner = GraphedStep(eng) if graphed else None
    losses = []
    for _ in range(steps):
        idx = torch.randint(0, cfg.vocab_size, (1, T), device="cuda", generator=g)
        if runner is None:
            loss = eng(idx, idx.roll(-1, 1))[1]
            eng.backward(loss)
            eng.step()
        else:
            loss = runner(idx, idx.roll(-1, 1))
        losses.append(loss.item())
    if runner is not None:
        assert len(runner.graphs) == eng.accum
    sd = {k: v.detach().clone() for k, v in eng.full_state_dict().items()}
    del eng, model, runner
    torch.cuda.empty_cache()
    return losses, sd


def _same(a, b):
    return a[0] == b[0] and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def _close_to(a, b):
    """The fallback when ``off`` itself is not repeatable: losses and the trained state within the model
    tolerances of tests/test_mistral_gpu.py."""
    for x, y in zip(a[0], b[0]):
        assert abs(x - y) < 1e-2 * abs(y), (a[0], b[0])
    for k in b[1]:
        assert rel(a[1][k], b[1][k]) < 6e-2, k


@pytest.mark.parametrize("strategy", ["zero3", "fsdp", "zero2"])
def test_engine_steps_full_equals_off(strategy):
    off0 = _engine_run(strategy, "off")
    full = _engine_run(strategy, "full")
    assert all(l == l for l in full[0])
    if _same(off0, full):
        return
    off1 = _engine_run(strategy, "off")        # only now: is ``off`` itself repeatable?
    assert not _same(off0, off1), "two off runs agree bit for bit and the full run differs from them"
    _close_to(full, off0)


def test_graph_replay_full_equals_eager_full():
    eager = _engine_run("zero3", "full", graphed=False, tier="mtiny")
    replay = _engine_run("zero3", "full", graphed=True, tier="mtiny")
    off = _engine_run("zero3", "off", graphed=False, tier="mtiny")
    assert eager[0] == replay[0], (eager[0], replay[0])
    for k in eager[1]:
        assert torch.equal(eager[1][k], replay[1][k]), k
    assert _same(off, eager)


# ------------------------------------------------------------------------------------------- context parallel
CP_TOL = dict(loss_tol=1e-3, upd_tol=0.02, cos_min=0.9998, param_tol=0.03)      # tests/test_context_parallel_gpu.py


def _exact(a, b):
    return all(a[c]["losses"] == b[c]["losses"] and all(torch.equal(t, b[c]["final"][n])
                                                         for n, t in a[c]["final"].items()) for c in a)


def test_world2_cp2_full_equals_off_gpu(tmp_path):
    """Two ranks on one GPU (gloo, host-staged buffers), zigzag layout and a windowed contiguous one, lazy
    collectives so the re-gather's wait is proven: ``full`` trains what ``off`` trains."""
    args = ("--seq-len", "512", "--windows", "2", "--cases", "cp_zero3,cp_zero3_window", "--context-parallel", "2")
    env = {"DLTB_COMM": "host", "DLTB_COMM_LAZY": "1"}
    off = run(tmp_path / "off.pt", 2, "cuda", extra=args, env_extra=env, timeout=300)
    full = run(tmp_path / "full.pt", 2, "cuda", extra=args + ("--activation-recompute", "full"), env_extra=env,
               timeout=300)
    assert set(off) == set(full) == {"cp_zero3", "cp_zero3_window"}
    if _exact(off, full):
        return
    off1 = run(tmp_path / "off1.pt", 2, "cuda", extra=args, env_extra=env, timeout=300)
    assert not _exact(off, off1), "two off runs agree bit for bit and the full run differs from them"
    bad = compare(off, full, **CP_TOL)
    assert not bad, bad


# ------------------------------------------------------------------------------------------- memory
def _dropped_bytes(cfg, n_tok, mode):
    """Bytes of the tensors ``mode`` does not keep, over all layers (bf16 activations, fp32 row statistics)."""
    d, f = cfg.n_embd, cfg.ffn_dim
    kvd = cfg.kv_heads * cfg.head_dim
    if mode == "selective":
        per_tok, stats = 2 * d + f, 0                                  # h1, h2, hh
    else:
        per_tok, stats = 3 * d + (d + 2 * kvd) + 2 * f + f, 2         # h1, h2, x1, qkv, gu, hh; rstd1, rstd2
    return cfg.n_layer * n_tok * (2 * per_tok + 4 * stats)


def _memory(model, idx, mode):
    model.activation_recompute = mode
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    _, loss = model(idx, idx.roll(-1, 1))
    after_fwd = torch.cuda.memory_allocated() - base
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del loss
    return after_fwd, peak


def test_saved_activation_memory():
    torch.manual_seed(0)
    cfg = get_model_config("mtiny", 256)
    cfg.n_layer = 4
    model = build_model(cfg).to("cuda", torch.bfloat16)
    model.rt = ParamRuntime()
    idx = torch.randint(0, cfg.vocab_size, (2, 256), device="cuda")
    _memory(model, idx, "off")                  # the first step allocates what stays: gradients, RoPE tables
    fwd, peak = {}, {}
    for mode in ("off", "selective", "full"):
        fwd[mode], peak[mode] = _memory(model, idx, mode)
    for mode in MODES:                           # the allocator only rounds sizes up: no margin
        assert fwd["off"] - fwd[mode] >= _dropped_bytes(cfg, idx.numel(), mode), (mode, fwd)
    assert fwd["full"] < fwd["selective"] < fwd["off"]
    assert peak["full"] < peak["off"], peak     # the rebuilt working set is one layer's; off holds all four
