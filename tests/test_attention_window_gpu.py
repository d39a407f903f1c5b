"""Sliding-window causal attention kernels (``window = W``: query i sees key j iff ``i - W < j <= i``)
on the MI355X against the fp32 reference of dltb.ops.ref, which shares the dropout hash with the kernels.

Every comparison first asserts that the kernel output is finite: ``err > tol`` is false for NaN, and a
NaN (a fully masked row in a lower-edge tile, an empty key split) is the failure a window is most likely
to produce.
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
from dltb.parallel import ParamRuntime, engine_config, make_engine

pytestmark = pytest.mark.gpu
DEV = "cuda"
SITE = 11


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


def run_kernels(qkv, do, B, T, Hq, Hkv, D, p, window, sd, fused, causal=True):
    """(o, lse, dq, dk, dv) of the HIP kernels; ``fused``: the model's path (dQ pass forms delta itself)."""
    C = ext()
    q, k, v = split(qkv, Hq, Hkv, D)
    scale = 1.0 / math.sqrt(D)
    amask = C.attn_mask(B, T, Hq, p, sd.device_tensor, SITE, q) if p else None
    o, lse = C.attn_fwd(q, k, v, amask, B, T, Hq, Hkv, scale, causal, p, window=window)
    dqkv = torch.full_like(qkv, float("nan"))          # every element must be written
    if fused:
        F_.attn_bwd(q, k, v, o, do, lse, amask, *split(dqkv, Hq, Hkv, D), B, T, Hq, Hkv, scale, causal, p, sd, SITE,
                    window=window)
    else:
        C.attn_bwd(q, k, v, o, do, lse, amask, *split(dqkv, Hq, Hkv, D), B, T, Hq, Hkv, scale, causal, p,
                   window=window)
    return (o, lse) + split(dqkv, Hq, Hkv, D)


def check_against_ref(B, T, Hq, Hkv, D, p, window, dtype=torch.bfloat16):
    qkv, do = inputs(B, T, Hq, Hkv, D, dtype)
    q, k, v = split(qkv, Hq, Hkv, D)
    scale = 1.0 / math.sqrt(D)
    sd = seed_obj()
    o, lse, dq, dk, dv = run_kernels(qkv, do, B, T, Hq, Hkv, D, p, window, sd, fused=False)
    assert o.dtype == dtype
    ro, rlse = ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, p, sd, SITE, window=window)
    # tolerances of test_kernels_gpu.py::test_attention for the same quantities
    close(lse, rlse, 8e-3, 1e-3, "lse")
    close(o, ro, 2e-2, 3e-2, "O")
    rdqkv = torch.empty_like(qkv)
    ref.attn_bwd(q, k, v, o, do, lse, *split(rdqkv, Hq, Hkv, D), B, T, Hq, Hkv, scale, True, p, sd, SITE,
                 window=window)
    for name, a, b in zip("qkv", (dq, dk, dv), split(rdqkv, Hq, Hkv, D)):
        close(a, b, 5e-2, 5e-2, "d" + name)
    fo, flse, fdq, fdk, fdv = run_kernels(qkv, do, B, T, Hq, Hkv, D, p, window, sd, fused=True)
    for name, a, b in zip("qkv", (fdq, fdk, fdv), split(rdqkv, Hq, Hkv, D)):
        close(a, b, 5e-2, 5e-2, "fused-delta d" + name)


# T = 512 is four query blocks of 128 and eight key tiles of 64.  The widths reach: one visible key (1);
# a band inside one tile and across one, two and three tile edges (31 .. 129); lower-edge tiles that are
# fully masked for the later rows of a wave (every W that is not a multiple of 64, and W < 32 for whole
# waves); key splits with no tile at all (W <= 65 leaves two or three tiles for the three D = 64 forward
# splits); three and more visible tiles (192, 200) and the widest band that is not plain causal (511).
WINDOWS = [1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 192, 200, 511]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("Hq,Hkv,D", [(2, 2, 64), (8, 2, 128)])      # (8, 2, 128): the head-split dK/dV path
@pytest.mark.parametrize("window", WINDOWS)
def test_window_edge_sweep(window, Hq, Hkv, D, p):
    check_against_ref(2, 512, Hq, Hkv, D, p, window)


@pytest.mark.parametrize("p", [0.1, 0.0])
def test_window_long_t_d64_dq(p):
    """Causal D = 64 from T = 1024: the causal dQ pass goes to three key splits there.  The windowed pass
    does so without dropout; with dropout it stays at two (three would spill, csrc/attention.hip launch_dq)."""
    check_against_ref(1, 1024, 4, 4, 64, p, 100)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("Hq,Hkv,D", [(4, 2, 64), (4, 2, 128)])
def test_window_exact_locality(Hq, Hkv, D, p):
    """Keys j <= i0 - W are outside the window of every row i >= i0: replacing them changes no bit of
    those rows (skipped tiles, exact p = 0), while row i0 - 1 still sees key i0 - W."""
    B, T, W, i0 = 1, 512, 100, 300
    qkv, do = inputs(B, T, Hq, Hkv, D)
    sd = seed_obj()
    o, lse, dq, _, _ = run_kernels(qkv, do, B, T, Hq, Hkv, D, p, W, sd, fused=False)
    qkv2 = qkv.clone()
    g = torch.Generator(device=DEV).manual_seed(5)
    fresh = torch.randn(i0 - W + 1, 2 * Hkv * D, device=DEV, generator=g).to(qkv.dtype)
    qkv2[:i0 - W + 1, Hq * D:] = fresh                     # K and V rows 0 .. i0 - W (B = 1)
    o2, lse2, dq2, _, _ = run_kernels(qkv2, do, B, T, Hq, Hkv, D, p, W, sd, fused=False)
    for x in (o, lse, dq, o2, lse2, dq2):
        assert torch.isfinite(x).all()
    assert torch.equal(o[i0:], o2[i0:])
    assert torch.equal(lse[..., i0:], lse2[..., i0:])
    assert torch.equal(dq[i0:], dq2[i0:])
    assert not torch.equal(o[i0 - 1], o2[i0 - 1])


@pytest.mark.parametrize("window", [512, 4096])
@pytest.mark.parametrize("Hq,Hkv,D", [(2, 2, 64), (8, 2, 128)])
def test_window_of_t_or_more_is_bitwise_causal(window, Hq, Hkv, D):
    B, T, p = 2, 512, 0.1
    qkv, do = inputs(B, T, Hq, Hkv, D)
    sd = seed_obj()
    base = run_kernels(qkv, do, B, T, Hq, Hkv, D, p, 0, sd, fused=False)
    got = run_kernels(qkv, do, B, T, Hq, Hkv, D, p, window, sd, fused=False)
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), got, base):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), name


def test_window_refusals():
    C = ext()
    B, T, Hq, Hkv, D = 2, 512, 2, 2, 64
    qkv, do = inputs(B, T, Hq, Hkv, D)
    q, k, v = split(qkv, Hq, Hkv, D)
    scale = 1.0 / math.sqrt(D)
    o, lse = C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, False, 0.0)
    g = split(torch.empty_like(qkv), Hq, Hkv, D)
    delta = torch.empty_like(lse)
    with pytest.raises(RuntimeError, match="causal"):
        C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, False, 0.0, window=64)
    with pytest.raises(RuntimeError, match="causal"):
        C.attn_bwd(q, k, v, o, do, lse, None, *g, B, T, Hq, Hkv, scale, False, 0.0, window=64)
    with pytest.raises(RuntimeError, match="causal"):
        C.attn_bwd_part(1, q, k, v, do, lse, delta, None, g[0], None, B, T, Hq, Hkv, scale, False, 0.0, window=64)
    with pytest.raises(RuntimeError, match=">= 0"):
        C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, window=-1)
    with pytest.raises(RuntimeError, match=">= 0"):
        C.attn_bwd(q, k, v, o, do, lse, None, *g, B, T, Hq, Hkv, scale, True, 0.0, window=-1)
    with pytest.raises(ValueError, match="causal"):
        F_.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, False, 0.0, seed_obj(), SITE, window=64)
    torch.cuda.synchronize()


def test_window_fp16_build():
    """fp16 tensors select the fp16 objects of the same kernels (tests/test_fp16_gpu.py)."""
    check_against_ref(2, 512, 8, 2, 128, 0.1, 65, dtype=torch.float16)


def _window_model_cfg():
    cfg = get_model_config("mtiny", 256)
    cfg.sliding_window = 64
    cfg.validate()
    return cfg


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


def test_window_mistral_hip_matches_cpu_reference():
    """Method and tolerances of tests/test_mistral_gpu.py::test_mistral_hip_matches_cpu_reference."""
    torch.manual_seed(0)
    cfg = _window_model_cfg()
    m_cpu = build_model(cfg)
    m_gpu = copy.deepcopy(m_cpu).to("cuda", torch.bfloat16)
    m_cpu.rt, m_gpu.rt = ParamRuntime(), ParamRuntime()
    idx = torch.randint(0, cfg.vocab_size, (2, 256))
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


def test_window_mistral_zero3_step():
    torch.manual_seed(0)
    cfg = _window_model_cfg()
    with torch.device("cuda"):
        model = build_model(cfg)
    eng = make_engine(model, engine_config("zero3", 1, "reference"), "cuda:0")
    eng.train()
    idx = torch.randint(0, cfg.vocab_size, (1, 256), device="cuda")
    loss = eng(idx, idx.roll(-1, 1))[1]
    eng.backward(loss)
    eng.step()
    torch.cuda.synchronize()
    assert math.isfinite(loss.item())
