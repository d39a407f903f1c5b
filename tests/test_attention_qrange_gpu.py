"""Query-range attention kernels (``q_range = (q_begin, q_end)``: the query-side tensors hold only those rows of a
length-T problem, K / V / dK / dV all T rows, every mask in global positions) on the MI355X against the fp32
reference of dltb.ops.ref with the same range, and against the existing whole-row call.

Comparison helper and tolerances: tests/test_attention_window_gpu.py (those of test_kernels_gpu.py::test_attention);
every comparison first asserts that the kernel output is finite.

The range kernels leave a query block's key walk untouched (same tile range, same key splits -- the dQ split count
follows T, not the range), so O, LSE and dQ of a range are compared BITWISE with the same rows of the whole-row call.
"""
import functools
import math

import pytest
import torch

import dltb
from dltb.data import SyntheticDataset
from dltb.ops import functional as F_
from dltb.ops import ref
from dltb.ops._ext import ext
from dltb.ops.rng import StepSeed

pytestmark = pytest.mark.gpu
DEV = "cuda"
SITE = 11
B, T = 2, 512
SHAPES = [(2, 1, 64), (4, 2, 128)]
# the three ranks of an uneven split, the second half, and the zigzag pair of a middle rank (cp = 2: chunks 1 and 2)
RANGES = [(0, 128), (128, 384), (384, 512), (256, 512), (128, 256), (256, 384)]
PARTITIONS = [[(0, 128), (128, 384), (384, 512)], [(0, 128), (128, 256), (256, 384), (384, 512)]]
# plain causal; windows that straddle a 64-key tile (96) and a 128-row block (200); packed documents
MASKS = ["causal", "w96", "w200", "doc"]


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


@functools.lru_cache(maxsize=None)
def mask_args(mask, B, T):
    """(window, bounds) of a mask name; the document bounds come from a seeded packed table."""
    if mask == "causal":
        return 0, None
    if mask.startswith("w"):
        return int(mask[1:]), None
    ds = SyntheticDataset(256, T, size=B, seed=7, doc_len=96)
    idx = ds.data[:B].to(DEV)
    return 0, F_.doc_bounds(idx, ds.eos_id, 0)


def rows(x, B, T, qb, qe):
    """Rows qb .. qe - 1 of every batch row of a [B * T, C] tensor, as a contiguous [B * (qe - qb), C] tensor."""
    return x.view(B, T, -1)[:, qb:qe].reshape(B * (qe - qb), -1).contiguous()


def run_range(qkv, do, B, T, Hq, Hkv, D, window, bounds, rng, fused=True):
    """(o, lse, dq, dk, dv) of the HIP kernels for one range (None: the existing whole-row call)."""
    C = ext()
    q, k, v = split(qkv, Hq, Hkv, D)
    scale = 1.0 / math.sqrt(D)
    if rng is not None:
        q, do = rows(q, B, T, *rng), rows(do, B, T, *rng)
    kw = {} if rng is None else {"q_range": rng}
    o, lse = C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, window=window, bounds=bounds, **kw)
    dq = torch.full_like(q, float("nan"))               # every element must be written
    dk = torch.full_like(k, float("nan")).contiguous()
    dv = torch.full_like(v, float("nan")).contiguous()
    if fused:
        F_.attn_bwd(q, k, v, o, do, lse, None, dq, dk, dv, B, T, Hq, Hkv, scale, True, 0.0, seed_obj(), SITE,
                    window=window, bounds=bounds, **kw)
    else:
        C.attn_bwd(q, k, v, o, do, lse, None, dq, dk, dv, B, T, Hq, Hkv, scale, True, 0.0, window=window,
                   bounds=bounds, **kw)
    return o, lse, dq, dk, dv


@functools.lru_cache(maxsize=None)
def full_call(B, T, Hq, Hkv, D, mask, dtype=torch.bfloat16):
    qkv, do = inputs(B, T, Hq, Hkv, D, dtype)
    window, bounds = mask_args(mask, B, T)
    return run_range(qkv, do, B, T, Hq, Hkv, D, window, bounds, None)


def check_range(B, T, Hq, Hkv, D, mask, rng, dtype=torch.bfloat16, fused=True):
    qkv, do = inputs(B, T, Hq, Hkv, D, dtype)
    window, bounds = mask_args(mask, B, T)
    q, k, v = split(qkv, Hq, Hkv, D)
    scale = 1.0 / math.sqrt(D)
    qb, qe = rng
    o, lse, dq, dk, dv = run_range(qkv, do, B, T, Hq, Hkv, D, window, bounds, rng, fused)
    assert o.dtype == dtype and o.shape == (B * (qe - qb), Hq * D) and lse.shape == (B, Hq, qe - qb)
    for name, x in zip(("o", "lse", "dq", "dk", "dv"), (o, lse, dq, dk, dv)):
        assert torch.isfinite(x).all(), f"{name}: non-finite values in the kernel output"
    # the fp32 reference with the same range
    ql, dol = rows(q, B, T, qb, qe), rows(do, B, T, qb, qe)
    sd = seed_obj()
    ro, rlse = ref.attn_fwd(ql, k, v, B, T, Hq, Hkv, scale, True, 0.0, sd, SITE, window=window, bounds=bounds,
                            q_range=rng)
    close(lse, rlse, 8e-3, 1e-3, "lse")
    close(o, ro, 2e-2, 3e-2, "O")
    rdq, rdk, rdv = torch.empty_like(dq), torch.empty_like(dk), torch.empty_like(dv)
    ref.attn_bwd(ql, k, v, o, dol, lse, rdq, rdk, rdv, B, T, Hq, Hkv, scale, True, 0.0, sd, SITE, window=window,
                 bounds=bounds, q_range=rng)
    for name, a, b in zip("qkv", (dq, dk, dv), (rdq, rdk, rdv)):
        close(a, b, 5e-2, 5e-2, "d" + name)
    # no query of the range sees a key at or past q_end: exact zeros
    for name, x in (("dk", dk), ("dv", dv)):
        tail = x.view(B, T, -1)[:, qe:]
        assert torch.equal(tail, torch.zeros_like(tail)), f"{name}: rows beyond the range's last query are not zero"
    return o, lse, dq, dk, dv


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_qrange_against_ref_and_full_call(Hq, Hkv, D, mask):
    fo, flse, fdq, fdk, fdv = full_call(B, T, Hq, Hkv, D, mask)
    got = {}
    for rng in RANGES:
        qb, qe = rng
        o, lse, dq, dk, dv = got[rng] = check_range(B, T, Hq, Hkv, D, mask, rng)
        # the block's key walk is untouched: bitwise the same rows of the whole-row call
        assert torch.equal(o, rows(fo, B, T, qb, qe)), f"O {rng}"
        assert torch.equal(lse, flse[..., qb:qe]), f"lse {rng}"
        assert torch.equal(dq, rows(fdq, B, T, qb, qe)), f"dQ {rng}"
    for part in PARTITIONS:     # dK / dV summed over a partition of [0, T) match the whole-row call
        sk = sum(got[r][3].float() for r in part)
        sv = sum(got[r][4].float() for r in part)
        close(sk, fdk, 5e-2, 5e-2, f"sum dK {part}")
        close(sv, fdv, 5e-2, 5e-2, f"sum dV {part}")


@pytest.mark.parametrize("mask", ["causal", "w200"])
def test_qrange_unfused_delta(mask):
    """The extension's own attn_bwd (delta kernel over the range's rows, then dK/dV, then dQ)."""
    check_range(B, T, 4, 2, 128, mask, (128, 384), fused=False)


@pytest.mark.parametrize("mask", ["causal", "w96", "doc"])
def test_qrange_long_t_d64_dq_splits(mask):
    """D = 64 from T = 1024: the causal and windowed dQ pass runs three key splits, every split more than one
    round deep for the range's last blocks; one head per KV head, so dK / dV take the unsplit (bf16 store) path."""
    Bl, Tl, Hq, Hkv, D, rng = 1, 1024, 4, 4, 64, (640, 1024)
    fo, flse, fdq, _, _ = full_call(Bl, Tl, Hq, Hkv, D, mask)
    o, lse, dq, _, _ = check_range(Bl, Tl, Hq, Hkv, D, mask, rng)
    assert torch.equal(o, rows(fo, Bl, Tl, *rng))
    assert torch.equal(lse, flse[..., rng[0]:rng[1]])
    assert torch.equal(dq, rows(fdq, Bl, Tl, *rng))


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_qrange_whole_row_is_bitwise_existing_call(Hq, Hkv, D, mask):
    qkv, do = inputs(B, T, Hq, Hkv, D)
    window, bounds = mask_args(mask, B, T)
    base = full_call(B, T, Hq, Hkv, D, mask)
    got = run_range(qkv, do, B, T, Hq, Hkv, D, window, bounds, (0, T))
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), got, base):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), name


def test_qrange_whole_row_with_dropout_allowed():
    """(0, T) is the square problem: dropout stays allowed and the result is the existing call's."""
    C = ext()
    Hq, Hkv, D, p = 2, 1, 64, 0.1
    qkv, do = inputs(B, T, Hq, Hkv, D)
    q, k, v = split(qkv, Hq, Hkv, D)
    sd = seed_obj()
    m = C.attn_mask(B, T, Hq, p, sd.device_tensor, SITE, q)
    o0, l0 = C.attn_fwd(q, k, v, m, B, T, Hq, Hkv, 0.125, True, p)
    o1, l1 = C.attn_fwd(q, k, v, m, B, T, Hq, Hkv, 0.125, True, p, q_range=(0, T))
    assert torch.equal(o0, o1) and torch.equal(l0, l1)


def test_qrange_refusals():
    C = ext()
    Hq, Hkv, D = 2, 1, 64
    qkv, do = inputs(B, T, Hq, Hkv, D)
    q, k, v = split(qkv, Hq, Hkv, D)
    scale = 1.0 / math.sqrt(D)
    ql, dol = rows(q, B, T, 128, 384), rows(do, B, T, 128, 384)
    o, lse = C.attn_fwd(ql, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, q_range=(128, 384))
    dq, dk, dv = torch.empty_like(ql), torch.empty_like(k).contiguous(), torch.empty_like(v).contiguous()
    sd = seed_obj()
    m = C.attn_mask(B, T, Hq, 0.1, sd.device_tensor, SITE, q)
    with pytest.raises(RuntimeError, match="dropout"):
        C.attn_fwd(ql, k, v, m, B, T, Hq, Hkv, scale, True, 0.1, q_range=(128, 384))
    with pytest.raises(RuntimeError, match="dropout"):
        C.attn_bwd(ql, k, v, o, dol, lse, m, dq, dk, dv, B, T, Hq, Hkv, scale, True, 0.1, q_range=(128, 384))
    with pytest.raises(ValueError, match="dropout"):
        F_.attn_fwd(ql, k, v, B, T, Hq, Hkv, scale, True, 0.1, sd, SITE, q_range=(128, 384))
    with pytest.raises(RuntimeError, match="causal"):
        C.attn_fwd(ql, k, v, None, B, T, Hq, Hkv, scale, False, 0.0, q_range=(128, 384))
    with pytest.raises(RuntimeError, match="causal"):
        C.attn_bwd_part(1, ql, k, v, dol, lse, torch.empty_like(lse), None, dq, None, B, T, Hq, Hkv, scale, False,
                        0.0, q_range=(128, 384))
    with pytest.raises(ValueError, match="causal"):
        F_.attn_bwd(ql, k, v, o, dol, lse, None, dq, dk, dv, B, T, Hq, Hkv, scale, False, 0.0, sd, SITE,
                    q_range=(128, 384))
    for bad in [(64, 384), (128, 320), (100, 228)]:
        with pytest.raises(RuntimeError, match="multiples of 128"):
            C.attn_fwd(ql, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, q_range=bad)
        with pytest.raises(ValueError, match="multiples of 128"):
            F_.attn_fwd(ql, k, v, B, T, Hq, Hkv, scale, True, 0.0, sd, SITE, q_range=bad)
    for bad in [(128, 128), (384, 128), (-128, 128), (384, 640)]:
        with pytest.raises(RuntimeError, match="begin < end"):
            C.attn_fwd(ql, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, q_range=bad)
        with pytest.raises(ValueError, match="begin < end"):
            F_.attn_fwd(ql, k, v, B, T, Hq, Hkv, scale, True, 0.0, sd, SITE, q_range=bad)
    with pytest.raises(RuntimeError, match="shape"):      # q must hold the range's rows only
        C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, q_range=(128, 384))
    torch.cuda.synchronize()


def test_qrange_fp16_build():
    """fp16 tensors select the fp16 objects of the same kernels (tests/test_fp16_gpu.py)."""
    fo, flse, fdq, _, _ = full_call(B, T, 4, 2, 128, "w96", torch.float16)
    o, lse, dq, _, _ = check_range(B, T, 4, 2, 128, "w96", (128, 384), dtype=torch.float16)
    assert torch.equal(o, rows(fo, B, T, 128, 384)) and torch.equal(dq, rows(fdq, B, T, 128, 384))
