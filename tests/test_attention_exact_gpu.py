"""The attention kernels of csrc/attention.hip, bit for bit, on inputs for which every rounding point is exact: the
count, selector and unit-probability probes of tests/attn_ref.py (derivations, assumptions and what each probe can
and cannot see: its docstring; the helpers' own checks: tests/test_attn_ref_cpu.py).

    count probe        C.attn_fwd with Q = 0: lse = ln l and O = acc / l inside the two derived bounds (K_O = 2,
                       K_LSE = 5, MARGIN = 2); the worst error / bound ratio of every case is printed
    selector probe     C.attn_fwd: O[i] == V[j*(i)], torch.equal
    unit probability   C.attn_bwd_part 0 and 1 on supplied lse = 0 and delta, then C.attn_bwd and F_.attn_bwd on an
                       integer o: dq, dk, dv == round16(want), torch.equal
    determinism        two runs on N(0, 1) inputs: forward, dK/dV and dQ torch.equal
    sensitivity        the kernel called with W + 1, a bounds plane shifted by one token or the neighbouring query
                       range fails the comparison against the unshifted expectation

No variant falls back from torch.equal to a bound: the soft-capped kernels stay exact at a zero score (attn_ref's
docstring, ``cap_exact``).  The exp2 / rescale path on non-degenerate scores and the accuracy on random data are
covered only by the close() tests of the other attention files.

B = 2, T = 512 (four query blocks, eight key tiles, every D = 64 key split populated), the three head shapes of
attn_ref.HEADS ((8, 2, 128) takes the head-split dK/dV path), bf16 and fp16; one causal D = 64 case at T = 1024,
B = 1 for the three-split dQ pass.  Every operand is a view inside a NaN-filled buffer, every output a view inside
a NaN-filled buffer whose padding must come back bit-identical.
"""
import functools

import pytest
import torch

import dltb  # noqa: F401
from dltb.ops import functional as F_
from dltb.ops._ext import ext
from dltb.ops.rng import StepSeed

import attn_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
FORMATS = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
HEADS = pytest.mark.parametrize("Hq,Hkv,D", A.HEADS)
ALL = pytest.mark.parametrize("name", list(A.CASES))
BWD = pytest.mark.parametrize("name", A.BWD_CASES)
B, T = 2, 512


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert ext().arch() == "gfx950"


def gen(n=0):
    return torch.Generator(device=DEV).manual_seed(4321 + n)


@functools.lru_cache(maxsize=None)
def seed_obj():
    s = StepSeed(42, 0, device=DEV)
    s.next()
    return s


@functools.lru_cache(maxsize=None)
def bounds_dev(Bn, T_, window):
    return ext().attn_doc_bounds(A.doc_tokens(A.doc_ids(Bn, T_, device=DEV)), 0, window)


def kernel_kw(name, Bn=B, T_=T, dtype=BF16, Hq=1, sel=False):
    """(keyword arguments of the bindings for a case, Tq, q0)"""
    c = A.case(name)
    kw = {}
    if c["docs"]:
        kw["bounds"] = bounds_dev(Bn, T_, c["window"])
    elif c["window"]:
        kw["window"] = c["window"]
    if c["q_range"]:
        kw["q_range"] = c["q_range"]
    if c["cap"]:
        kw["softcap"] = A.SEL_CAP if sel else A.CAP
    qb, qe = c["q_range"] or (0, T_)
    return kw, qe - qb, qb


def fwd_kw(name, kw, Hq, dtype):
    s = A.case(name)["sink"]
    return kw if s is None else dict(kw, sink=torch.full((Hq,), s, device=DEV).to(dtype))


def pv(x, dtype):
    return A.poisoned_view(A.to16(x, dtype), (3, 5), 8)[0]


def mask_of(name, Bn, T_, Hq, like):
    p = A.case(name)["p"]
    return ext().attn_mask(Bn, T_, Hq, p, seed_obj().device_tensor, A.SITE, like) if p > 0 else None


def run_fwd(name, q, k, v, Bn, T_, Hq, Hkv, D, dtype, kw):
    c = A.case(name)
    qv, kv, vv = pv(q, dtype), pv(k, dtype), pv(v, dtype)
    o, buf, snap = A.sentinel_out(q.shape[0], Hq * D, dtype, DEV, contiguous=True)
    o2, lse = ext().attn_fwd(qv, kv, vv, mask_of(name, Bn, T_, Hq, qv), Bn, T_, Hq, Hkv, A.SCALE, c["causal"], c["p"],
                             o_out=o, **kw)
    torch.cuda.synchronize()
    assert o2.data_ptr() == o.data_ptr()
    A.check_sentinel(f"{name} o", o, buf, snap)
    assert bool(torch.isfinite(lse).all())
    return o, lse


# ------------------------------------------------------------------------------ document bounds
@pytest.mark.parametrize("window", [0, 1, 65, 129])
def test_doc_bounds_kernel_follows_from_visible(window):
    vis = A.visible(B, T, True, window, A.doc_ids(B, T, device=DEV))
    want = A.bounds_of(vis)
    got = bounds_dev(B, T, window)
    assert torch.equal(got[0], want[0]), "lo plane"
    assert torch.equal(got[1], want[1]), "hi plane"


# ------------------------------------------------------------------------------ count probe
@functools.lru_cache(maxsize=4)
def count_case(name, Hq, Hkv, D, Bn=B, T_=T):
    c = A.case(name)
    _, Tq, q0 = kernel_kw(name, Bn, T_)
    vis = A.case_visible(name, Bn, T_, DEV)
    keep = A.keep_of(name, Bn, T_, Hq, seed_obj(), DEV)
    q, k, v = A.count_inputs(gen(), Bn, T_, Tq, Hq, Hkv, D)
    o, lse, _, _ = A.count_expect(v, vis, keep, c["p"], c["sink"], Bn, T_, Hq, Hkv, D)
    return (q, k, v), (o, lse)


def check_count(name, Hq, Hkv, D, dtype, Bn=B, T_=T):
    (q, k, v), (wo, wl) = count_case(name, Hq, Hkv, D, Bn, T_)
    kw = fwd_kw(name, kernel_kw(name, Bn, T_)[0], Hq, dtype)
    o, lse = run_fwd(name, q, k, v, Bn, T_, Hq, Hkv, D, dtype, kw)
    A.report(f"count {name} lse", lse, wl, A.lse_bound(wl))
    A.report(f"count {name} O", o, wo, A.o_bound(wo, dtype))
    return o, lse


@FORMATS
@HEADS
@ALL
def test_count_probe(name, Hq, Hkv, D, dtype):
    o, lse = check_count(name, Hq, Hkv, D, dtype)
    if name == "sinkneg":           # exp2 underflows: every bit as without a sink
        o0, lse0 = check_count("causal", Hq, Hkv, D, dtype)
        assert torch.equal(o.view(torch.int16), o0.view(torch.int16)) and torch.equal(lse.view(torch.int32),
                                                                                      lse0.view(torch.int32))


@FORMATS
def test_count_probe_long_row(dtype):
    check_count("causal", 2, 2, 64, dtype, 1, 1024)


# ------------------------------------------------------------------------------ selector probe
@functools.lru_cache(maxsize=4)
def selector_case(name, Hq, Hkv, D, Bn=B, T_=T):
    c = A.case(name)
    _, Tq, q0 = kernel_kw(name, Bn, T_)
    vis = A.case_visible(name, Bn, T_, DEV)
    keep = A.keep_of(name, Bn, T_, Hq, seed_obj(), DEV)
    q, k, v, tgt = A.selector_inputs(gen(1), vis, Bn, T_, Hq, Hkv, D)
    A.selector_check(q, k, vis, tgt, Bn, T_, Hq, Hkv, D, cap=A.SEL_CAP if c["cap"] else 0.0)
    return (q, k, v, tgt), A.selector_expect(v, tgt, keep, c["p"], q0, Bn, T_, Hq, Hkv, D)


def check_selector(name, Hq, Hkv, D, dtype, Bn=B, T_=T):
    (q, k, v, tgt), want = selector_case(name, Hq, Hkv, D, Bn, T_)
    kw = fwd_kw(name, kernel_kw(name, Bn, T_, sel=True)[0], Hq, dtype)
    o, _ = run_fwd(name, q, k, v, Bn, T_, Hq, Hkv, D, dtype, kw)
    assert torch.equal(o.to(F64), want), A.selector_blame(o, want, v, tgt, Bn, T_, Hq, Hkv, D)


@FORMATS
@HEADS
@ALL
def test_selector_probe(name, Hq, Hkv, D, dtype):
    check_selector(name, Hq, Hkv, D, dtype)


@FORMATS
def test_selector_probe_long_row(dtype):
    check_selector("causal", 2, 2, 64, dtype, 1, 1024)


# ------------------------------------------------------------------------------ unit-probability probe
@functools.lru_cache(maxsize=4)
def unit_case(name, variant, Hq, Hkv, D, dtype, Bn=B, T_=T):
    c = A.case(name)
    _, Tq, q0 = kernel_kw(name, Bn, T_)
    vis = A.case_visible(name, Bn, T_, DEV)
    keep = A.keep_of(name, Bn, T_, Hq, seed_obj(), DEV)
    q, k, v, do, o = A.unit_inputs(gen(2), variant, Bn, T_, Tq, Hq, Hkv, D)
    delta = A.unit_delta(do, o, Bn, Tq, Hq, D)
    return (q, k, v, do, o), delta, A.unit_expect(q, k, v, do, delta, vis, keep, c["p"], Bn, T_, Hq, Hkv, D, dtype)


def bwd_outputs(Bn, T_, Tq, Hq, Hkv, D, dtype):
    return [A.sentinel_out(r, h * D, dtype, DEV) for r, h in ((Bn * Tq, Hq), (Bn * T_, Hkv), (Bn * T_, Hkv))]


def check_bwd_outputs(what, outs, want):
    torch.cuda.synchronize()
    for nm, (view, buf, snap), w in zip(("dq", "dk", "dv"), outs, want):
        A.check_sentinel(f"{what} {nm}", view, buf, snap)
        bad = (view.to(F64) != w).nonzero()
        assert bad.numel() == 0, (f"{what} {nm}: {bad.shape[0]} of {w.numel()} elements differ; first at {bad[0].tolist()}: "
                                  f"{float(view[tuple(bad[0])])} instead of {float(w[tuple(bad[0])])}")


def check_unit(name, variant, Hq, Hkv, D, dtype, Bn=B, T_=T):
    c = A.case(name)
    C = ext()
    (q, k, v, do, o), delta, want = unit_case(name, variant, Hq, Hkv, D, dtype, Bn, T_)
    kw, Tq, q0 = kernel_kw(name, Bn, T_)
    qv, kv, vv, dov, ov = (pv(x, dtype) for x in (q, k, v, do, o))
    mask = mask_of(name, Bn, T_, Hq, qv)
    lse = torch.zeros(Bn, Hq, Tq, dtype=F32, device=DEV)
    d32 = delta.to(F32).contiguous()
    args = (Bn, T_, Hq, Hkv, A.SCALE, c["causal"], c["p"])
    # the two passes on the supplied lse and delta
    outs = bwd_outputs(Bn, T_, Tq, Hq, Hkv, D, dtype)
    C.attn_bwd_part(0, qv, kv, vv, dov, lse, d32, mask, outs[1][0], outs[2][0], *args, **kw)
    C.attn_bwd_part(1, qv, kv, vv, dov, lse, d32, mask, outs[0][0], None, *args, **kw)
    check_bwd_outputs(f"unit {name} {variant} parts", outs, want)
    # delta from the integer o: the delta kernel (C.attn_bwd), the dQ pass's fused delta (F_.attn_bwd)
    outs = bwd_outputs(Bn, T_, Tq, Hq, Hkv, D, dtype)
    C.attn_bwd(qv, kv, vv, ov, dov, lse, mask, outs[0][0], outs[1][0], outs[2][0], *args, **kw)
    check_bwd_outputs(f"unit {name} {variant} C.attn_bwd", outs, want)
    outs = bwd_outputs(Bn, T_, Tq, Hq, Hkv, D, dtype)
    fk = dict(kw)
    cap = fk.pop("softcap", 0.0)
    F_.attn_bwd(qv, kv, vv, ov, dov, lse, mask, outs[0][0], outs[1][0], outs[2][0], *args, seed_obj(), A.SITE,
                fk.get("window", 0), fk.get("bounds"), fk.get("q_range"), softcap=cap)
    check_bwd_outputs(f"unit {name} {variant} F_.attn_bwd", outs, want)
    if c["q_range"]:        # key rows no query of the range sees: exactly 0
        vis = A.case_visible(name, Bn, T_, DEV)
        unseen = ~vis.any(1).reshape(Bn * T_)
        assert bool(unseen.any()) == (name != "qr3")      # the last block alone, without a window, sees every key
        for view, _, _ in outs[1:]:
            assert bool((view[unseen] == 0).all()), "a key row no query of the range sees is not 0"


@FORMATS
@pytest.mark.parametrize("variant", ["q0", "k0"])
@HEADS
@BWD
def test_unit_probability_probe(name, variant, Hq, Hkv, D, dtype):
    check_unit(name, variant, Hq, Hkv, D, dtype)


@FORMATS
@pytest.mark.parametrize("variant", ["q0", "k0"])
def test_unit_probability_probe_long_row(variant, dtype):
    check_unit("causal", variant, 2, 2, 64, dtype, 1, 1024)


# ------------------------------------------------------------------------------ determinism
@functools.lru_cache(maxsize=None)
def random_inputs(Hq, Hkv, D, dtype):
    g = gen(3)
    mk = lambda r, h: torch.randn(r, h * D, generator=g, device=DEV).to(dtype)      # noqa: E731
    return mk(B * T, Hq), mk(B * T, Hkv), mk(B * T, Hkv), mk(B * T, Hq)


@FORMATS
@HEADS
@ALL
def test_two_runs_are_bit_identical(name, Hq, Hkv, D, dtype):
    c = A.case(name)
    C = ext()
    kw, Tq, q0 = kernel_kw(name)
    q, k, v, do = random_inputs(Hq, Hkv, D, dtype)
    if c["q_range"]:
        q, do = (x.view(B, T, -1)[:, q0:q0 + Tq].reshape(B * Tq, -1).contiguous() for x in (q, do))
    mask = mask_of(name, B, T, Hq, q)
    args = (B, T, Hq, Hkv, 1.0 / D ** 0.5, c["causal"], c["p"])
    runs = []
    for _ in range(2):
        o, lse = C.attn_fwd(q, k, v, mask, *args, **fwd_kw(name, kw, Hq, dtype))
        res = [o, lse]
        if name in A.BWD_CASES:
            dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
            C.attn_bwd(q, k, v, o, do, lse, mask, dq, dk, dv, *args, **kw)
            res += [dq, dk, dv]
        runs.append(res)
    torch.cuda.synchronize()
    for nm, a, b in zip(("o", "lse", "dq", "dk", "dv"), *runs):
        assert bool(torch.isfinite(a).all()), nm
        assert torch.equal(a, b), f"{name} {nm}: two runs differ"


# ------------------------------------------------------------------------------ sensitivity on the device
def count_rejected(name, kw, Hq=4, Hkv=2, D=64, dtype=BF16):
    """The count probe's comparison rejects the kernel's result under the (altered) arguments ``kw``."""
    (q, k, v), (wo, wl) = count_case(name, Hq, Hkv, D)
    o, lse = run_fwd(name, q, k, v, B, T, Hq, Hkv, D, dtype, kw)
    if o.shape != wo.shape:
        return True
    return A.flagged(lse, wl, A.lse_bound(wl)) > 0 or A.flagged(o, wo, A.o_bound(wo, dtype)) > 0


@pytest.mark.parametrize("name", ["w63", "w64", "w65", "w129"])
def test_window_plus_one_fails_the_count_probe(name):
    kw = kernel_kw(name)[0]
    assert not count_rejected(name, kw)
    assert count_rejected(name, dict(kw, window=kw["window"] + 1))


def shifted_bounds(bounds):
    """Both planes one token late / early, still monotone and with lo[i] <= i < hi[i]: lo'[i] = lo[i - 1] (0 at
    i = 0), hi'[j] = hi[j + 1] (T at the last key)."""
    lo, hi = bounds[0], bounds[1]
    lo2 = torch.cat([torch.zeros_like(lo[:, :1]), lo[:, :-1]], 1)
    hi2 = torch.cat([hi[:, 1:], torch.full_like(hi[:, :1], bounds.shape[2])], 1)
    i = torch.arange(bounds.shape[2], device=bounds.device, dtype=torch.int32)
    assert bool((lo2 <= i).all()) and bool((hi2 > i).all())
    assert bool((lo2[:, 1:] >= lo2[:, :-1]).all()) and bool((hi2[:, 1:] >= hi2[:, :-1]).all())
    return torch.stack([lo2, hi2]).contiguous()


@pytest.mark.parametrize("name", ["doc", "doc_w65"])
def test_shifted_bounds_fail_the_probes(name):
    kw = kernel_kw(name)[0]
    bad = dict(kw, bounds=shifted_bounds(kw["bounds"]))
    assert not count_rejected(name, kw)
    assert count_rejected(name, bad)
    # the backward: dV of the dK/dV pass (hi plane) and dQ (lo plane) against the unshifted expectation
    Hq, Hkv, D, dtype = 4, 2, 64, BF16
    (q, k, v, do, o), delta, want = unit_case(name, "q0", Hq, Hkv, D, dtype)
    qv, kv, vv, dov = (pv(x, dtype) for x in (q, k, v, do))
    lse = torch.zeros(B, Hq, T, dtype=F32, device=DEV)
    outs = bwd_outputs(B, T, T, Hq, Hkv, D, dtype)
    args = (B, T, Hq, Hkv, A.SCALE, True, 0.0)
    ext().attn_bwd_part(0, qv, kv, vv, dov, lse, delta.to(F32), None, outs[1][0], outs[2][0], *args, **bad)
    ext().attn_bwd_part(1, qv, kv, vv, dov, lse, delta.to(F32), None, outs[0][0], None, *args, **bad)
    torch.cuda.synchronize()
    assert not torch.equal(outs[2][0].to(F64), want[2]), "dV does not see the shifted hi plane"
    assert not torch.equal(outs[0][0].to(F64), want[0]), "dQ does not see the shifted lo plane"


@pytest.mark.parametrize("name", ["qr1", "qr1_w65", "qr1_doc"])
def test_neighbouring_query_range_fails_the_count_probe(name):
    kw = kernel_kw(name)[0]
    assert not count_rejected(name, kw)
    assert count_rejected(name, dict(kw, q_range=(256, 384)))
    assert count_rejected(name, dict(kw, q_range=(0, 128)))
