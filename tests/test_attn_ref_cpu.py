"""The helpers of the bit-exact attention tests (tests/attn_ref.py), checked on the CPU.

Agreement: the probes' expected values equal dltb.ops.ref.attn_fwd / attn_bwd run in float64 on the same inputs
(ref keeps fp64 inputs fp64), ``visible`` equals the mask ref._attn_probs implies, and the document-bounds planes of
ref.doc_bounds equal the ones the visibility matrix implies, lo and hi.  Preconditions: the selector's underflow and
margin conditions and the exactness assertions inside count_expect / unit_expect hold for every case and head shape
the GPU tests run.  Sensitivity: a one-key error at a window, document, query-range or tile edge, a shifted keep
column, a swapped kv head and a swapped V tile each move the expectation by more than the comparison accepts.
"""
import functools

import pytest
import torch

import dltb  # noqa: F401
from dltb.ops import ref
from dltb.ops.rng import StepSeed

import attn_ref as A

F64, BF16, F16 = torch.float64, torch.bfloat16, torch.float16
B, T = 2, 512
ALL = pytest.mark.parametrize("name", list(A.CASES))
BWD = pytest.mark.parametrize("name", A.BWD_CASES)
HEADS = pytest.mark.parametrize("Hq,Hkv,D", A.HEADS)
MID = (4, 2, 64)


def seed_obj():
    s = StepSeed(42, 0)
    s.next()
    return s


def gen(n=0):
    return torch.Generator().manual_seed(1234 + n)


@functools.lru_cache(maxsize=None)
def ref_kw(name, T_=T):
    """(arguments of ref.attn_fwd / attn_bwd for a case, Tq, q0)"""
    c = A.case(name)
    kw = {}
    if c["docs"]:
        kw["bounds"] = ref.doc_bounds(A.doc_tokens(A.doc_ids(B, T_)), 0, c["window"])
    elif c["window"]:
        kw["window"] = c["window"]
    if c["q_range"]:
        kw["q_range"] = c["q_range"]
    qb, qe = c["q_range"] or (0, T_)
    return kw, qe - qb, qb


def sink_of(name, Hq):
    s = A.case(name)["sink"]
    return None if s is None else torch.full((Hq,), s, dtype=F64)


# ------------------------------------------------------------------------------ visibility
@ALL
def test_visible_is_the_reference_mask(name):
    c = A.case(name)
    kw, Tq, q0 = ref_kw(name)
    z = torch.zeros(B * Tq, 8, dtype=F64)
    s = ref._attn_probs(z, torch.zeros(B * T, 8, dtype=F64), B, T, 1, 1, 8, 1.0, c["causal"], kw.get("window", 0),
                        kw.get("bounds"), q0, q0 + Tq)
    assert torch.equal(torch.isfinite(s)[:, 0], A.case_visible(name, B, T))


@pytest.mark.parametrize("window", [0, 1, 65, 129])
def test_bounds_planes_follow_from_visible(window):
    ids = A.doc_ids(B, T)
    vis = A.visible(B, T, True, window, ids)
    got = ref.doc_bounds(A.doc_tokens(ids), 0, window)
    want = A.bounds_of(vis)
    assert torch.equal(got[0], want[0]), "lo plane"
    assert torch.equal(got[1], want[1]), "hi plane"
    # the documents the issue names: starts at 1, 63, 64, 65, 128, and one-token documents at 63 and 64
    assert ids[0, [0, 1, 62, 63, 64, 65, 127, 128]].tolist() == [0, 1, 1, 2, 3, 4, 4, 5]
    if window == 0:
        assert vis[0, 63].sum() == 1 and vis[0, 64].sum() == 1 and vis[0, 0].sum() == 1


# ------------------------------------------------------------------------------ count probe
def count_case(name, Hq, Hkv, D, T_=T, Bn=B):
    c = A.case(name)
    kw, Tq, q0 = ref_kw(name, T_)
    vis = A.case_visible(name, Bn, T_)
    seed = seed_obj()
    keep = A.keep_of(name, Bn, T_, Hq, seed, "cpu")
    q, k, v = A.count_inputs(gen(), Bn, T_, Tq, Hq, Hkv, D)
    o, lse, acc, l = A.count_expect(v, vis, keep, c["p"], c["sink"], Bn, T_, Hq, Hkv, D)
    return c, kw, seed, vis, keep, (q, k, v), (o, lse)


@ALL
@HEADS
def test_count_probe_is_the_reference(name, Hq, Hkv, D):
    c, kw, seed, vis, keep, (q, k, v), (o, lse) = count_case(name, Hq, Hkv, D)
    ro, rl = ref.attn_fwd(q, k, v, B, T, Hq, Hkv, A.SCALE, c["causal"], c["p"], seed, A.SITE, sink=sink_of(name, Hq),
                          softcap=A.CAP if c["cap"] else 0.0, **kw)
    assert ro.dtype == F64 and rl.dtype == F64
    assert float((ro - o).abs().max()) < 1e-12 and float((rl - lse).abs().max()) < 1e-12
    for dt in (BF16, F16):
        for x in (q, k, v):
            A.to16(x, dt)


def test_count_probe_sinks():
    """sink = 0 adds exactly 1 to l; the negative sink changes nothing."""
    base = count_case("causal", *MID)[6]
    s0 = count_case("sink0", *MID)[6]
    sn = count_case("sinkneg", *MID)[6]
    assert torch.equal(sn[0], base[0]) and torch.equal(sn[1], base[1])
    assert torch.equal(torch.exp(s0[1]).round(), torch.exp(base[1]).round() + 1)


# ------------------------------------------------------------------------------ selector probe
def selector_case(name, Hq, Hkv, D, T_=T, Bn=B):
    c = A.case(name)
    kw, Tq, q0 = ref_kw(name, T_)
    vis = A.case_visible(name, Bn, T_)
    seed = seed_obj()
    keep = A.keep_of(name, Bn, T_, Hq, seed, "cpu")
    q, k, v, tgt = A.selector_inputs(gen(1), vis, Bn, T_, Hq, Hkv, D)
    cap = A.SEL_CAP if c["cap"] else 0.0
    cond = A.selector_check(q, k, vis, tgt, Bn, T_, Hq, Hkv, D, cap=cap)
    want = A.selector_expect(v, tgt, keep, c["p"], q0, Bn, T_, Hq, Hkv, D)
    return c, kw, seed, cap, (q, k, v, tgt), want, cond


@ALL
@HEADS
def test_selector_probe_conditions_and_reference(name, Hq, Hkv, D):
    c, kw, seed, cap, (q, k, v, tgt), want, cond = selector_case(name, Hq, Hkv, D)
    print(f"{name}: largest non-target probability 2^{cond[0]:.0f}, margin / rounding {cond[1]:.0f}")
    ro, _ = ref.attn_fwd(q, k, v, B, T, Hq, Hkv, A.SCALE, c["causal"], c["p"], seed, A.SITE, sink=sink_of(name, Hq),
                         softcap=cap, **kw)
    assert float((ro - want).abs().max()) < 2.0 ** -150
    for dt in (BF16, F16):
        for x in (q, k, v):
            A.to16(x, dt)
    assert "exact" == A.selector_blame(want, want, v, tgt, B, T, Hq, Hkv, D)


def test_selector_long_row():
    selector_case("causal", 2, 2, 64, 1024, 1)


def test_selector_blame_names_the_key():
    c, kw, seed, cap, (q, k, v, tgt), want, _ = selector_case("causal", *MID)
    got = want.clone().view(B, T, 4, 64)
    got[1, 300, 3] = v.view(B, T, 2, 64)[1, 17, 1]
    msg = A.selector_blame(got.view(B * T, -1), want, v, tgt, B, T, *MID)
    assert "i=300, h=3" in msg and "(1, 17, 1)" in msg


# ------------------------------------------------------------------------------ unit-probability probe
def unit_case(name, variant, Hq, Hkv, D, dtype, T_=T, Bn=B):
    c = A.case(name)
    kw, Tq, q0 = ref_kw(name, T_)
    vis = A.case_visible(name, Bn, T_)
    seed = seed_obj()
    keep = A.keep_of(name, Bn, T_, Hq, seed, "cpu")
    q, k, v, do, o = A.unit_inputs(gen(2), variant, Bn, T_, Tq, Hq, Hkv, D)
    delta = A.unit_delta(do, o, Bn, Tq, Hq, D)
    want = A.unit_expect(q, k, v, do, delta, vis, keep, c["p"], Bn, T_, Hq, Hkv, D, dtype)
    return c, kw, seed, (q, k, v, do, o), delta, want


@BWD
@HEADS
@pytest.mark.parametrize("variant", ["q0", "k0"])
def test_unit_probe_is_the_reference(name, variant, Hq, Hkv, D):
    outs = {}
    for dt in (BF16, F16):
        c, kw, seed, (q, k, v, do, o), delta, outs[dt] = unit_case(name, variant, Hq, Hkv, D, dt)
        for x in (q, k, v, do, o):
            A.to16(x, dt)
    Tq = q.shape[0] // B
    assert bool((delta % 2 == 0).all()) and float(delta.abs().max()) == 2
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ref.attn_bwd(q, k, v, o, do, torch.zeros(B, Hq, Tq, dtype=F64), dq, dk, dv, B, T, Hq, Hkv, A.SCALE, c["causal"],
                 c["p"], seed, A.SITE, softcap=A.CAP if c["cap"] else 0.0, **kw)
    for dt in (BF16, F16):
        for got, want in zip((dq, dk, dv), outs[dt]):
            assert torch.equal(A.round16(got, dt), want)
    assert float((dq if variant == "q0" else dk).abs().max()) > 0 and float(dv.abs().max()) > 0


def test_unit_long_row():
    unit_case("causal", "q0", 2, 2, 64, BF16, 1024, 1)


def test_cap_keeps_the_zero_score_exact():
    assert A.cap_exact(A.CAP)
    assert not A.cap_exact(1.0)         # X = 1.44: X + 2 needs one more bit


# ------------------------------------------------------------------------------ sensitivity
def rejects_count(got, want, dtype=BF16):
    """The comparison of the count probe rejects (o, lse) ``got`` against ``want``."""
    return (A.flagged(got[0], want[0], A.o_bound(want[0], dtype)) > 0
            or A.flagged(got[1], want[1], A.lse_bound(want[1])) > 0)


def count_with(name, vis=None, keep="case", v_map=None, Hq=4, Hkv=2, D=64):
    c = A.case(name)
    _, Tq, _ = ref_kw(name)
    if vis is None:
        vis = A.case_visible(name, B, T)
    seed = seed_obj()
    kp = A.keep_of(name, B, T, Hq, seed, "cpu") if isinstance(keep, str) else keep
    _, _, v = A.count_inputs(gen(), B, T, vis.shape[1], Hq, Hkv, D)
    if v_map is not None:
        v = v_map(v)
    return A.count_expect(v, vis, kp, c["p"], c["sink"], B, T, Hq, Hkv, D)[:2]


@pytest.mark.parametrize("name,d", [(n, d) for n in ["w1", "w63", "w64", "w65", "w129", "w511", "doc_w65", "qr1_w65",
                                                       "cap_w65"] for d in (-1, 1) if (n, d) != ("w1", -1)])
def test_window_off_by_one_is_seen(name, d):      # (w1, -1) would be window 0, which means no window
    want = count_with(name)
    assert not rejects_count(want, want)
    assert rejects_count(count_with(name, A.case_visible(name, B, T, window_delta=d)), want)


@pytest.mark.parametrize("name", ["doc", "doc_w65", "qr1_doc", "qr3_doc"])
def test_document_boundary_moved_by_one_is_seen(name):
    want = count_with(name)
    for which in range(5):
        for d in (-1, 1):
            starts = tuple(tuple(s + d if n == which else s for n, s in enumerate(row)) for row in A.DOC_STARTS)
            vis = A.case_visible(name, B, T, starts=starts)
            if torch.equal(vis, A.case_visible(name, B, T)):
                continue                      # a boundary the range's queries never reach
            assert rejects_count(count_with(name, vis), want), (which, d)
    assert rejects_count(count_with(name, A.case_visible(name, B, T, starts=((1, 63, 64, 65, 129), (128, 129, 200, 321, 449)))),
                         want)


@pytest.mark.parametrize("name", ["qr1", "qr3", "qr1_w65", "qr1_doc"])
def test_query_range_shifted_by_a_block_is_seen(name):
    qb, qe = A.case(name)["q_range"]
    want = count_with(name)
    other = (qb - 128, qe - 128)
    assert rejects_count(count_with(name, A.case_visible(name, B, T, q_range=other)), want)


@pytest.mark.parametrize("name", ["drop", "drop_causal"])
def test_keep_column_shifted_by_one_is_seen(name):
    keep = A.keep_of(name, B, T, 4, seed_obj(), "cpu")
    want = count_with(name)
    assert rejects_count(count_with(name, keep=keep.roll(1, -1)), want)
    c, kw, seed, cap, (q, k, v, tgt), sel, _ = selector_case(name, *MID)
    assert not torch.equal(A.selector_expect(v, tgt, keep.roll(1, -1), 0.5, 0, B, T, *MID), sel)


@pytest.mark.parametrize("name", ["full", "causal", "w65"])
def test_swapped_kv_head_is_seen(name):
    swap = lambda v: v.view(B * T, 2, 64).flip(1).reshape(B * T, 128)      # noqa: E731
    want = count_with(name)
    assert rejects_count(count_with(name, v_map=swap), want)
    c, kw, seed, cap, (q, k, v, tgt), sel, _ = selector_case(name, *MID)
    assert not torch.equal(A.selector_expect(swap(v), tgt, None, 0.0, 0, B, T, *MID), sel)


@pytest.mark.parametrize("name", ["full", "causal"])
@pytest.mark.parametrize("t", [0, 2, 6])
def test_swapped_v_tile_is_seen(name, t):
    """V tile t <-> t + 1 (the K / V pairing of one key split): the selector sees it in every row aimed at either."""
    def swap(v):
        v = v.clone().view(B, T, -1)
        v[:, 64 * t:64 * t + 64], v[:, 64 * t + 64:64 * t + 128] = (v[:, 64 * t + 64:64 * t + 128].clone(),
                                                                     v[:, 64 * t:64 * t + 64].clone())
        return v.view(B * T, -1)
    c, kw, seed, cap, (q, k, v, tgt), sel, _ = selector_case(name, *MID)
    got = A.selector_expect(swap(v), tgt, None, 0.0, 0, B, T, *MID)
    wrong = (got != sel).any(-1).view(B, T)
    aimed = ((tgt // 64 == t) | (tgt // 64 == t + 1)).any(1)
    assert bool(wrong.any()) and torch.equal(wrong, aimed)


@pytest.mark.parametrize("name", ["full", "causal", "w129", "doc"])
def test_one_dropped_pair_at_a_tile_edge_is_seen(name):
    want = count_with(name)
    vis = A.case_visible(name, B, T).clone()
    i = 511
    j = int(vis[1, i].nonzero()[:, 0][vis[1, i].nonzero()[:, 0] % 64 == 0][-1])      # a tile's first key
    vis[1, i, j] = False
    got = count_with(name, vis)
    assert rejects_count(got, want)
    assert A.flagged(got[1], want[1], A.lse_bound(want[1])) > 0          # l is off by one: lse sees 1 / n
