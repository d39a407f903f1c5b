"""Shared helpers of the bit-exact attention tests (tests/test_attention_exact_gpu.py; checked themselves in
tests/test_attn_ref_cpu.py).  Plain torch in float64 on whatever device the inputs live on; the extension is never
loaded.  The only project code used is the dropout keep-mask hash ``dltb.ops.ref._attn_keep``, which the kernels
share by construction (csrc/common.h rng_attn_pair).

Three probes.  Each chooses inputs for which every rounding point of csrc/attention.hip is exact, so its expectation
needs no error model of the MFMA, of exp2 or of the bf16 probability operand.

    count probe (forward)       Q = 0: every score is exactly 0 under any scale folding and under the soft-cap
                                (tanh 0 = 0), every visible probability is exp2(0) = 1.  V holds small integers,
                                distinct per (batch, kv head).  acc = sum_visible z V and l = n_i (+ exp(sink)) are
                                exact integers; O = acc / l and lse = ln l take the derived bounds below.
    selector probe (forward)    key j carries a +-A code of j, query i the code of a target key j*(i): the target's
                                probability is exactly 1, every other one underflows to exactly 0, O[i] == V[j*(i)]
                                bit for bit (times the exact dropout factor 0 or 2).
    unit-probability probe      backward with lse = 0 and scores of exactly 0 (Q = 0 with integer K, or K = 0 with
    (backward)                  integer Q): P = 1 on the visible set, dV, dS, dQ, dK are exact integers (times
                                scale = 1/8), compared with torch.equal against round16(want).

What the probes see: which (query, key) pairs a kernel takes as visible (one key too many or too few changes l by 1
and lse by 1 / n), which V / dO / Q / K row is paired with which probability (head, batch, tile and key-split
offsets), the dropout bit of each pair, the merge of the key splits and the rescale that must wipe earlier tiles to
exactly 0.  What they cannot see: the accuracy of exp2 and of the rescale on non-degenerate scores, the rounding of
the bf16 probability operand, and the accuracy on random data: those stay with the close() tests.

Bounds of the count probe (the only two tolerances of these tests), with U = 2^-24 and MARGIN = 2 as in gemm_ref.py:

    O    half_ulp(want) + MARGIN * K_O * U * |want|,  K_O = 2: after the exact accumulator the forward epilogue does
         ``inv = drop_scale / l`` (one IEEE division: the file is built without fast-math, the drop scale is its
         numerator, and with a sink ``a / l`` with a = exp2(0) = 1) and ``acc * inv`` in store_acc_rows (one
         multiply); then the one rounding to 16 bits.
    lse  MARGIN * K_LSE * U * max(1, |want|),  K_LSE = 5: ``(m + __log2f(l)) * 0.693...`` with m = 0 is v_log_f32
         (1 ulp = 2 U), the add, the multiply and the rounding of the constant ln 2 itself.  l is exact: the sinks
         used here are 0 (exp2(0) = 1, l + 1) or so negative that exp2 underflows (l + 0).

ASSUMPTIONS, the ones the CAP comment of csrc/attention.hip makes too: v_exp_f32, v_log_f32 and v_rcp_f32 are good
to 1 ulp, and they are exact where the result is a power of two from a power-of-two argument: exp2(0) = 1,
exp2(2) = 4, rcp(2) = 0.5, exp2(x) = 0 for x < -150.  Nothing in this tree states that; the probes would show it.

The CAP kernels stay exact at a zero score: t = fma(-2, rcp(1 + exp2(0)), 1) = 0; the forward's exponent is
fma(-2 X, 0.5, X - m) with X = fl(cap log2 e), exactly -m; the dQ pass forms 4 p = exp2(fma(-2 X, 0.5, fl(fl(X + nl)
+ 2))), which is exp2(2) = 4 exactly iff X + 2 is a float (``cap_exact``: true for cap = 50, X = 72.13 and X + 2 in
one binade), times r - r^2 = 0.25.  So no variant falls back from torch.equal to a bound.
"""
import math

import torch

from dltb.ops.ref import _attn_keep  # noqa: F401  (the hash the kernels share; re-exported)
from gemm_ref import EXACT_LIMIT, MARGIN, U, poisoned_view  # noqa: F401
from rowwise_ref import half_ulp, round16

F64 = torch.float64
LOG2E = math.log2(math.e)
K_O = 2          # fp32 operations after the exact accumulator (module docstring)
K_LSE = 5
SCALE = 0.125    # an argument of the kernels: the same exact power of two for both head sizes
CAP = 50.0       # count and backward probes (cap_exact)
SEL_CAP = 16384.0   # selector probe: large enough that the capped margin still underflows (selector_check)
SINK_NEG = -30000.0  # exp2(-30000 log2 e) = 0 in fp32
SITE = 11

# (Hq, Hkv, D): plain, GQA, and GQA at D = 128 (the head-split dK/dV path)
HEADS = [(2, 2, 64), (4, 2, 64), (8, 2, 128)]
# document starts per batch row: boundaries at tokens 1, 63, 64, 65, 128 (tokens 63 and 64 are one-token documents)
DOC_STARTS = ((1, 63, 64, 65, 128), (128, 129, 200, 321, 448))

# every mask case of the GPU tests; only what csrc/bindings.cpp allows together
CASES = {
    "full": dict(causal=False),
    "causal": dict(causal=True),
    "w1": dict(causal=True, window=1),
    "w63": dict(causal=True, window=63),
    "w64": dict(causal=True, window=64),
    "w65": dict(causal=True, window=65),
    "w129": dict(causal=True, window=129),
    "w511": dict(causal=True, window=511),
    "doc": dict(causal=True, docs=True),
    "doc_w65": dict(causal=True, docs=True, window=65),
    "qr1": dict(causal=True, q_range=(128, 256)),
    "qr3": dict(causal=True, q_range=(384, 512)),
    "qr1_w65": dict(causal=True, q_range=(128, 256), window=65),
    "qr3_w129": dict(causal=True, q_range=(384, 512), window=129),
    "qr1_doc": dict(causal=True, q_range=(128, 256), docs=True),
    "qr3_doc": dict(causal=True, q_range=(384, 512), docs=True),
    "sink0": dict(causal=True, sink=0.0),
    "sinkneg": dict(causal=True, sink=SINK_NEG),
    "cap": dict(causal=True, cap=True),
    "cap_w65": dict(causal=True, cap=True, window=65),
    "drop": dict(causal=False, p=0.5),
    "drop_causal": dict(causal=True, p=0.5),
}
BWD_CASES = [c for c in CASES if not c.startswith("sink")]      # the backward kernels have no sink


def case(name):
    c = dict(causal=False, window=0, docs=False, q_range=None, sink=None, cap=False, p=0.0)
    c.update(CASES[name])
    return c


# ------------------------------------------------------------------------------ visibility, from the definition
def doc_ids(B, T, starts=DOC_STARTS, device=None):
    """int64 [B, T]: the document of every token; a document starts at token 0 and at every listed token."""
    t = torch.arange(T, device=device)
    return torch.stack([sum((t >= s).long() for s in starts[b % len(starts)]) for b in range(B)])


def doc_tokens(ids, eos_id=0):
    """A token table [B, T] whose documents are ``ids``: the last token of every document (but the row's last) is
    ``eos_id``, every other token 1.  The input of ref.doc_bounds / attn_doc_bounds."""
    idx = torch.ones_like(ids)
    idx[:, :-1][ids[:, 1:] != ids[:, :-1]] = eos_id
    return idx


def visible(B, T, causal, window=0, doc_ids=None, q_range=None, device=None):
    """bool [B, Tq, T]: query i (global position) sees key j.  causal: j <= i; window W: i - W < j; documents:
    the same document id.  ``q_range`` keeps the rows of the range."""
    dev = doc_ids.device if doc_ids is not None else device
    i = torch.arange(T, device=dev)[:, None]
    j = torch.arange(T, device=dev)[None, :]
    vis = torch.ones(T, T, dtype=torch.bool, device=dev)
    if causal:
        vis &= j <= i
    if window:
        assert causal
        vis &= i - window < j
    vis = vis[None].repeat(B, 1, 1)
    if doc_ids is not None:
        assert causal
        vis &= doc_ids[:, :, None] == doc_ids[:, None, :]
    if q_range is not None:
        vis = vis[:, q_range[0]:q_range[1]]
    return vis


def case_visible(name, B, T, device=None, window_delta=0, starts=DOC_STARTS, q_range="case"):
    c = case(name)
    ids = doc_ids(B, T, starts, device) if c["docs"] else None
    w = c["window"] + window_delta if c["window"] else 0
    return visible(B, T, c["causal"], w, ids, c["q_range"] if q_range == "case" else q_range, device)


def bounds_of(vis):
    """The [2, B, T] lo / hi planes a full-range causal visibility matrix implies: lo[i] the first key of query i,
    hi[j] one past the last query that sees key j."""
    B, Tq, T = vis.shape
    assert Tq == T
    lo = vis.int().argmax(2)
    hi = T - vis.flip(1).int().argmax(1)
    return torch.stack([lo, hi]).to(torch.int32)


def keep_of(name, B, T, Hq, seed, device):
    """bool [B, Hq, T, T] keep decisions of a case, None without dropout."""
    return _attn_keep(B, Hq, T, case(name)["p"], seed, SITE, device)


def _zfac(vis, keep, p):
    """float64 [B, Hq | 1, Tq, T]: visible times the dropout factor (1, or keep / (1 - p))."""
    z = vis[:, None].to(F64)
    if keep is not None:
        z = z * keep.to(F64) / (1.0 - p)
    return z


def _heads(x, B, T, H, D, G=1):
    """[B * T, H * D] -> float64 [B, H * G, T, D]"""
    x = x.to(F64).reshape(B, T, H, D).transpose(1, 2)
    return x.repeat_interleave(G, dim=1) if G > 1 else x


def _rows(x):
    """[B, H, T, D] -> [B * T, H * D]"""
    B, H, T, D = x.shape
    return x.transpose(1, 2).reshape(B * T, H * D)


def ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen, device=gen.device).to(F64)


def to16(x, dtype):
    y = x.to(dtype)
    assert torch.equal(y.to(F64), x.to(F64)), "value not representable in the 16-bit format"
    return y


# ------------------------------------------------------------------------------ count probe (forward)
def count_inputs(gen, B, T, Tq, Hq, Hkv, D):
    """(q, k, v) in float64, exact in both 16-bit formats: q = 0, k random finite, v integers in [-8, 8] drawn
    apart for every (batch, kv head)."""
    q = torch.zeros(B * Tq, Hq * D, dtype=F64, device=gen.device)
    k = torch.randn(B * T, Hkv * D, generator=gen, device=gen.device).bfloat16().half().to(F64)   # fits both
    v = ints(gen, (B * T, Hkv * D), -8, 8)
    return q, k, v


def count_expect(v, vis, keep, p, sink, B, T, Hq, Hkv, D):
    """(o, lse, acc, l) in float64: o [B * Tq, Hq * D], lse [B, Hq, Tq].  ``sink``: None or one logit for every head.
    Asserts the exactness preconditions: acc and l are integers below 2^24 and the probability operand is 0 or 1."""
    z = _zfac(vis, keep, p)                                         # 0 / 1 / 2
    zk = z * (1.0 - p)                                              # what the kernel holds: p & keep, 0 or 1
    assert bool(((zk == 0) | (zk == 1)).all())
    vh = _heads(v, B, T, Hkv, D, Hq // Hkv)
    acc_k = torch.matmul(zk, vh)                                    # the kernel's accumulator
    l = vis.sum(-1).to(F64)[:, None].expand(B, Hq, vis.shape[1]).clone()
    assert float(torch.matmul(zk, vh.abs()).max()) < EXACT_LIMIT and float(l.max()) < EXACT_LIMIT
    assert float(l.min()) >= 1
    if sink is not None:
        e = math.exp(sink)
        assert e in (0.0, 1.0), "only sinks whose exp is exact"
        l = l + e
    acc = acc_k / (1.0 - p)
    return _rows(acc / l[..., None]), torch.log(l), acc, l


def o_bound(want, dtype):
    return half_ulp(want, dtype) + MARGIN * K_O * U * want.abs()


def lse_bound(want):
    return MARGIN * K_LSE * U * want.abs().clamp(min=1.0)


def flagged(got, want, bnd):
    """Share of elements of ``got`` outside ``bnd`` of ``want``."""
    return float((~((got.to(F64) - want.to(F64)).abs() <= bnd)).double().mean())


def report(what, got, want, bnd):
    """Every element within its bound; prints and returns the worst error / bound ratio."""
    got, want = got.to(F64), want.to(F64)
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} against {tuple(want.shape)}"
    err = (got - want).abs()
    ratio = torch.where(bnd > 0, err / bnd, torch.where(err > 0, torch.full_like(err, math.inf), err))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    worst = float(ratio.max())
    print(f"{what}: worst error/bound {worst:.3f} ({got.numel()} elements)")
    nbad = int((~(err <= bnd)).sum())
    assert nbad == 0, f"{what}: {nbad} of {got.numel()} elements outside their bound, worst error/bound {worst:.3f}"
    return worst


# ------------------------------------------------------------------------------ selector probe (forward)
SEL_A = 32.0     # code amplitude


def selector_targets(vis, Hq):
    """int64 [B, Hq, Tq]: the target key j*(i) of every query, by a fixed formula over the row's visible keys
    (a contiguous run first .. first + n - 1 in every mask case): rows i % 3 == 0 take the first visible key,
    i % 3 == 1 the last (the diagonal under a causal mask), the others first + (37 i + 11 h + 5 b) % n.  Asserts
    that the targets are visible and that every key tile with a visible key is some query's target tile."""
    B, Tq, T = vis.shape
    n = vis.sum(-1)
    first = vis.int().argmax(-1)
    last = T - 1 - vis.flip(-1).int().argmax(-1)
    assert bool((n >= 1).all()) and bool((last - first + 1 == n).all()), "visible keys must be one run per row"
    dev = vis.device
    i = torch.arange(Tq, device=dev)[None, None, :]
    h = torch.arange(Hq, device=dev)[None, :, None]
    b = torch.arange(B, device=dev)[:, None, None]
    nn = n[:, None, :]
    off = torch.where(i % 3 == 0, torch.zeros_like(nn), torch.where(i % 3 == 1, nn - 1, (37 * i + 11 * h + 5 * b) % nn))
    tgt = first[:, None, :] + off
    assert bool(torch.gather(vis[:, None].expand(B, Hq, Tq, T), 3, tgt[..., None]).all())
    seen = torch.zeros(T // 64, dtype=torch.bool, device=dev)
    seen[(vis.any(1).nonzero()[:, 1] // 64).unique()] = True
    hit = torch.zeros_like(seen)
    hit[(tgt // 64).unique()] = True
    assert torch.equal(seen, hit), "targets must reach every key tile with a visible key"
    return tgt


def _code(j, nb, D):
    """float64 [..., D]: +-SEL_A by bit d of j in the first nb dimensions, 0 in the rest."""
    d = torch.arange(D, device=j.device)
    bit = (j[..., None] >> d.clamp(max=nb - 1)) & 1
    return torch.where(d < nb, (2 * bit - 1).to(F64) * SEL_A, torch.zeros((), dtype=F64, device=j.device))


def selector_inputs(gen, vis, B, T, Hq, Hkv, D):
    """(q, k, v, tgt) in float64, exact in both formats.  k's unused dimensions hold small integers (q is 0 there),
    v is N(0, 1) rounded to both formats: distinct rows, so a wrong row is named by ``selector_blame``."""
    dev = vis.device
    Tq = vis.shape[1]
    nb = max(1, (T - 1).bit_length())
    assert nb <= D
    tgt = selector_targets(vis, Hq)
    q = _code(tgt, nb, D).transpose(1, 2).reshape(B * Tq, Hq * D)
    kc = _code(torch.arange(T, device=dev), nb, D)                        # [T, D]
    k = kc[None, :, None, :].expand(B, T, Hkv, D).clone()
    k[..., nb:] = ints(gen, (B, T, Hkv, D - nb), -2, 2)
    v = torch.randn(B * T, Hkv * D, generator=gen, device=dev).bfloat16().half().to(F64)
    return q, k.reshape(B * T, Hkv * D), v, tgt


def selector_check(q, k, vis, tgt, B, T, Hq, Hkv, D, scale=SCALE, cap=0.0):
    """The two float64 conditions of the selector probe; returns (log2 of the largest non-target probability,
    margin / rounding ratio).  (a) every visible non-target score lies more than 160 octaves under the target's:
    its probability is below 2^-160, far under the smallest fp32 subnormal, so exp2 gives exactly 0 and a rescale
    by it wipes earlier tiles.  (b) that margin is at least 16 times 2^-9 |target score|, the relative rounding of
    Q scale log2 e to 16 bits."""
    Tq = vis.shape[1]
    s = torch.matmul(_heads(q, B, Tq, Hq, D), _heads(k, B, T, Hkv, D, Hq // Hkv).transpose(-1, -2)) * scale
    if cap:
        s = cap * torch.tanh(s / cap)
    st = torch.gather(s, 3, tgt[..., None])
    other = vis[:, None].expand_as(s).clone()
    other.scatter_(3, tgt[..., None], False)
    rest = s.masked_fill(~other, -math.inf).amax(-1, keepdim=True)
    margin = (st - rest) * LOG2E                                      # octaves; +inf for a row with one key
    worst = float(-margin.min())
    ratio = float((margin / (2.0 ** -9 * st.abs() * LOG2E)).min())
    assert worst < -160.0, f"selector: a non-target probability is 2^{worst:.1f}"
    assert ratio >= 16.0, f"selector: margin only {ratio:.1f} roundings of the folded scale"
    return worst, ratio


def selector_expect(v, tgt, keep, p, vis_q0, B, T, Hq, Hkv, D):
    """float64 [B * Tq, Hq * D]: V[j*(i)] of the query's kv head, times the dropout factor of the pair (0 or 2).
    ``vis_q0``: the global position of query row 0 (the keep mask is indexed by global query)."""
    vh = _heads(v, B, T, Hkv, D, Hq // Hkv)
    want = torch.gather(vh, 2, tgt[..., None].expand(*tgt.shape, D))
    if keep is not None:
        Tq = tgt.shape[2]
        kz = torch.gather(keep[:, :, vis_q0:vis_q0 + Tq], 3, tgt[..., None]).to(F64) / (1.0 - p)
        want = want * kz
    return _rows(want)


def selector_blame(got, want, v, tgt, B, T, Hq, Hkv, D):
    """Failure message: the first wrong output row, its target key, and the key(s) whose V row it equals."""
    Tq = tgt.shape[2]
    g = got.to(F64).reshape(B, Tq, Hq, D)
    w = want.to(F64).reshape(B, Tq, Hq, D)
    bad = (g != w).any(-1).nonzero()
    if bad.numel() == 0:
        return "exact"
    b, i, h = (int(x) for x in bad[0])
    vh = v.to(F64).reshape(B, T, Hkv, D)
    row = g[b, i, h]
    hits = [(bb, int(j), hk) for bb in range(B) for hk in range(Hkv)
            for j in ((vh[bb, :, hk] == row).all(-1) | (2 * vh[bb, :, hk] == row).all(-1)).nonzero().flatten()[:4]]
    return (f"{bad.shape[0]} of {B * Tq * Hq} rows wrong; first o[b={b}, i={i}, h={h}] should be V[key "
            f"{int(tgt[b, h, i])}] of kv head {h // (Hq // Hkv)}; it equals V (or 2 V) at (batch, key, kv head) = "
            f"{hits if hits else 'no single key (a mixture, or NaN)'}")


# ------------------------------------------------------------------------------ unit-probability probe (backward)
def cap_exact(cap):
    """The dQ pass's CAP exponent at a zero score and lse = 0 is exactly 2 (module docstring): X + 2 is a float."""
    f32 = torch.float32
    X = torch.tensor(cap, dtype=f32) * torch.tensor(1.4426950408889634, dtype=f32)
    c0 = (X + torch.tensor(-0.0, dtype=f32)) + torch.tensor(2.0, dtype=f32)
    return float(c0.double() - X.double()) == 2.0


def unit_inputs(gen, variant, B, T, Tq, Hq, Hkv, D):
    """(q, k, v, do, o) in float64.  ``variant`` "q0": Q = 0, K integers in [-2, 2]; "k0": the reverse.  V in
    {-1, 0, 1}, dO in {-1, 0, 1}; o has one non-zero per (row, head), +-2 at column (7 i + 3 h) % D, so that
    delta = rowsum(dO o) is an exact even integer in {-2, 0, 2}."""
    dev = gen.device
    qi = ints(gen, (B * Tq, Hq * D), -2, 2)
    ki = ints(gen, (B * T, Hkv * D), -2, 2)
    q, k = (torch.zeros_like(qi), ki) if variant == "q0" else (qi, torch.zeros_like(ki))
    assert variant in ("q0", "k0")
    v = ints(gen, (B * T, Hkv * D), -1, 1)
    do = ints(gen, (B * Tq, Hq * D), -1, 1)
    o = torch.zeros(B * Tq, Hq, D, dtype=F64, device=dev)
    r = torch.arange(B * Tq, device=dev)[:, None]
    h = torch.arange(Hq, device=dev)[None, :]
    col = (7 * r + 3 * h) % D
    o.scatter_(2, col[..., None], (2.0 * (2 * ((r + h) % 2) - 1)).to(F64)[..., None])
    return q, k, v, do, o.reshape(B * Tq, Hq * D)


def unit_delta(do, o, B, Tq, Hq, D):
    """float64 [B, Hq, Tq] = rowsum(dO o)"""
    return (_heads(do, B, Tq, Hq, D) * _heads(o, B, Tq, Hq, D)).sum(-1)


def unit_expect(q, k, v, do, delta, vis, keep, p, B, T, Hq, Hkv, D, dtype, scale=SCALE):
    """(dq, dk, dv) as round16 of the exact float64 values, for lse = 0 and scores of exactly 0.

    Read from csrc/attention.hip: both backward kernels hold, per pair, the probability operand pd = p & keep (0 or
    1) and ds' = keep dP - delta / s with s = 1 / (1 - p) the drop scale (dK/dV: ``fma(pdv, dp[i], p * Dv[e])`` with
    Dv = -delta inv_s; dQ: ``p * keep_sel(dp, nd)`` with the accumulator started at nd = -delta / s), round ds' to
    the 16-bit MFMA operand (pack_frag), accumulate dV += dO^T pd, dK += Q^T ds', dQ += K^T ds' in fp32, sum the
    key / query splits and the GQA group in fp32, and multiply by s (dV) or scale s (dQ, dK) at the store.  Asserted
    here: ds' is representable in ``dtype`` (under p = 0.5 it holds delta / 2, hence the even delta), every fp32
    sum of magnitudes stays below 2^24, and scale s is a power of two."""
    G = Hq // Hkv
    Tq = vis.shape[1]
    s = 1.0 / (1.0 - p)
    assert math.frexp(scale * s)[0] == 0.5
    visf = vis[:, None].to(F64)
    zk = visf if keep is None else visf * keep.to(F64)              # pd: 0 or 1
    qh, doh = _heads(q, B, Tq, Hq, D), _heads(do, B, Tq, Hq, D)
    kh, vh = _heads(k, B, T, Hkv, D, G), _heads(v, B, T, Hkv, D, G)
    dP = torch.matmul(doh, vh.transpose(-1, -2))
    dsk = visf * (zk * dP - delta[..., None] / s)                   # the kernels' ds'
    assert torch.equal(round16(dsk, dtype), dsk), "ds' is not representable as the 16-bit MFMA operand"
    assert float(dP.abs().max()) + float(delta.abs().max()) < EXACT_LIMIT
    dS = dsk * s                                                     # = vis (z dP - delta)
    for a, b_ in ((dsk.abs(), kh.abs()), (dsk.abs().transpose(-1, -2), qh.abs()), (zk.transpose(-1, -2), doh.abs())):
        t = torch.matmul(a, b_)
        assert float(t.view(B, Hkv, G, *t.shape[2:]).sum(2).max()) < EXACT_LIMIT
    dq = torch.matmul(dS, kh) * scale
    dk = (torch.matmul(dS.transpose(-1, -2), qh) * scale).view(B, Hkv, G, T, D).sum(2)
    dv = (torch.matmul(zk.transpose(-1, -2), doh) * s).view(B, Hkv, G, T, D).sum(2)
    return tuple(round16(_rows(x), dtype) for x in (dq, dk, dv))


# ------------------------------------------------------------------------------ memory discipline
def sentinel_out(rows, cols, dtype, device, contiguous=False):
    """(view, buffer, snapshot): an output view [rows, cols] inside a NaN-filled buffer (strided like
    ``poisoned_view``, or, for outputs the bindings want contiguous, a row range of a taller buffer)."""
    if contiguous:
        buf = torch.full((rows + 16, cols), math.nan, dtype=dtype, device=device)
        view = buf[8:8 + rows]
        assert view.is_contiguous() and view.data_ptr() % 16 == 0
    else:
        view, buf = poisoned_view(torch.full((rows, cols), math.nan, dtype=dtype, device=device), (3, 5), 8)
    return view, buf, buf.clone()


def check_sentinel(what, view, buf, snap):
    """No NaN left inside the view; every bit outside it as before."""
    assert not bool(torch.isnan(view).any()), f"{what}: elements of the output were not written"
    after = buf.clone()
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(True)
    i16 = torch.int16
    assert torch.equal(after.view(i16)[~inside], snap.view(i16)[~inside]), f"{what}: wrote outside its output view"
