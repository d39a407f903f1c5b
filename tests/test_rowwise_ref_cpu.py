"""The float64 references of tests/rowwise_ref.py against torch's own float64 operators, and half_ulp /
round16 against torch.nextafter.  tests/test_rowwise_gpu.py derives every kernel bound from these
references, so this file is what makes those bounds trustworthy.  No GPU, no extension."""
import math

import pytest
import torch
import torch.nn.functional as F

from rowwise_ref import (embed64, embed_dwpe64, embed_dwte64, gelu64, gelu_grad64, half_ulp, layernorm64,
                         norm_bwd64, rmsnorm64, rope64, round16, silu_mul64, silu_mul_grad64, xent64)

F64 = torch.float64
FORMATS = [torch.bfloat16, torch.float16]
# float64 against float64, a handful of operations each: 1e-12 relative to the largest magnitude involved
RTOL = 1e-12


def gen(seed):
    return torch.Generator().manual_seed(seed)


def close(a, b, scale=None):
    scale = float(b.abs().max()) if scale is None else scale
    err = float((a - b).abs().max())
    print(f"max error {err:.3e} (allowed {RTOL * max(scale, 1.0):.3e})")
    assert err <= RTOL * max(scale, 1.0)


# ------------------------------------------------------------------------------ the storage formats
def all_finite(dtype):
    """Every finite value of the format, by bit pattern."""
    v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)
    return v[torch.isfinite(v)]


@pytest.mark.parametrize("dtype", FORMATS)
def test_half_ulp_is_half_the_gap_to_the_next_value(dtype):
    """At every non-negative finite value v below the largest: half_ulp(v) = (nextafter(v, inf) - v) / 2, and
    the same inside the gap; normal, subnormal and zero alike."""
    v = all_finite(dtype)
    v = v[v >= 0].sort().values
    up = torch.nextafter(v, torch.full_like(v, math.inf))
    v, up = v[:-1].double(), up[:-1].double()              # the largest finite value is checked below
    assert bool((up > v).all())
    assert torch.equal(half_ulp(v, dtype), (up - v) / 2)
    mid = v + (up - v) * 0.75
    assert torch.equal(half_ulp(mid, dtype), (up - v) / 2)
    assert torch.equal(half_ulp(-mid, dtype), (up - v) / 2)
    sub = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133}[dtype]
    assert float(half_ulp(0.0, dtype)) == sub / 2 == float(half_ulp(sub * 3, dtype))
    tiny = torch.finfo(dtype).tiny                           # smallest normal: still the subnormal spacing
    assert float(half_ulp(tiny, dtype)) == sub / 2 and float(half_ulp(2 * tiny, dtype)) == sub


@pytest.mark.parametrize("dtype", FORMATS)
def test_half_ulp_and_round16_at_the_largest_finite_value(dtype):
    top = torch.finfo(dtype).max
    below = float(torch.nextafter(torch.tensor(top, dtype=dtype), torch.tensor(0.0, dtype=dtype)))
    h = (top - below) / 2
    assert float(half_ulp(top, dtype)) == h
    x = torch.tensor([top, top + 0.999 * h, top + h, -(top + h), 2 * top, math.inf, math.nan], dtype=F64)
    hu = half_ulp(x, dtype)
    assert hu[:2].tolist() == [h, h] and bool(torch.isinf(hu[2:]).all())
    r = round16(x, dtype)
    assert r[:6].tolist() == [top, top, math.inf, -math.inf, math.inf, math.inf] and math.isnan(float(r[6]))


@pytest.mark.parametrize("dtype", FORMATS)
def test_round16_is_nearest_even(dtype):
    """Exact on every finite value; nearest in both halves of every gap; ties to the even pattern; and right
    where float64 -> float32 -> 16 bit rounds twice (a hair above a tie)."""
    v = all_finite(dtype)
    assert torch.equal(round16(v.double(), dtype), v.double())
    pos = v[v >= 0].sort().values
    lo, hi = pos[:-1].double(), pos[1:].double()
    gap = hi - lo
    assert torch.equal(round16(lo + 0.25 * gap, dtype), lo)
    assert torch.equal(round16(-(lo + 0.75 * gap), dtype), -hi)
    even_lo = (pos[:-1].view(torch.int16) % 2 == 0)
    assert torch.equal(round16(lo + 0.5 * gap, dtype), torch.where(even_lo, lo, hi))
    nrm = lo >= float(torch.finfo(dtype).tiny)
    hair = (lo + 0.5 * gap)[nrm] * (1.0 + 2.0 ** -40)          # float32 rounds this onto the tie
    assert torch.equal(round16(hair, dtype), hi[nrm])
    got = round16(hair, dtype)
    err = (got - hair).abs()
    assert bool((err <= half_ulp(hair, dtype)).all())


# ------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("d", [8, 520])
def test_layernorm64_matches_torch(d):
    g = gen(d)
    x = torch.randn(5, d, generator=g, dtype=F64) + 3.0
    w, b = torch.randn(d, generator=g, dtype=F64), torch.randn(d, generator=g, dtype=F64)
    for eps in (1e-5, 1e-2):
        y, mean, rstd, s = layernorm64(x, w, b, eps)
        close(y, F.layer_norm(x, (d,), w, b, eps))
        close(mean, x.mean(-1))
        close(rstd, 1.0 / (x.var(-1, unbiased=False) + eps).sqrt())
        assert torch.equal(s, x)
        yr, none, rr, _ = rmsnorm64(x, w, eps)
        assert none is None
        close(yr, x / (x.pow(2).mean(-1, keepdim=True) + eps).sqrt() * w)
        if hasattr(F, "rms_norm"):
            close(yr, F.rms_norm(x, (d,), w, eps))


@pytest.mark.parametrize("dtype", FORMATS)
def test_norm_residual_stream_is_rounded_to_the_format(dtype):
    g = gen(7)
    x, r = torch.randn(4, 16, generator=g).to(dtype), torch.randn(4, 16, generator=g).to(dtype)
    keep = torch.rand(4, 16, generator=g) < 0.7
    w, b = torch.ones(16, dtype=F64), torch.zeros(16, dtype=F64)
    y, mean, rstd, s = layernorm64(x, w, b, 1e-5, residual=r, keep=keep, p=0.25)
    want_s = x.double() + torch.where(keep, r.double() / 0.75, torch.zeros(4, 16, dtype=F64))
    assert torch.equal(s, round16(want_s, dtype)) and torch.equal(s, s.to(dtype).double())
    close(y, F.layer_norm(s, (16,), w, b, 1e-5))
    assert torch.equal(rmsnorm64(x, w, 1e-5, residual=r)[3], round16(x.double() + r.double(), dtype))


@pytest.mark.parametrize("rms", [False, True])
def test_norm_bwd64_matches_autograd(rms):
    g = gen(11)
    N, d, eps = 7, 24, 1e-3
    s = (torch.randn(N, d, generator=g, dtype=F64) + 1.0).requires_grad_()
    w = torch.randn(d, generator=g, dtype=F64).requires_grad_()
    b = torch.randn(d, generator=g, dtype=F64).requires_grad_()
    dy, dres = torch.randn(N, d, generator=g, dtype=F64), torch.randn(N, d, generator=g, dtype=F64)
    if rms:
        y = s / (s.pow(2).mean(-1, keepdim=True) + eps).sqrt() * w
        _, mean, rstd, _ = rmsnorm64(s.detach(), w.detach(), eps)
    else:
        y = F.layer_norm(s, (d,), w, b, eps)
        _, mean, rstd, _ = layernorm64(s.detach(), w.detach(), b.detach(), eps)
    y.backward(dy)
    dx, dgamma, dbeta, dxs = norm_bwd64(dy, s.detach(), w.detach(), mean, rstd, dres, dxsum_dtype=torch.bfloat16)
    close(dx, s.grad + dres)
    close(dgamma, w.grad)
    if rms:
        assert dbeta is None
    else:
        close(dbeta, b.grad)
    assert torch.equal(dxs, round16(dx, torch.bfloat16).sum(0))
    assert float((dxs - dx.sum(0)).abs().max()) <= N * float(half_ulp(dx.abs().max(), torch.bfloat16))


# ------------------------------------------------------------------------------------ elementwise
def test_gelu64_matches_torch_and_keeps_the_negative_tail():
    x = torch.linspace(-12.0, 12.0, 4801, dtype=F64).requires_grad_()
    y = F.gelu(x)
    y.sum().backward()
    xd = x.detach()
    # torch evaluates 1 + erf, which cancels in the negative tail: absolute agreement there
    close(gelu64(xd), y.detach())
    close(gelu_grad64(xd), x.grad)
    # the tail itself, against the asymptotic Phi(x) ~ phi(x) / |x| (1 - 1/x^2 + 3/x^4), relative
    t = torch.tensor([-9.0, -10.0, -12.0], dtype=F64)
    phi = torch.exp(-0.5 * t * t) / math.sqrt(2 * math.pi)
    asym = t * phi / t.abs() * (1 - 1 / t ** 2 + 3 / t ** 4)
    assert bool(((gelu64(t) - asym).abs() <= 15 / t ** 6 * asym.abs()).all())
    assert float(gelu64(torch.tensor(0.0))) == 0.0 and float(gelu_grad64(torch.tensor(0.0))) == 0.5


def test_silu_mul64_matches_autograd():
    g = gen(3)
    gate = (torch.randn(6, 40, generator=g, dtype=F64) * 4).requires_grad_()
    up = torch.randn(6, 40, generator=g, dtype=F64).requires_grad_()
    dh = torch.randn(6, 40, generator=g, dtype=F64)
    h = F.silu(gate) * up
    h.backward(dh)
    close(silu_mul64(gate.detach(), up.detach()), h.detach())
    dg, du = silu_mul_grad64(dh, gate.detach(), up.detach())
    close(dg, gate.grad)
    close(du, up.grad)


def test_rope64_rotates_and_inverts():
    g = gen(5)
    N, T, H, D = 6, 3, 2, 16
    x = torch.randn(N, H, D, generator=g, dtype=F64)
    ang = torch.rand(T, D // 2, generator=g, dtype=F64) * 6
    cos, sin = ang.cos().float(), ang.sin().float()          # the tables as the kernel reads them
    y = rope64(x, cos, sin, T)
    for r in range(N):
        for i in range(D // 2):
            c, s = float(cos[r % T, i]), float(sin[r % T, i])
            for h in range(H):
                a, b = float(x[r, h, i]), float(x[r, h, i + D // 2])
                assert abs(float(y[r, h, i]) - (a * c - b * s)) <= 1e-14
                assert abs(float(y[r, h, i + D // 2]) - (b * c + a * s)) <= 1e-14
    back = rope64(y, cos, sin, T, inverse=True)
    # cos^2 + sin^2 of the float32 tables is 1 to 2^-23
    assert float((back - x).abs().max()) <= 2.0 ** -22 * float(x.abs().max())


# -------------------------------------------------------------------------------------- embedding
def test_embedding_references_match_index_add():
    g = gen(9)
    V, d, B, T, P = 11, 8, 3, 5, 7
    wte = torch.randn(V, d, generator=g, dtype=F64, requires_grad=True)
    wpe = torch.randn(P, d, generator=g, dtype=F64, requires_grad=True)
    idx = torch.randint(0, 4, (B, T), generator=g)
    keep = torch.rand(B, T, d, generator=g) < 0.8
    p = 0.2
    x = (wte[idx] + wpe[:T][None]) * keep / (1 - p)
    close(embed64(idx, wte.detach(), wpe.detach(), keep, p), x.detach())
    close(embed64(idx, wte.detach(), wpe.detach()), (wte[idx] + wpe[:T][None]).detach())
    dx = torch.randn(B, T, d, generator=g, dtype=F64)
    x.backward(dx)
    close(embed_dwte64(dx, idx, V, keep, p), wte.grad)
    close(embed_dwpe64(dx, P, keep, p), wpe.grad)
    assert bool((embed_dwpe64(dx, P, keep, p)[T:] == 0).all())
    # ids -1 and V are skipped
    idx2 = idx.clone()
    idx2[0, 0], idx2[1, 2] = -1, V
    ok = ((idx2 >= 0) & (idx2 < V)).reshape(-1)
    want = torch.zeros(V, d, dtype=F64).index_add_(0, idx2.reshape(-1)[ok], dx.reshape(-1, d)[ok])
    close(embed_dwte64(dx, idx2, V), want)


# ------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("V", [8, 1000])
def test_xent64_matches_torch(V):
    g = gen(V)
    N = 6
    z = (torch.randn(N, V, generator=g, dtype=F64) * 2).requires_grad_()
    with torch.no_grad():
        z[1] = 3.0                                           # equal logits
        z[2, 3] = 40.0                                       # one dominant logit
        z[4] += 30000.0
    t = torch.randint(0, V, (N,), generator=g)
    t[3] = -1
    t[2] = 3
    loss = F.cross_entropy(z, t, reduction="none", ignore_index=-1)
    loss.sum().backward()
    got_loss, lse, dz = xent64(z.detach(), t)
    close(got_loss, loss.detach(), scale=1.0)
    close(lse, torch.logsumexp(z.detach(), -1), scale=1.0)
    close(dz, z.grad, scale=1.0)
    assert float(got_loss[3]) == 0.0 and bool((dz[3] == 0).all())
    assert abs(float(lse[1]) - (3.0 + math.log(V))) <= 1e-12
