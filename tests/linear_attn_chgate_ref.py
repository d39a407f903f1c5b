"""float64 O(T^2) definition of linear attention with per-channel decay gates (the GLA form) with autograd gradients,
and the sums that bound its kernels:
o[i] = 1 / sqrt(D) sum_{j <= i} (sum_d q[i,d] k[j,d] exp2(L[i,d] - L[j,d])) v[j], L the running sum along a row of the
log2 decays l [.., Hkv D], g = h // (Hq // Hkv); no chunking, one head at a time (the [T, T, D] weights of a head stay
under 100 MB).  The kernels are handed ``cum`` (fp32, the prefix sum of l inside each chunk of 64), so L here is rebuilt
from exactly those values.

Bound (u = 2^-8 bf16, 2^-11 fp16), elementwise |x - x_ref| <= c u A + 1e-30 with A the same sum over absolute values (the
per-channel weights inside) and c = the 16-bit roundings a term passes in the contract of csrc/linear_attn_chgate.hip,
plus 1.  The longest chains:
  o   off-diagonal sub-block: q~, k~, the score tile, the output; state term: k~ of the state product, the state, q~,
      the output: 4, c = 5  (a diagonal term passes 2)
  dq  k~, the dP tile, the output; state term: k~, the state, the output: 3, c = 4
  dk  q~, the dP tile, the output; state term: the decayed q operand, the state gradient, the output: 3, c = 4
  dv  q~, k~, the score tile, the output; state term: the decayed q operand, the state gradient, k~, the output: 4, c = 5
  dl  the suffix sum of dL = sum_h dq q - dk k per channel, both products from the fp32 accumulators: the chains of dq and
      dk without the output rounding: 2, c = 3, A_dl = suffix sum of (sum_h A_dq |q| + A_dk |k|).  ln 2 is folded away.

The gate kernels work in fp32 throughout; their bounds are fp32 ones (eps = 2^-24), built as in linear_attn_gate_ref.py:
a dot product of n terms gets (n + 2) eps times the sum of absolute products (the row dots: n_embd / 8 + 7), an input's
bound is carried through the next product, the log-sigmoid gets 4 eps (1 + |u| + |l|), a 16-bit output one u."""
import math

import torch

from linear_attn_gate_ref import C, EPS, LOG2E
from linear_attn_ref import SENTINEL, U

CB = {"o": 5.0, "dq": 4.0, "dk": 4.0, "dv": 5.0, "dl": 3.0}


def draw_cum(B, T, Hkv, D, gen):
    """fp32 [B*T, Hkv*D] chunk prefix sums of l.  Channel d of head g is of kind (d + g + T / C) % 4, so the kinds
    alternate along d inside a head: 0 no decay (l = 0 exactly), 1 typical gates, 2 gates whose exp2(cum) underflows
    inside a chunk (l in -3..-5), 3 gates of about -40 per token."""
    r = torch.rand(B, T, Hkv, D, generator=gen, dtype=torch.float64)
    kind = (torch.arange(D).view(1, D) + torch.arange(Hkv).view(Hkv, 1) + T // C) % 4
    l = torch.where(kind == 0, 0.0 * r, torch.where(kind == 1, torch.log2(torch.sigmoid(3.0 + 2.0 * (r - 0.5))),
                                                    torch.where(kind == 2, -3.0 - 2.0 * r, -40.0 - r)))
    return l.view(B, T // C, C, Hkv * D).cumsum(2).reshape(B * T, Hkv * D).float()


def row_sums(cum, B, T):
    """L [B, T, Hkv*D] in float64 from the chunk prefix sums."""
    lam = cum.detach().double().cpu().view(B, T // C, C, -1)
    tot = lam[:, :, -1].cumsum(1) - lam[:, :, -1]
    return (lam + tot[:, :, None]).reshape(B, T, -1)


def reference(q, k, v, do, L, B, T, Hq, Hkv):
    """-> {name: (value, A)} for o, dq [B*T, Hq*D], dk, dv, dl [B*T, Hkv*D]; L: float64 [B, T, Hkv*D]."""
    G, D = Hq // Hkv, q.shape[1] // Hq
    sc = 1.0 / math.sqrt(D)
    q, k, v, do = (t.detach().double().cpu().view(B, T, -1, D) for t in (q, k, v, do))
    L = L.view(B, T, Hkv, D)
    causal = torch.tril(torch.ones(T, T, dtype=torch.float64))[:, :, None]
    names = ("o", "dq", "dk", "dv", "dl")
    val = {n: torch.zeros(B, T, (Hq if n in ("o", "dq") else Hkv), D, dtype=torch.float64) for n in names}
    A = {n: torch.zeros_like(val[n]) for n in names}
    for b in range(B):
        for h in range(Hq):
            g = h // G
            qh, kh, vh, Lg = (t.clone().requires_grad_() for t in (q[b, :, h], k[b, :, g], v[b, :, g], L[b, :, g]))
            E = torch.exp2((Lg[:, None, :] - Lg[None, :, :]).clamp(max=0)) * causal          # [T, T, D]
            o = sc * torch.einsum("id,jd,ijd->ij", qh, kh, E) @ vh
            dq, dk, dv, dL = torch.autograd.grad(o, (qh, kh, vh, Lg), do[b, :, h])
            E, aq, ak, av, ado = E.detach(), q[b, :, h].abs(), k[b, :, g].abs(), v[b, :, g].abs(), do[b, :, h].abs()
            Sa, dPa = sc * torch.einsum("id,jd,ijd->ij", aq, ak, E), sc * ado @ av.t()
            Adq, Adk = torch.einsum("ij,jd,ijd->id", dPa, ak, E), torch.einsum("ij,id,ijd->jd", dPa, aq, E)
            for n, x, a, hh in (("o", o.detach(), Sa @ av, h), ("dq", dq, Adq, h), ("dk", dk, Adk, g),
                                ("dv", dv, Sa.t() @ ado, g), ("dl", dL / math.log(2.0), Adq * aq + Adk * ak, g)):
                val[n][b, :, hh] += x
                A[n][b, :, hh] += a
    for t in (val, A):
        t["dl"] = t["dl"].flip(1).cumsum(1).flip(1)
    return {n: (val[n].reshape(B * T, -1), A[n].reshape(B * T, -1)) for n in names}


def compare(got, want, dtype):
    """Every element within c u A + 1e-30; the worst ratio is printed."""
    for name, (val, A) in want.items():
        if name not in got:
            continue
        err = (got[name].detach().cpu().double() - val).abs()
        ratio = float((err / (CB[name] * U[dtype] * A + 1e-30)).max())
        print(f"{name}: max |err| / bound = {ratio:.3f}, max |err| = {float(err.max()):.3e}")
        assert got[name].shape == val.shape and bool(torch.isfinite(got[name]).all()) and ratio <= 1.0, (name, ratio)


def _dl(F_, gq, gk, Hkv, D, B, T, device, dtype):
    """The suffix sum alone: a zero up-projection and a zero bias give 1 - a = 1/2, exactly."""
    w1, w2 = torch.zeros(8, 8, device=device, dtype=dtype), torch.zeros(Hkv * D, 8, device=device, dtype=dtype)
    z1 = torch.zeros(B * T, 8, device=device)
    return F_.linear_attn_gate_bwd(gq, gk, z1, torch.zeros(Hkv, device=device), w1, None, B, T, up=w2)[2]


def check_case(F_, dtype, D, Hq, Hkv, T, device):
    """``F_.linear_attn_fwd / _bwd`` under a per-channel ``cum=`` and the suffix sum of ``F_.linear_attn_gate_bwd``
    against the reference: B = 2, strided views of a fused qkv, a fused dqkv with sentinel columns."""
    B, qd, kd = 2, Hq * D, Hkv * D
    g = torch.Generator().manual_seed(1000 * T + 10 * D + Hq)
    qkv = torch.randn(B * T, qd + 2 * kd + 8, generator=g).to(device, dtype)
    do = torch.randn(B * T, qd, generator=g).to(device, dtype)
    cum = draw_cum(B, T, Hkv, D, g).to(device)
    l2g = F_.linear_attn_log2_gamma(Hkv, device)                        # not read under cum=
    q, k, v = qkv[:, :qd], qkv[:, qd:qd + kd], qkv[:, qd + kd:qd + 2 * kd]
    want = reference(q, k, v, do, row_sums(cum, B, T), B, T, Hq, Hkv)
    assert all(bool(torch.isfinite(x).all()) for pair in want.values() for x in pair)
    got = {"o": F_.linear_attn_fwd(q, k, v, B, T, Hq, Hkv, l2g, cum=cum)}
    dqkv = torch.full_like(qkv, SENTINEL)
    got["dq"], got["dk"], got["dv"] = dqkv[:, :qd], dqkv[:, qd:qd + kd], dqkv[:, qd + kd:qd + 2 * kd]
    gq, gk = F_.linear_attn_bwd(q, k, v, do, got["dq"], got["dk"], got["dv"], B, T, Hq, Hkv, l2g, cum=cum)
    assert bool((dqkv[:, qd + 2 * kd:] == SENTINEL).all()), "columns outside dq | dk | dv were written"
    got["dl"] = _dl(F_, gq, gk, Hkv, D, B, T, device, dtype)
    compare(got, want, dtype)


def check_zero_up(F_, dtype, D, Hq, Hkv, T, device, R=8):
    """A zero up-projection: ``gate_fwd``'s cum, then o and the gradients, against the float64 form with the RetNet
    decays gamma_g on every channel of head g."""
    B, d, qd, kd = 2, 128, Hq * D, Hkv * D
    g = torch.Generator().manual_seed(T + D)
    xn = torch.randn(B * T, d, generator=g).to(device, dtype)
    qkv = torch.randn(B * T, qd + 2 * kd, generator=g).to(device, dtype)
    do = torch.randn(B * T, qd, generator=g).to(device, dtype)
    w1 = (0.1 * torch.randn(R, d, generator=g)).to(device, dtype)
    z1, cum = F_.linear_attn_gate_fwd(xn, w1, F_.linear_attn_gate_bias(Hkv, device), B, T,
                                      up=torch.zeros(kd, R, device=device, dtype=dtype))
    q, k, v = qkv[:, :qd], qkv[:, qd:qd + kd], qkv[:, qd + kd:]
    l2g = F_.linear_attn_log2_gamma(Hkv, device)
    L = (torch.arange(1, T + 1, dtype=torch.float64).view(1, T, 1) * l2g.double().cpu().repeat_interleave(D))
    want = reference(q, k, v, do, L.expand(B, T, kd).contiguous(), B, T, Hq, Hkv)
    got = {"o": F_.linear_attn_fwd(q, k, v, B, T, Hq, Hkv, l2g, cum=cum)}
    got["dq"], got["dk"], got["dv"] = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    F_.linear_attn_bwd(q, k, v, do, got["dq"], got["dk"], got["dv"], B, T, Hq, Hkv, l2g, cum=cum)
    compare(got, want, dtype)


def _within(name, got, ref_, tol):
    ratio = float(((got.double().cpu() - ref_).abs() / (tol + 1e-30)).max())
    print(f"{name}: max |err| / bound = {ratio:.3f}")
    assert got.shape == ref_.shape and bool(torch.isfinite(got).all()) and ratio <= 1.0, (name, ratio)


def check_gate_kernels(F_, dtype, R, Hkv, device, D=64, d=128, T=2 * C, B=2, G=2):
    """``gate_fwd``'s z1 and cum and ``gate_bwd``'s dl, dz, dz1, dW2 and in-place dxn against float64 under the fp32
    bounds of the module docstring."""
    g = torch.Generator().manual_seed(10 * R + Hkv)
    kvd, N = Hkv * D, B * T
    xn = torch.randn(N, d, generator=g).to(device, dtype)
    w1 = (0.1 * torch.randn(R, d, generator=g)).to(device, dtype)
    w2 = (0.5 * torch.randn(kvd, R, generator=g)).to(device, dtype)
    bias = F_.linear_attn_gate_bias(Hkv).to(device)
    z1, cum = F_.linear_attn_gate_fwd(xn, w1, bias, B, T, up=w2)
    x64, a64, u64 = xn.double().cpu(), w1.double().cpu(), w2.double().cpu()
    b64 = bias.double().cpu().repeat_interleave(D)
    z164 = x64 @ a64.t()
    tz1 = (d / 8 + 7) * EPS * (x64.abs() @ a64.abs().t())
    z64 = z164 @ u64.t()
    tz = tz1 @ u64.abs().t() + (R + 2) * EPS * (z164.abs() @ u64.abs().t())
    u = (z64 + b64) * LOG2E
    l64 = torch.minimum(u, torch.zeros_like(u)) - torch.log2(1 + torch.exp2(-u.abs()))
    tl = LOG2E * tz + 4 * EPS * (1 + u.abs() + l64.abs())
    chunk_sum = lambda t: t.view(B, T // C, C, kvd).cumsum(2).reshape(N, kvd)  # noqa: E731
    _within("z1", z1, z164, tz1)
    _within("cum", cum, chunk_sum(l64), chunk_sum(tl) + C * EPS * chunk_sum(l64.abs()))

    gq = torch.randn(N, Hkv * G * D, generator=g).to(device)
    gk = torch.randn(N, kvd, generator=g).to(device)
    dxn = torch.randn(N, d, generator=g).to(device, dtype)
    dw2 = torch.randn(kvd, R, generator=g).to(device, dtype)
    dx0, dw0 = dxn.double().cpu(), dw2.double().cpu()
    dz1, dz, dl = F_.linear_attn_gate_bwd(gq, gk, z1, bias, w1, dxn, B, T, up=w2, dup=dw2, accumulate=True)
    q64, k64 = gq.double().cpu().view(B, T, Hkv, G, D), gk.double().cpu().view(B, T, Hkv, D)
    suffix = lambda t: t.flip(1).cumsum(1).flip(1).reshape(N, kvd)  # noqa: E731
    dl64, adl = suffix(q64.sum(3) - k64), suffix(q64.abs().sum(3) + k64.abs())
    tdl = (T + G + 2) * EPS * adl
    zk = z1.double().cpu()                                              # a is rebuilt from the kept fp32 z1
    zb = zk @ u64.t() + b64
    om = 1.0 - torch.sigmoid(zb)
    tom = 0.25 * (R + 2) * EPS * (zk.abs() @ u64.abs().t()) + 4 * EPS * (om + EPS * zb.abs())
    dz64 = dl64 * om
    tdz = tdl * om + dl64.abs() * tom + 2 * EPS * dz64.abs()
    dz164 = dz64 @ u64
    tdz1 = tdz @ u64.abs() + (kvd + 2) * EPS * (dz64.abs() @ u64.abs())
    dw64 = dw0 + dz64.t() @ zk
    tdw = U[dtype] * dw64.abs() + tdz.t() @ zk.abs() + (N + 3) * EPS * (dw0.abs() + dz64.abs().t() @ zk.abs())
    dx64 = dx0 + dz164 @ a64
    tdx = U[dtype] * dx64.abs() + tdz1 @ a64.abs() + (R + 2) * EPS * (dx0.abs() + dz164.abs() @ a64.abs())
    for name, got, ref_, tol in (("dl", dl, dl64, tdl), ("dz", dz, dz64, tdz), ("dz1", dz1, dz164, tdz1),
                                 ("dW2", dw2, dw64, tdw), ("dxn", dxn, dx64, tdx)):
        _within(name, got, ref_, tol)
