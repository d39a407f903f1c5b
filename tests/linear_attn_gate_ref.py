"""float64 O(T^2) definition of gated linear attention with autograd gradients, and the sums that bound its kernels:
o[i] = 1 / sqrt(D) sum_{j <= i} exp2(L[i] - L[j]) (q[i] . k[j]) v[j], L the running sum along a row of the log2 decays l,
g = h // (Hq // Hkv); no chunking.  The kernels are handed ``cum`` (fp32, the prefix sum of l inside each chunk of 64), so
L here is rebuilt from exactly those values.

Bound (u = 2^-8 bf16, 2^-11 fp16), elementwise |x - x_ref| <= c u A + 1e-30 with A the same sum over absolute values and
c = the 16-bit roundings a term passes in the contract + 1: c = 3 for o, dq, dk, dv as in linear_attn_ref.py.  dl is the
suffix sum of dL = sum_h dq . q - dk . k with both dots taken from the fp32 accumulators, so a term of it passes no
output rounding: an intra-chunk term passes one (the decayed score tile), an inter-chunk term two (the decayed V / dO
operand of the state product, then the state), so c = 2 + 1 = 3 for dl too, with
A_dl = suffix sum of (sum_h sum_d A_dq |q| + sum_d A_dk |k|).  ln 2 is folded away: dl is the gradient with respect to
l ln 2.

The gate kernels work in fp32 throughout; their bounds are fp32 ones (eps = 2^-24): z from a chain of n_embd / 8
multiply-adds per lane and a six-level wave reduction, l from z through a few correctly rounded steps and two
transcendental instructions (2^-22 absolute each at most), cum and dl from sequential sums of at most 64 and T terms."""
import math

import torch

from linear_attn_ref import SENTINEL, U, _heads

C = 64
EPS = 2.0 ** -24
LOG2E = math.log2(math.e)


def draw_cum(B, T, Hq, Hkv, gen):
    """fp32 [B*T, Hkv] chunk prefix sums of l; head g of a case is of kind (g + T / C + Hq / 2) % 3: 0 no decay (l = 0
    exactly), 1 typical gates, 2 gates so strong that exp2(cum) underflows inside a chunk."""
    l = torch.empty(B, T, Hkv, dtype=torch.float64)
    for g in range(Hkv):
        kind = (g + T // C + Hq // 2) % 3
        r = torch.rand(B, T, generator=gen, dtype=torch.float64)
        l[:, :, g] = (0.0 * r, torch.log2(torch.sigmoid(3.0 + 2.0 * (r - 0.5))), -3.0 - 2.0 * r)[kind]
    return l.view(B, T // C, C, Hkv).cumsum(2).reshape(B * T, Hkv).float()


def row_sums(cum, B, T):
    """L [B, T, Hkv] in float64 from the chunk prefix sums."""
    lam = cum.detach().double().cpu().view(B, T // C, C, -1)
    tot = lam[:, :, -1].cumsum(1) - lam[:, :, -1]
    return (lam + tot[:, :, None]).reshape(B, T, -1)


def reference(q, k, v, do, L, B, T, Hq, Hkv):
    """-> {name: (value, A)} for o, dq, dk, dv [B*T, H*D] and dl [B*T, Hkv]; L: float64 [B, T, Hkv]."""
    G, D = Hq // Hkv, q.shape[1] // Hq
    q, k, v, do = (t.cpu() for t in (q, k, v, do))
    Lh = L.transpose(1, 2).repeat_interleave(G, 1).requires_grad_()              # [B, Hq, T]
    i = torch.arange(T)
    W = torch.where(i[:, None] >= i[None, :], torch.exp2((Lh[..., :, None] - Lh[..., None, :]).clamp(max=0)),
                    torch.zeros((), dtype=torch.float64)) / math.sqrt(D)
    qh, doh = _heads(q, B, T, Hq).requires_grad_(), _heads(do, B, T, Hq)
    kh, vh = _heads(k, B, T, Hkv, G).requires_grad_(), _heads(v, B, T, Hkv, G).requires_grad_()
    o = (W * (qh @ kh.transpose(-1, -2))) @ vh
    dq, dk, dv, dL = torch.autograd.grad(o, (qh, kh, vh, Lh), doh)
    aq, ak, av, ado = qh.detach().abs(), kh.detach().abs(), vh.detach().abs(), doh.abs()
    Wd = W.detach()
    Ws, Wd = Wd * (aq @ ak.transpose(-1, -2)), Wd * (ado @ av.transpose(-1, -2))
    Adq, Adk = Wd @ ak, Wd.transpose(-1, -2) @ aq

    def rows(t, grouped):                                               # [B, H, T, .] -> [B*T, H*.]
        if grouped:
            t = t.reshape(B, Hkv, G, *t.shape[2:]).sum(2)
        return t.transpose(1, 2).reshape(B * T, -1)

    def suffix(t):                                                      # [B*T, Hkv]: sum over the later rows of a row
        return t.view(B, T, Hkv).flip(1).cumsum(1).flip(1).reshape(B * T, Hkv)

    return {"o": (rows(o.detach(), False), rows(Ws @ av, False)),
            "dq": (rows(dq, False), rows(Adq, False)),
            "dk": (rows(dk, True), rows(Adk, True)),
            "dv": (rows(dv, True), rows(Ws.transpose(-1, -2) @ ado, True)),
            "dl": (suffix(rows(dL[..., None] / math.log(2.0), True)),
                   suffix(rows((Adq * aq + Adk * ak).sum(-1, keepdim=True), True)))}


def compare(got, want, dtype):
    """Every element within 3 u A + 1e-30; the worst ratio is printed."""
    for name, (val, A) in want.items():
        if name not in got:
            continue
        err = (got[name].detach().cpu().double() - val).abs()
        ratio = float((err / (3.0 * U[dtype] * A + 1e-30)).max())
        print(f"{name}: max |err| / bound = {ratio:.3f}, max |err| = {float(err.max()):.3e}")
        assert got[name].shape == val.shape and bool(torch.isfinite(got[name]).all()) and ratio <= 1.0, (name, ratio)


def check_case(F_, dtype, D, Hq, Hkv, T, device):
    """``F_.linear_attn_fwd / _bwd`` under ``cum=`` and the suffix sum of ``F_.linear_attn_gate_bwd`` against the
    reference: B = 2, strided views of a fused qkv, a fused dqkv with sentinel columns."""
    B, qd, kd = 2, Hq * D, Hkv * D
    g = torch.Generator().manual_seed(1000 * T + 10 * D + Hq)
    qkv = torch.randn(B * T, qd + 2 * kd + 8, generator=g).to(device, dtype)
    do = torch.randn(B * T, qd, generator=g).to(device, dtype)
    cum = draw_cum(B, T, Hq, Hkv, g).to(device)
    l2g = F_.linear_attn_log2_gamma(Hkv, device)                        # not read under cum=
    q, k, v = qkv[:, :qd], qkv[:, qd:qd + kd], qkv[:, qd + kd:qd + 2 * kd]
    want = reference(q, k, v, do, row_sums(cum, B, T), B, T, Hq, Hkv)
    got = {"o": F_.linear_attn_fwd(q, k, v, B, T, Hq, Hkv, l2g, cum=cum)}
    dqkv = torch.full_like(qkv, SENTINEL)
    got["dq"], got["dk"], got["dv"] = dqkv[:, :qd], dqkv[:, qd:qd + kd], dqkv[:, qd + kd:qd + 2 * kd]
    gq, gk = F_.linear_attn_bwd(q, k, v, do, got["dq"], got["dk"], got["dv"], B, T, Hq, Hkv, l2g, cum=cum)
    assert bool((dqkv[:, qd + 2 * kd:] == SENTINEL).all()), "columns outside dq | dk | dv were written"
    wg = torch.zeros(Hkv, 8, device=device, dtype=dtype)                # z None: the suffix sum alone, wg for its shape
    got["dl"] = F_.linear_attn_gate_bwd(gq, gk, None, torch.zeros(Hkv, device=device), wg, None, B, T)
    compare(got, want, dtype)


def check_zero_gate(F_, dtype, D, Hq, Hkv, T, device):
    """A zero gate weight: ``gate_fwd``'s cum, then the gated forward, against the float64 fixed-decay form with the
    schedule's gamma_g and r = 1."""
    B, d, qd, kd = 2, 128, Hq * D, Hkv * D
    g = torch.Generator().manual_seed(T + D)
    xn = torch.randn(B * T, d, generator=g).to(device, dtype)
    qkv = torch.randn(B * T, qd + 2 * kd, generator=g).to(device, dtype)
    z, cum = F_.linear_attn_gate_fwd(xn, torch.zeros(Hkv, d, device=device, dtype=dtype),
                                     F_.linear_attn_gate_bias(Hkv, device), B, T)
    assert not z.any()
    q, k, v = qkv[:, :qd], qkv[:, qd:qd + kd], qkv[:, qd + kd:]
    l2g = F_.linear_attn_log2_gamma(Hkv, device)
    L = (torch.arange(1, T + 1, dtype=torch.float64).view(1, T, 1) * l2g.double().cpu()).expand(B, T, Hkv)
    want = reference(q, k, v, torch.zeros_like(q), L, B, T, Hq, Hkv)
    compare({"o": F_.linear_attn_fwd(q, k, v, B, T, Hq, Hkv, l2g, cum=cum)}, {"o": want["o"]}, dtype)


def check_gate_kernels(F_, dtype, Hkv, device, d=128, T=2 * C, B=2, G=2):
    """``gate_fwd``'s z and cum and ``gate_bwd``'s dz and in-place dxn against float64 under the fp32 bounds of the
    module docstring.  Rows 0 and 1 carry z + b = +60 and -60 (up to the 16-bit rounding of xn) on head 0."""
    g = torch.Generator().manual_seed(Hkv)
    xn = torch.randn(B * T, d, generator=g)
    wg = 0.1 * torch.randn(Hkv, d, generator=g)
    bias = F_.linear_attn_gate_bias(Hkv)
    for r, t in ((0, 60.0), (1, -60.0)):
        xn[r] = wg[0] * (t - float(bias[0])) / float(wg[0] @ wg[0])
    xn, wg, bias = xn.to(device, dtype), wg.to(device, dtype), bias.to(device)
    z, cum = F_.linear_attn_gate_fwd(xn, wg, bias, B, T)
    x64, w64, b64 = xn.double().cpu(), wg.double().cpu(), bias.double().cpu()
    z64 = x64 @ w64.t()
    tz = (d / 8 + 7) * EPS * (x64.abs() @ w64.abs().t())
    u = (z64 + b64) * LOG2E
    l64 = torch.minimum(u, torch.zeros_like(u)) - torch.log2(1 + torch.exp2(-u.abs()))
    tl = LOG2E * tz + 4 * EPS * (1 + u.abs() + l64.abs())
    chunk_sum = lambda t: t.view(B, T // C, C, Hkv).cumsum(2).reshape(B * T, Hkv)  # noqa: E731
    tc = chunk_sum(tl) + C * EPS * chunk_sum(l64.abs())
    for name, got, ref_, tol in (("z", z, z64, tz), ("cum", cum, chunk_sum(l64), tc)):
        ratio = float(((got.double().cpu() - ref_).abs() / (tol + 1e-30)).max())
        print(f"{name}: max |err| / bound = {ratio:.3f}")
        assert bool(torch.isfinite(got).all()) and ratio <= 1.0, (name, ratio)
    assert 55.0 < float(z[0, 0] + bias[0]) < 65.0 and -65.0 < float(z[1, 0] + bias[0]) < -55.0

    gq = torch.randn(B * T, Hkv * G, generator=g).to(device)
    gk = torch.randn(B * T, Hkv, generator=g).to(device)
    dxn = torch.randn(B * T, d, generator=g).to(device, dtype)
    dx0 = dxn.double().cpu()
    dz = F_.linear_attn_gate_bwd(gq, gk, z, bias, wg, dxn, B, T)
    q64, k64 = gq.double().cpu().view(B, T, Hkv, G), gk.double().cpu().view(B, T, Hkv)
    suffix = lambda t: t.flip(1).cumsum(1).flip(1).reshape(B * T, Hkv)  # noqa: E731
    dl64, adl = suffix(q64.sum(-1) - k64), suffix(q64.abs().sum(-1) + k64.abs())
    om = 1.0 - torch.sigmoid(z.double().cpu() + b64)                    # a is rebuilt from the kept fp32 z
    tdz = (T + G + 2) * EPS * adl * om + 4 * EPS * dl64.abs()           # the sums; 1 - a, formed in fp32
    dz64 = dl64 * om
    dx64 = dx0 + dz64 @ w64
    tdx = U[dtype] * dx64.abs() + tdz @ w64.abs() + (Hkv + 2) * EPS * (dx0.abs() + dz64.abs() @ w64.abs())
    for name, got, ref_, tol in (("dz", dz, dz64, tdz), ("dxn", dxn, dx64, tdx)):
        ratio = float(((got.double().cpu() - ref_).abs() / (tol + 1e-30)).max())
        print(f"{name}: max |err| / bound = {ratio:.3f}")
        assert bool(torch.isfinite(got).all()) and ratio <= 1.0, (name, ratio)
    assert float(dz[0, 0]) == 0.0 and float(dz[1, 0]) != 0.0            # 1 - a rounds to 0 at +60, to 1 at -60
