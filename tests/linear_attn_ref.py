"""float64 O(T^2) definition of fixed-decay linear attention, autograd gradients, and the sums that bound its kernels:
o[i] = r[g,i] / sqrt(D) sum_{j <= i} gamma_g^(i-j) (q[i] . k[j]) v[j], gamma_g = 2^log2_gamma[g],
r[g,i] = sqrt((1 - gamma_g) / (1 - gamma_g^(i+1))), g = h // (Hq // Hkv).  Bound (u = 2^-8 bf16, 2^-11 fp16): two 16-bit
roundings per term plus one unit for the fp32 work, |x - x_ref| <= 3 u A + 1e-30 elementwise, A the same sum of absolute
values."""
import math

import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SENTINEL = 77.0


def _heads(t, B, T, H, rep=1):
    t = t.detach().double().reshape(B, T, H, -1).transpose(1, 2)      # [B, H, T, D]
    return t.repeat_interleave(rep, dim=1) if rep > 1 else t


def weights(T, Hq, Hkv, D, log2_gamma):
    """W[h, i, j] = r[g,i] scale gamma_g^(i-j) for j <= i, else 0 (float64)."""
    l2g = log2_gamma.detach().double().cpu().repeat_interleave(Hq // Hkv).view(Hq, 1, 1)
    i = torch.arange(T, dtype=torch.float64)
    diff = (i[:, None] - i[None, :]).clamp(min=0)
    r = torch.sqrt(torch.expm1(l2g * math.log(2.0)) / torch.expm1(l2g * (i + 1).view(1, T, 1) * math.log(2.0)))
    return torch.where(i[:, None] >= i[None, :], torch.exp2(l2g * diff), torch.zeros((), dtype=torch.float64)) \
        * r / math.sqrt(D)


def reference(q, k, v, do, B, T, Hq, Hkv, log2_gamma):
    """q / do [B*T, Hq*D], k / v [B*T, Hkv*D] (16-bit, any strides) -> {name: (value, A)} for o, dq, dk, dv."""
    G, D = Hq // Hkv, q.shape[1] // Hq
    q, k, v, do = (t.cpu() for t in (q, k, v, do))
    W = weights(T, Hq, Hkv, D, log2_gamma)
    qh, doh = _heads(q, B, T, Hq).requires_grad_(), _heads(do, B, T, Hq)
    kh, vh = _heads(k, B, T, Hkv, G).requires_grad_(), _heads(v, B, T, Hkv, G).requires_grad_()
    o = (W * (qh @ kh.transpose(-1, -2))) @ vh
    dq, dk, dv = torch.autograd.grad(o, (qh, kh, vh), doh)
    aq, ak, av, ado = qh.detach().abs(), kh.detach().abs(), vh.detach().abs(), doh.abs()
    Ws, Wd = W * (aq @ ak.transpose(-1, -2)), W * (ado @ av.transpose(-1, -2))

    def rows(t, grouped):                                               # [B, H, T, D] -> [B*T, H*D]
        if grouped:
            t = t.reshape(B, Hkv, G, T, D).sum(2)
        return t.transpose(1, 2).reshape(B * T, -1)

    return {"o": (rows(o.detach(), False), rows(Ws @ av, False)),
            "dq": (rows(dq, False), rows(Wd @ ak, False)),
            "dk": (rows(dk, True), rows(Wd.transpose(-1, -2) @ aq, True)),
            "dv": (rows(dv, True), rows(Ws.transpose(-1, -2) @ ado, True))}


def check_case(F_, dtype, D, Hq, Hkv, T, device):
    """``F_.linear_attn_fwd / _bwd`` against the reference: B = 2, strided views of a fused qkv, a fused dqkv with sentinel
    columns.  Hkv > 1: the schedule (its fastest decay); Hkv = 1: the slowest, 1 - 2^-12, so no inter-chunk term hides."""
    B, qd, kd = 2, Hq * D, Hkv * D
    g = torch.Generator(device).manual_seed(1000 * T + 10 * D + Hq)
    qkv = torch.randn(B * T, qd + 2 * kd + 8, device=device, generator=g).to(dtype)
    do = torch.randn(B * T, qd, device=device, generator=g).to(dtype)
    l2g = F_.linear_attn_log2_gamma(Hkv, device) if Hkv > 1 else torch.log2(torch.tensor([1 - 2.0 ** -12], device=device))
    q, k, v = qkv[:, :qd], qkv[:, qd:qd + kd], qkv[:, qd + kd:qd + 2 * kd]
    want = reference(q, k, v, do, B, T, Hq, Hkv, l2g)
    got = {"o": F_.linear_attn_fwd(q, k, v, B, T, Hq, Hkv, l2g)}
    o_out = torch.full_like(got["o"], SENTINEL)
    assert F_.linear_attn_fwd(q, k, v, B, T, Hq, Hkv, l2g, o_out=o_out) is o_out and torch.equal(got["o"], o_out)
    dqkv = torch.full_like(qkv, SENTINEL)
    got["dq"], got["dk"], got["dv"] = dqkv[:, :qd], dqkv[:, qd:qd + kd], dqkv[:, qd + kd:qd + 2 * kd]
    F_.linear_attn_bwd(q, k, v, do, got["dq"], got["dk"], got["dv"], B, T, Hq, Hkv, l2g)
    assert bool((dqkv[:, qd + 2 * kd:] == SENTINEL).all()), "columns outside dq | dk | dv were written"
    for name, (val, A) in want.items():            # every element within 3 u A + 1e-30; the worst ratio is printed
        err = (got[name].detach().cpu().double() - val).abs()
        ratio = float((err / (3.0 * U[dtype] * A + 1e-30)).max())
        print(f"{name}: max |err| / bound = {ratio:.3f}, max |err| = {float(err.max()):.3e}")
        assert got[name].shape == val.shape and bool(torch.isfinite(got[name]).all()) and ratio <= 1.0, (name, ratio)
