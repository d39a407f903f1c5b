"""The auxiliary router losses of the mixture-of-experts FFN on the MI355X: ``moe_aux_fwd``, ``moe_aux_bwd_`` and the
dense router weight-gradient kernel of csrc/moe.hip against float64 with bounds derived from the number formats,
determinism, HIP-graph replay, the layer and the model against the float64 / CPU paths, and the strategies, fp16,
two ranks, ``--strict-kernels`` and the harness record with the flags on.  (The formulas against autograd:
tests/test_moe_aux_cpu.py.)  Helpers and tolerances are those of tests/test_moe_gpu.py."""
import copy
import json
import math
import os

import pytest
import torch

import dltb
from dltb.models import build_model, get_model_config
from dltb.models import mistral
from dltb.ops import functional as F_
from dltb.ops import ref
from dltb.parallel import GraphedStep, ParamRuntime, engine_config, make_engine
from multirank_util import compare, run
import test_moe_gpu as base

pytestmark = pytest.mark.gpu
DEV = "cuda"
U32 = base.U32
DTYPES, IDS, TOL = base.DTYPES, base.IDS, base.TOL
A, B = 0.01, 0.001
SHAPES = [(1, 2), (63, 64), (200, 5), (200, 8), (1030, 7), (4100, 64)]
K_OF = {2: 1, 5: 2, 7: 2, 8: 2, 64: 4}
kcase = base.kcase                   # the module fixture of tests/test_moe_gpu.py: N = 200, d = 128, E = 8, K = 2, drops


# ------------------------------------------------------------------------------------------- inputs and bounds
def _inputs(N, E, shift=0.0):
    """Random fp32 logits of spread 2 (plus ``shift``) and counts of N K assignments with experts nobody chose."""
    gen = torch.Generator().manual_seed(1000 * N + E)
    logits = (2.0 * torch.randn(N, E, generator=gen) + shift).float()
    K = K_OF[E]
    w = torch.rand(E, generator=gen) + 0.05
    w[E - 1] = 0.0
    if E > 4:
        w[1] = 0.0
    counts = torch.bincount(torch.multinomial(w, N * K, replacement=True, generator=gen), minlength=E).to(torch.int32)
    assert int(counts.sum()) == N * K and int(counts.min()) == 0
    return logits, counts, K


def lse_bound(lse64, E):
    """|lse| 4 u32 (one logf at twice HIP's documented 2 ulp, the last add) plus (E + 2) u32: the relative error of
    the sum of E exp() results (4 u32 each, an E-term fp32 sum) is the absolute error of its logarithm."""
    return lse64.abs() * 4 * U32 + (E + 2) * U32


def half_ulp32(v):
    """Half a unit in the last place of fp32 at magnitude ``v`` (float64 tensor)."""
    return torch.pow(2.0, torch.floor(torch.log2(v.clamp(min=2.0 ** -126))) - 24)


def fwd_bounds(logits, counts, K):
    """float64 (lse, balance, z) of fp32 ``logits`` and the bounds on the fp32 results.  balance and z: exactly the
    form of tests/test_moe_gpu.py ``bound`` with an fp32 result -- (n + 1) u32 on the summed magnitude for n = N + E
    fp32 operations (both sums have positive terms only, so that magnitude is the value), 4 u32 more on it for the
    exp() behind every term, and half an fp32 ulp at the error-widened magnitude for the result's rounding.  Nothing
    is added for z's use of the kernel's own rounded lse."""
    N, E = logits.shape
    lse, out = ref.moe_aux_fwd(logits.double(), counts, K)
    b_lse = lse_bound(lse, E)
    acc = (N + E + 1 + 4) * U32 * out
    b = acc + half_ulp32(out.abs() + acc)
    return lse, out, b_lse, b[0], b[1]


def check_fwd(got_lse, got_out, logits, counts, K, what):
    lse, out, b_lse, b_bal, b_z = fwd_bounds(logits, counts, K)
    r_lse = ((got_lse.double().cpu() - lse).abs() / b_lse).max().item()
    r_bal = (abs(got_out[0].double().item() - out[0].item()) / b_bal).item()
    r_z = (abs(got_out[1].double().item() - out[1].item()) / b_z).item()
    print(f"{what}: max err / bound: lse {r_lse:.3f} balance {r_bal:.3f} z {r_z:.3f}")
    assert r_lse <= 1.0 and r_bal <= 1.0 and r_z <= 1.0, (what, r_lse, r_bal, r_z)


def term64(logits, lse, counts, g, K):
    """The added gradient in float64 from fp32 ``logits`` and ``lse``, and its bound: p = exp(logits - lse) carries
    the exp()'s 4 u32 and the rounding of its argument, |logits - lse| u32; the row dot is a 64-lane butterfly of
    E products (7 operations on positive terms); f, the two factors and the rest are at most 17 operations more --
    (24 + 4 + |logits - lse|) u32 on the summed magnitudes of the element."""
    N, E = logits.shape
    lg, l = logits.double(), lse.double()[:, None]
    p = torch.exp(lg - l)
    f = counts.double() / (N * K)
    dot = (f * p).sum(-1, keepdim=True)
    g = g.double()
    want = g[0] * (E / N) * p * (f - dot) + g[1] * (2.0 / N) * l * p
    mag = g[0].abs() * (E / N) * p * (f + dot) + g[1].abs() * (2.0 / N) * l.abs() * p
    return want, (28 + (lg - l).abs()) * U32 * mag


# ------------------------------------------------------------------------------------------- moe_aux_fwd
@pytest.mark.parametrize("N,E", SHAPES)
def test_aux_fwd_against_float64(N, E):
    for shift in (0.0, 80.0, -80.0):
        logits, counts, K = _inputs(N, E, shift)
        row = torch.full((2,), float("nan"), device=DEV)
        lse, out = F_.moe_aux_fwd(logits.to(DEV), counts.to(DEV), K, row)
        torch.cuda.synchronize()
        assert lse.shape == (N,) and out.shape == (2,) and lse.dtype == out.dtype == torch.float32
        assert torch.equal(row, out)                         # the record row gets the same bits
        check_fwd(lse, out, logits, counts, K, f"aux_fwd N={N} E={E} shift={shift}")
    # the max-subtraction: a shifted row's lse is the shift plus the unshifted one
    logits, counts, K = _inputs(N, E, 0.0)
    l0 = F_.moe_aux_fwd(logits.to(DEV), counts.to(DEV), K)[0].double().cpu()
    l1 = F_.moe_aux_fwd((logits.double() + 80.0).float().to(DEV), counts.to(DEV), K)[0].double().cpu()
    assert torch.isfinite(l1).all() and float((l1 - 80.0 - l0).abs().max()) < 1e-4


def test_aux_fwd_known_values():
    E, K, N = 8, 2, 200
    counts = torch.full((E,), N * K // E, dtype=torch.int32, device=DEV)
    _, out = F_.moe_aux_fwd(torch.zeros(N, E, device=DEV), counts, K)
    assert abs(out[0].item() - 1.0) < 1e-6 and abs(out[1].item() - math.log(E) ** 2) < 1e-5
    logits = torch.zeros(N, E, device=DEV)
    logits[:, 3] = 40.0
    counts = torch.zeros(E, dtype=torch.int32, device=DEV)
    counts[3] = N * K
    _, out = F_.moe_aux_fwd(logits, counts, K)
    assert abs(out[0].item() - E) < 1e-4 and abs(out[1].item() - 1600.0) < 1e-2


# ------------------------------------------------------------------------------------------- moe_aux_bwd_
@pytest.mark.parametrize("N,E", SHAPES)
def test_aux_bwd_against_float64(N, E):
    g = torch.tensor([0.7, -1.3])
    for shift in (0.0, 80.0, -80.0):
        logits, counts, K = _inputs(N, E, shift)
        lg, ct = logits.to(DEV), counts.to(DEV)
        lse, _ = F_.moe_aux_fwd(lg, ct, K)
        got = F_.moe_aux_bwd_(torch.zeros(N, E, device=DEV), lg, lse, ct, g.to(DEV), K)
        want, b = term64(logits, lse.cpu(), counts, g, K)
        err = (got.double().cpu() - want).abs()
        worst = (err / b.clamp(min=1e-300)).max().item()
        print(f"aux_bwd N={N} E={E} shift={shift}: max err / bound = {worst:.3f}")
        assert worst <= 1.0 and float(want.abs().max()) > 0
        # scaling by a power of two (the fp16 loss scale) is exact
        big = F_.moe_aux_bwd_(torch.zeros(N, E, device=DEV), lg, lse, ct, (g * 1024.0).to(DEV), K)
        assert torch.equal(big, got * 1024.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_aux_bwd_adds_to_the_sparse_dlogits(kcase, dtype):
    N, E, K = kcase["N"], kcase["E"], kcase["K"]
    h, wr, expert, gate, slot, src = base._routed(kcase, dtype)
    _, _, logits = F_.moe_route(h, wr, K)
    counts = F_.moe_assign(expert, E, kcase["C"])[3]
    ye, dm = kcase["ye"].to(DEV, dtype), kcase["dm"].to(DEV, dtype)
    _, _, sparse = F_.moe_combine_bwd(dm, ye, slot, src, expert, gate, E)
    assert float((sparse == 0).float().mean()) >= (E - K) / E
    lse, _ = F_.moe_aux_fwd(logits, counts, K)
    g = torch.tensor([0.7, -1.3], device=DEV)
    term = F_.moe_aux_bwd_(torch.zeros_like(sparse), logits, lse, counts, g, K)
    got = F_.moe_aux_bwd_(sparse.clone(), logits, lse, counts, g, K)
    exact = sparse.double() + term.double()
    assert ((got.double() - exact).abs() <= U32 * exact.abs()).all()        # one fp32 add
    assert (got != 0).all()                                                  # dense now


# ------------------------------------------------------------------------------------------- dense router wgrad
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("E", [2, 5, 8, 64])
def test_dense_router_wgrad_against_float64(E, dtype):
    for d in (64, 576, 1088):
        for N in (1, 200, 1030):
            gen = torch.Generator().manual_seed(E * 10000 + d + N)
            h = torch.randn(N, d, generator=gen).to(dtype)
            dl = torch.randn(N, E, generator=gen)
            want = dl.double().t() @ h.double()
            mag = dl.double().abs().t() @ h.double().abs()
            hg, dlg = h.to(DEV), dl.to(DEV)
            dwr = torch.full((E, d), float("nan"), device=DEV, dtype=dtype)
            F_.moe_router_wgrad(dlg, hg, dwr, False, dense=True)
            base.check(dwr, want, mag, N, dtype, f"dense router_wgrad E={E} d={d} N={N}")
            first = dwr.clone()
            F_.moe_router_wgrad(dlg, hg, dwr, True, dense=True)
            base.check(dwr, want + first.double().cpu(), mag + first.double().cpu().abs(), N + 1, dtype,
                       f"dense router_wgrad accumulate E={E} d={d} N={N}")
            # on a sparse dlogits the two kernels agree within the sum of their bounds
            keep = torch.rand(N, E, generator=gen) < 0.25
            sp = torch.where(keep, dl, torch.zeros(()))
            a = torch.full((E, d), float("nan"), device=DEV, dtype=dtype)
            b = torch.full((E, d), float("nan"), device=DEV, dtype=dtype)
            F_.moe_router_wgrad(sp.to(DEV), hg, a, False, dense=True)
            F_.moe_router_wgrad(sp.to(DEV), hg, b, False)
            w_sp = sp.double().t() @ h.double()
            m_sp = sp.double().abs().t() @ h.double().abs()
            both = 2 * base.bound(w_sp, m_sp, N, dtype)
            assert ((a.double().cpu() - b.double().cpu()).abs() <= both).all(), (E, d, N)
            base.check(a, w_sp, m_sp, N, dtype, f"dense router_wgrad on sparse E={E} d={d} N={N}")


# ------------------------------------------------------------------------------------------- determinism, graphs
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_new_kernels_are_deterministic(dtype):
    N, E, d = 4100, 64, 576
    logits, counts, K = _inputs(N, E)
    gen = torch.Generator().manual_seed(3)
    h = torch.randn(N, d, generator=gen).to(DEV, dtype)
    g = torch.tensor([0.7, -1.3], device=DEV)

    def once():
        lg, ct = logits.to(DEV), counts.to(DEV)
        lse, out = F_.moe_aux_fwd(lg, ct, K)
        dl = F_.moe_aux_bwd_(torch.zeros(N, E, device=DEV), lg, lse, ct, g, K)
        dwr = torch.empty(E, d, device=DEV, dtype=dtype)
        F_.moe_router_wgrad(dl, h, dwr, False, dense=True)
        return [t.cpu() for t in (lse, out, dl, dwr)]

    for i, (x, y) in enumerate(zip(once(), once())):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), i


def _train(strategy, graphed, dtype=None, steps=6, accum=2, T=128, same_batch=False, E=8, K=2, a=A, b=B):
    torch.manual_seed(0)
    cfg = get_model_config("mtiny", T)
    cfg.n_experts, cfg.moe_top_k, cfg.moe_aux_loss_coef, cfg.moe_z_loss_coef = E, K, a, b
    cfg.validate()
    with torch.device(DEV):
        model = build_model(cfg)
    kw = {} if dtype is None else {"compute_dtype": dtype}
    eng = make_engine(model, engine_config(strategy, accum, "reference", **kw), "cuda:0")
    eng.train()
    g = torch.Generator(device=DEV).manual_seed(1)
    runner = GraphedStep(eng) if graphed else None
    losses, aux = [], []
    idx = None
    for _ in range(steps):
        if idx is None or not same_batch:
            idx = torch.randint(0, cfg.vocab_size, (2, T), device=DEV, generator=g)
        if runner is None:
            loss = eng(idx, idx)[1]
            eng.backward(loss)
            eng.step()
        else:
            loss = runner(idx, idx)
        losses.append(loss.item())
        if cfg.moe_aux_on:
            aux.append(model.moe_aux(DEV).cpu().clone())
    if runner is not None:
        assert len(runner.graphs) == eng.accum and not runner.disabled
    return losses, eng.full_state_dict(), aux, eng


def test_graph_replay_is_eager_bit_for_bit():
    l0, s0, a0, _ = _train("zero3", False)
    l1, s1, a1, _ = _train("zero3", True)          # one eager window, then replays
    assert l0 == l1, (l0, l1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    for x, y in zip(a0, a1):
        assert torch.equal(x, y)
    assert not all(torch.equal(a0[0], x) for x in a0[1:])       # the record rows follow the batches
    assert all((x[:, 0] > 0).all() and (x[:, 0] <= 8).all() and (x[:, 1] > 0).all() for x in a0)


# ------------------------------------------------------------------------------------------- one layer against float64
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("E,K", [(8, 2), (8, 1), (32, 4)])
def test_layer_forward_backward_against_float64(E, K, dtype):
    """tests/test_moe_gpu.py's layer test with both losses on: the rows and the router lie on a dyadic grid, so the
    logits are exact on both sides and the routing is equal (asserted); dh2, every gradient and (balance, z) within
    that test's relative L2 bound.  At K = 1 the router's gradient comes from the auxiliary terms alone."""
    N, d = 200, 128
    cfg, model = base._layer_model(E, K, 1.0, dtype)
    cfg.moe_aux_loss_coef, cfg.moe_z_loss_coef = A, B
    cfg.validate()
    gen = torch.Generator().manual_seed(31 + E)
    h64 = base._grid((N, d), gen)
    wr64 = base._grid((E, d), gen) / 16.0
    wr64[E - 2] = wr64[1]
    h64[:, 0] = 1.0
    wr64[0, 0] += 1.0
    wr64[2, 0] += 0.75
    dm64 = torch.randn(N, d, generator=gen).to(dtype).double()
    with torch.no_grad():
        model.model.layers[0].mlp.router.weight.copy_(wr64)
        for ex in model.model.layers[0].mlp.experts:
            ex.gate_up_proj.weight.mul_(8.0)
            ex.down_proj.weight.mul_(8.0)
    m64 = copy.deepcopy(model).cpu().double()
    m64.rt = ParamRuntime()
    daux = torch.tensor([3.0, 0.5])          # large enough that the auxiliary part of the router gradient shows

    def run_layer(mod, h, dm, g):
        unit = mod.unit_blocks[0]
        ws = mod.rt.acquire(unit)
        m, saved, aux = mistral._moe_fwd(mod, 0, h, ws[4:])
        assert len(saved) == 12
        s = [(torch.full_like(w, float("nan")), False) for w in ws]
        dh = mistral._moe_bwd(mod, unit, dm, h, ws, s, saved, g)
        return m, dh, [t for t, _ in s[4:]], saved + (aux,)

    m_g, dh_g, grads_g, saved_g = run_layer(model, h64.to(DEV, dtype), dm64.to(DEV, dtype), daux.to(DEV))
    m_c, dh_c, grads_c, saved_c = run_layer(m64, h64, dm64, daux.double())
    for i in (0, 2, 3):
        assert torch.equal(saved_g[i].cpu(), saved_c[i]), i
    assert torch.equal(saved_g[11].cpu(), saved_c[11])                   # counts
    assert (saved_c[2] < 0).any()                                        # drops
    rel = base.rel
    assert rel(m_g, m_c) < 6e-2 and rel(dh_g, dh_c) < 6e-2, (rel(m_g, m_c), rel(dh_g, dh_c))
    assert rel(saved_g[12], saved_c[12]) < 6e-2 and rel(saved_g[10], saved_c[10]) < 6e-2
    assert torch.equal(model.moe_aux(DEV)[0], saved_g[12])
    names = ["router"] + [f"experts.{e}.{w}" for e in range(E) for w in ("gate_up", "down")]
    worst = 0.0
    for n, x, y in zip(names, grads_g, grads_c):
        assert float(y.abs().max()) > 0 or float(x.float().abs().max()) == 0, n
        r = rel(x, y)
        worst = max(worst, r)
        assert r < 6e-2, (n, r)
    assert float(grads_c[0].abs().max()) > 0 and float(grads_g[0].float().abs().max()) > 0     # also at K = 1
    print(f"E={E} K={K}: m {rel(m_g, m_c):.2e} dh {rel(dh_g, dh_c):.2e} aux {rel(saved_g[12], saved_c[12]):.2e} "
          f"router {rel(grads_g[0], grads_c[0]):.2e} worst gradient {worst:.2e}")


# ------------------------------------------------------------------------------------------- model level
def test_model_against_cpu_reference():
    """tests/test_moe_gpu.py's margin case (routers chosen so that no choice can flip between the precisions; the
    losses do not change the routing) with both losses on: the bf16 model on the GPU against the fp32 model on the CPU
    path, after that test's own routing checks (GPU-vs-float64 logit difference, chosen set per token), under ``TOL``
    in the form of multirank_util.compare, applied to one step's loss and gradients in place of a run's losses and
    updates: the loss within ``loss_tol``; all gradients as one vector within ``upd_tol`` relative L2 and ``cos_min``;
    every parameter's gradient within ``param_tol`` -- without compare's exemption of the parameters below 5 % of the
    largest, which would exempt the routers, the gradients this test is about.  Every figure is printed."""
    cfg, m_cpu, m64, idx, gap = base._margin_case()
    print(f"smallest gap between the 2nd and 3rd logit {gap:.3e}, required {base.GAP_FACTOR * base.LOGIT_DIFF:.3e}")
    assert gap >= base.GAP_FACTOR * base.LOGIT_DIFF, gap
    for m in (m_cpu, m64):
        m.cfg.moe_aux_loss_coef, m.cfg.moe_z_loss_coef = A, B
        m.cfg.validate()
    m_gpu = copy.deepcopy(m_cpu).to(DEV, torch.bfloat16)
    m_cpu.rt, m_gpu.rt = ParamRuntime(), ParamRuntime()
    assert m_gpu.cfg.moe_aux_on
    seen = {"cpu": [], "cuda": []}
    real_f = F_.moe_route

    def spy(h, wr, K):
        out = real_f(h, wr, K)
        seen[h.device.type].append((out[0].cpu(), out[2].detach().double().cpu()))
        return out

    tgt = idx.roll(-1, 1)
    F_.moe_route = spy
    try:
        m64(idx, tgt)
        want = list(seen["cpu"])
        seen["cpu"].clear()
        _, l_cpu = m_cpu(idx, tgt)
        _, l_gpu = m_gpu(idx.to(DEV), tgt.to(DEV))
    finally:
        F_.moe_route = real_f
    assert len(want) == len(seen["cuda"]) == len(seen["cpu"]) == cfg.n_layer
    diff = max(float((g[1] - w[1]).abs().max()) for g, w in zip(seen["cuda"], want))
    print(f"largest GPU-vs-float64 router logit difference {diff:.3e}")
    assert diff <= base.LOGIT_DIFF, diff
    for layer, (g, c, w) in enumerate(zip(seen["cuda"], seen["cpu"], want)):
        chosen = [t[0].sort(1).values for t in (g, c, w)]
        assert torch.equal(chosen[0], chosen[2]) and torch.equal(chosen[1], chosen[2]), f"routing flipped in layer {layer}"
    assert torch.equal(m_gpu.moe_counts(DEV).cpu(), m_cpu.moe_counts("cpu"))
    aux_rel = base.rel(m_gpu.moe_aux(DEV), m_cpu.moe_aux("cpu"))
    loss_rel = abs(l_cpu.item() - l_gpu.item()) / abs(l_cpu.item())
    print(f"loss cpu {l_cpu.item():.6f} gpu {l_gpu.item():.6f} (rel {loss_rel:.2e}, loss_tol {TOL['loss_tol']}); "
          f"(balance, z) rows rel {aux_rel:.2e}")
    assert loss_rel <= TOL["loss_tol"], loss_rel
    assert aux_rel <= TOL["loss_tol"], aux_rel
    l_cpu.backward()
    l_gpu.backward()
    gp = {n: p.grad.double().cpu() for n, p in m_gpu.named_parameters()}
    gc = {n: p.grad.double() for n, p in m_cpu.named_parameters()}
    vg = torch.cat([gp[n].reshape(-1) for n in gc])
    vc = torch.cat([gc[n].reshape(-1) for n in gc])
    whole = ((vg - vc).norm() / vc.norm()).item()
    cos = (torch.dot(vg, vc) / (vg.norm() * vc.norm())).item()
    print(f"all gradients: rel {whole:.3e} (upd_tol {TOL['upd_tol']}), cosine {cos:.6f} (cos_min {TOL['cos_min']})")
    bad = []
    for n in gc:
        r = base.rel(gp[n], gc[n])
        print(f"  {n}: rel {r:.3e}")
        if r > TOL["param_tol"]:
            bad.append((n, r))
    assert whole <= TOL["upd_tol"] and cos >= TOL["cos_min"], (whole, cos)
    assert not bad, bad
    routers = [n for n in gc if ".mlp.router." in n]
    assert len(routers) == cfg.n_layer and all(gc[n].norm().item() > 0 for n in routers)


# ------------------------------------------------------------------------------------------- end to end
def test_strategies_train_the_same_model():
    l2, s2, _, _ = _train("zero2", False, steps=4)
    l3, s3, _, _ = _train("zero3", False, steps=4)
    assert all(math.isfinite(v) for v in l2) and l2 == l3, (l2, l3)
    for k in s2:
        assert torch.equal(s2[k], s3[k]), k
    moe = [k for k in s2 if ".mlp.experts." in k or ".mlp.router." in k]
    assert len(moe) == 2 * 17
    for strategy in ("ddp", "fsdp", "zero3"):
        l, s, _, _ = _train(strategy, False, steps=6, same_batch=True)
        assert all(math.isfinite(v) for v in l), (strategy, l)
        assert l[-1] < l[0], (strategy, l)
        assert all(torch.isfinite(s[k].float()).all() for k in moe), strategy


def test_top1_router_gets_a_gradient_only_with_the_loss():
    """K = 1: the only gate is 1, so the router's gradient is exactly zero with both coefficients 0 and comes from the
    load-balancing term alone with ``a`` set (mtiny, E = 8, bf16, two layers)."""
    def router_grads(a):
        torch.manual_seed(0)
        cfg = get_model_config("mtiny", 128)
        cfg.n_experts, cfg.moe_top_k, cfg.moe_aux_loss_coef = 8, 1, a
        cfg.validate()
        model = build_model(cfg).to(DEV, torch.bfloat16)
        model.rt = ParamRuntime()
        idx = torch.randint(0, cfg.vocab_size, (2, 128), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        loss = model(idx, idx)[1]
        loss.backward()
        return [layer.mlp.router.weight.grad.float() for layer in model.model.layers]

    assert all(float(g.abs().max()) == 0.0 for g in router_grads(0.0))
    assert all(float(g.abs().max()) > 0.0 and torch.isfinite(g).all() for g in router_grads(A))


def test_fp16_build_trains_and_skips_no_step_more():
    l, s, _, eng = _train("ddp", False, dtype=torch.float16, steps=4)
    assert all(math.isfinite(v) for v in l), l
    assert all(torch.isfinite(t.float()).all() for t in s.values())
    _, _, _, eng0 = _train("ddp", False, dtype=torch.float16, steps=4, a=0.0, b=0.0)
    st, st0 = eng.scaler.stats(), eng0.scaler.stats()
    print(f"loss scaler with the losses {st}, without {st0}")
    assert st["optimizer_steps_skipped"] == st0["optimizer_steps_skipped"]
    assert st["optimizer_steps_taken"] == st0["optimizer_steps_taken"] > 0


def test_world2_host_staged_zero3_lazy(tmp_path):
    args = ("--seq-len", "128", "--windows", "2", "--cases", "zero3_mistral", "--moe-experts", "4",
            "--moe-capacity-factor", "2.0", "--moe-aux-loss-coef", str(A), "--moe-z-loss-coef", str(B))
    one = run(tmp_path / "w1.pt", 1, "cuda", extra=args)
    two = run(tmp_path / "w2.pt", 2, "cuda", extra=args, env_extra={"DLTB_COMM": "host", "DLTB_COMM_LAZY": "1"})
    # every rank forms f and P on its own rows: the two half-batch losses average to the one-rank loss only up to
    # the covariance of f and P between the halves, which at a = 0.01 is far below TOL's 1e-3 on a loss of 5.5
    bad = compare(one, two, **TOL)
    assert not bad, bad


def test_strict_kernels_and_the_record(tmp_path):
    from dltb.harness import main
    os.environ.pop("WORLD_SIZE", None)
    res = tmp_path / "res"
    assert main(["--strategy", "zero3", "--tier", "M7B_narrow", "--seq-len", "128", "--steps", "2", "--warmup-steps",
                 "1", "--per-device-batch", "1", "--grad-accum", "1", "--results-dir", str(res), "--log-every", "0",
                 "--moe-experts", "8", "--moe-top-k", "1", "--moe-aux-loss-coef", str(A), "--moe-z-loss-coef", str(B),
                 "--strict-kernels"]) == 0
    ext = [f for f in os.listdir(res) if f.endswith(".extended.json")]
    side = json.loads((res / ext[0]).read_text())
    assert side["torch_gemm_fallbacks"] is None and side["strict_kernels"] is True
    moe = side["moe"]
    assert moe["experts"] == 8 and moe["top_k"] == 1 and (moe["aux_loss_coef"], moe["z_loss_coef"]) == (A, B)
    assert len(moe["balance_loss"]) == len(moe["z_loss"]) == 32
    assert all(0.0 < v <= 8.0 for v in moe["balance_loss"]) and all(0.0 < v < 100.0 for v in moe["z_loss"])
    assert all(sum(c) == 128 for c in moe["counts"]) and len(moe["counts"]) == 32
