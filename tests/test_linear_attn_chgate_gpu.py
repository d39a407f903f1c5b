"""csrc/linear_attn_chgate.hip on the MI355X: the per-channel mixer kernels, the gate's own kernels and the zero
up-projection against float64 under the bounds of tests/linear_attn_chgate_ref.py (no element left out), and a two-layer causal-tier
model under ``--linear-attn-gate-rank 16``.  The chunk is C = 64, so T = C, 2 C, 3 C: no state, one hop, two hops."""
import copy

import pytest
import torch

import dltb  # noqa: F401
from dltb.models import build_model, get_model_config
from dltb.models.config import ModelConfig
from dltb.models.oracle import OracleMistral
from dltb.ops import functional as F_
from dltb.parallel import GraphedStep, ParamRuntime, engine_config, make_engine

from linear_attn_chgate_ref import check_case, check_gate_kernels, check_zero_up

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = 64
BF16, F16 = torch.bfloat16, torch.float16


@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (4, 1), (4, 2)])
@pytest.mark.parametrize("T", [C, 2 * C, 3 * C])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
def test_kernels_against_float64(dtype, D, T, Hq, Hkv):
    check_case(F_, dtype, D, Hq, Hkv, T, DEV)


@pytest.mark.parametrize("Hkv", [1, 2])
@pytest.mark.parametrize("R", [8, 16])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
def test_gate_kernels_against_float64(dtype, R, Hkv):
    check_gate_kernels(F_, dtype, R, Hkv, DEV)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
def test_zero_up_projection_is_the_fixed_schedule(dtype, D):
    check_zero_up(F_, dtype, D, 4, 2, 2 * C, DEV)


# ---- a two-layer causal-tier model under --linear-attn-gate-rank 16
T_MODEL = 2 * C


def _build(**kw):      # the flag-on model, its up-projections away from their zero initialisation
    torch.manual_seed(0)
    model = build_model(ModelConfig(**dict(get_model_config("mtiny", T_MODEL).to_dict(), linear_attn=True,
                                           linear_attn_gate=True, linear_attn_gate_rank=16, qk_norm=True, **kw)))
    with torch.no_grad():
        for layer in model.model.layers:
            layer.self_attn.decay_gate.up.weight.normal_(0.0, 0.5)
    return model


def _train(steps, strategy="zero3", accum=1, graphed=False, same_batch=False, recompute="off", eng_kw=None, **kw):
    model = _build(**kw).to(DEV)
    model.activation_recompute = recompute
    eng = make_engine(model, engine_config(strategy, accum, "reference", **(eng_kw or {})), "cuda:0")
    eng.train()
    g = torch.Generator(device=DEV).manual_seed(1)
    runner = GraphedStep(eng) if graphed else None
    losses = []
    for i in range(steps):
        if i == 0 or not same_batch:
            idx = torch.randint(0, model.cfg.vocab_size, (2, T_MODEL), device=DEV, generator=g)
        if runner is None:
            loss = eng(idx, idx.roll(-1, 1))[1]
            eng.backward(loss)
            eng.step()
        else:
            loss = runner(idx, idx.roll(-1, 1))
        losses.append(loss.item())
    assert runner is None or (len(runner.graphs) == eng.accum and not runner.disabled)
    return losses, {k: v.detach().clone() for k, v in eng.full_state_dict().items()}, eng


@pytest.mark.parametrize("strategy,kw", [
    ("ddp", dict(eng_kw=dict(compute_dtype=F16))), ("fsdp", dict(fp8_linear=True)),
    ("zero2", dict(eng_kw=dict(optimizer="muon"))), ("zero3", dict(eng_kw=dict(optimizer_state="fp8")))],
    ids=["ddp-fp16", "fsdp-fp8", "zero2-muon", "zero3-fp8-state"])
def test_layer_composes(strategy, kw):
    """Four steps on one batch: the loss is finite and falls; under fp16 the loss scaler skips no step."""
    losses, _, eng = _train(4, strategy, same_batch=True, **kw)
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
    assert eng.scaler is None or eng.scaler.stats()["optimizer_steps_skipped"] == 0


@pytest.fixture(scope="module")
def runs():
    base = _build()
    idx = torch.randint(0, base.cfg.vocab_size, (2, T_MODEL), generator=torch.Generator().manual_seed(3))
    out = {}
    for kind in ("oracle", "off", "full"):
        if kind == "oracle":
            m, i = OracleMistral(base.cfg).double(), idx
            m.load_state_dict(copy.deepcopy(base).double().state_dict())
        else:
            m, i = copy.deepcopy(base).to(DEV, BF16), idx.to(DEV)
            m.rt, m.activation_recompute = ParamRuntime(), kind
        loss = m(i, i.roll(-1, 1))[1]
        loss.backward()
        out[kind] = (loss.detach(), {n: p.grad for n, p in m.named_parameters()})
    return out


def test_model_matches_the_oracle(runs):
    """``models/oracle.py`` (the quadratic per-channel form, autograd) in float64; the tolerances of
    tests/test_linear_attn_gate_gpu.py.  Both gate weights' gradients are among the compared ones."""
    (l_ref, g_ref), (l_gpu, g_gpu) = runs["oracle"], runs["off"]
    assert abs(l_ref.item() - l_gpu.item()) < 1e-2 * abs(l_ref.item())
    assert any(n.endswith("decay_gate.up.weight") for n in g_ref)
    for n, g in g_ref.items():
        r = ((g_gpu[n].double().cpu() - g).norm() / g.norm().clamp(min=1e-12)).item()
        assert r < 6e-2, (n, r)


def test_model_recompute_full_equals_off_bit_for_bit(runs):
    (l0, g0), (l1, g1) = runs["off"], runs["full"]
    assert torch.equal(l0, l1), (l0.item(), l1.item())
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_graph_replay_equals_eager():
    (l0, s0, _), (l1, s1, _) = (_train(4, accum=2, recompute="full", graphed=gr) for gr in (False, True))
    assert all(l == l for l in l0) and l0 == l1, (l0, l1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
