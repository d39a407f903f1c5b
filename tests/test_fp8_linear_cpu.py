"""Row-scaled FP8 linear layers on the CPU: the contract of ops/ref.py (``fp8_quant_rows``, ``gemm_fp8_nt``) on
hand-made rows, the refusals of ``--fp8-linear``, and a two-layer causal model trained on a CPU engine with the flag."""
import copy

import pytest
import torch

import dltb  # noqa: F401
from dltb.harness import check_fp8_linear
from dltb.models import build_model, get_model_config
from dltb.models.config import ModelConfig
from dltb.ops import ref
from dltb.parallel import ParamRuntime, engine_config, make_engine

BF16, F16 = torch.bfloat16, torch.float16
K = 128


def _row(amax, dtype=BF16):
    """A row whose largest magnitude is ``amax``, the rest a ramp below it."""
    x = torch.linspace(-0.9, 0.9, K).to(dtype).float() * amax
    x[5] = -amax
    return x.to(dtype)


# (row, the scale's exponent or None for NaN): zero row; amax exactly 448 * 2^e; just above it (one bf16 ulp: 450 * 2^e);
# +-2^100; 2^-130 (a bf16 subnormal: the exponent clamps at -126); inf; NaN
SPECIAL = [(torch.zeros(K, dtype=BF16), 0), (_row(448.0), 0), (_row(448.0 * 2.0 ** -7), -7), (_row(450.0), 1),
           (_row(450.0 * 2.0 ** 9), 10), (_row(2.0 ** 100), 92), (_row(2.0 ** -130), -126),
           (torch.cat([_row(3.0)[:-1], torch.tensor([float("inf")], dtype=BF16)]), None),
           (torch.cat([_row(3.0)[:-1], torch.tensor([float("nan")], dtype=BF16)]), None)]


@pytest.mark.parametrize("k", range(len(SPECIAL)))
def test_quant_rows_contract_on_hand_made_rows(k):
    x, e = SPECIAL[k]
    q, s = ref.fp8_quant_rows(x[None])
    if e is None:
        assert bool(torch.isnan(s[0])) and int(q.sum()) == 0
        return
    assert s[0].item() == 2.0 ** e
    scaled = x.double() / 2.0 ** e
    assert float(scaled.abs().max()) <= 448.0
    # s is the SMALLEST power of two that does it (the clamp at -126 aside)
    assert float(x.abs().max()) == 0 or e == -126 or float(scaled.abs().max()) > 224.0
    want = scaled.float().to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(q[0], want)


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_representable_rows_round_trip_exactly(dtype):
    """x == dec(q) * s when every x / s is an E4M3 value: every code times a per-row power of two."""
    codes = torch.arange(256, dtype=torch.uint8)
    vals = ref.fp8_dec(codes)
    vals = vals[torch.isfinite(vals)][None].repeat(3, 1)
    vals = torch.cat([vals, torch.zeros(3, 2)], 1)                       # 256 columns
    x = (vals * torch.tensor([1.0, 2.0 ** -9, 2.0 ** 5])[:, None]).to(dtype)
    q, s = ref.fp8_quant_rows(x)
    assert torch.equal(ref.fp8_dec(q) * s[:, None], x.float())


def test_refusals_name_the_switch():
    mt = get_model_config("mtiny", 128).to_dict()
    for kw in (dict(arch="tinygpt", causal=False), dict(mt, n_experts=4)):
        with pytest.raises(ValueError, match="--fp8-linear"):
            ModelConfig(**dict(kw, fp8_linear=True))
    with pytest.raises(ValueError, match="--fp8-linear"):
        check_fp8_linear(True, get_model_config("A", 128), "A")
    with pytest.raises(ValueError, match="--fp8-linear"):
        check_fp8_linear(True, get_model_config("mtiny", 128), "mtiny", loss_scaling=True)
    torch.manual_seed(0)
    model = build_model(ModelConfig(**dict(mt, fp8_linear=True)))
    ecfg = engine_config("ddp", 1, "reference", compute_dtype=F16)
    ecfg.extra["loss_scaling"] = True
    with pytest.raises(ValueError, match="--fp8-linear"):
        make_engine(model, ecfg, "cpu")


def test_cpu_engine_trains_the_float64_contract():
    """Two optimizer steps of the two-layer mtiny model (d 128, 128 tokens: every dense product is tile-aligned and takes
    the FP8 contract) on a CPU ZeRO-2 engine with the flag.  Each step's loss equals the float64 evaluation of the same
    contract at the engine's weights to 1e-5 relative: fp32 and float64 choose a different code only where x / s lies
    within ~2^-24 of a rounding boundary 2^-4 wide (about one in 4e6 elements, of ~1e6 here, each moving one activation
    by at most 6 %), which leaves the fp32 evaluation of the rest, ~1e-6 of the loss.  Without the flag the losses differ
    from these in the third digit (asserted: the flag is live)."""
    cfg = ModelConfig(**dict(get_model_config("mtiny", 128).to_dict(), fp8_linear=True))
    torch.manual_seed(0)
    model = build_model(cfg)
    plain = copy.deepcopy(model)
    plain.cfg = ModelConfig(**dict(cfg.to_dict(), fp8_linear=False))
    plain.rt = ParamRuntime()
    eng = make_engine(model, engine_config("zero2", 1, "reference"), "cpu")
    eng.train()
    g = torch.Generator().manual_seed(5)
    for step in range(2):
        idx = torch.randint(0, cfg.vocab_size, (1, 128), generator=g)
        wide = build_model(cfg).double()
        wide.load_state_dict({k: v.double() for k, v in eng.full_state_dict().items()})
        wide.rt = ParamRuntime()
        want = wide(idx, idx.roll(-1, 1))[1].item()
        loss = eng(idx, idx.roll(-1, 1))[1]
        eng.backward(loss)
        eng.step()
        print(f"step {step}: engine {loss.item():.9f}  float64 {want:.9f}")
        assert abs(loss.item() - want) <= 1e-5 * abs(want)
        if step == 0:
            off = plain(idx, idx.roll(-1, 1))[1].item()
            assert abs(off - want) > 1e-4 * abs(want), "the flag changed nothing"
    assert eng.opt_steps == 2
