"""--linear-attn-gate without a GPU: ``ops/ref.py``'s chunked contract under the bounds of tests/linear_attn_gate_ref.py,
the flag, its refusal, the sidecar, the parameter and FLOP counts, and the mtiny model against ``models/oracle.py``
(tolerances of tests/test_linear_attn_cpu.py: loss atol 1e-10, gradients atol 1e-9 / rtol 1e-7)."""
import json
import os

import pytest
import torch

import dltb  # noqa: F401
from dltb.harness import build_parser, main
from dltb.models import build_model, get_model_config
from dltb.models.config import ModelConfig
from dltb.models.oracle import OracleMistral
from dltb.ops import functional as F_

from linear_attn_gate_ref import check_case, check_gate_kernels, check_zero_gate

C = 64
BASE = ["--strategy", "zero3", "--tier", "mtiny", "--seq-len", str(C), "--steps", "2", "--warmup-steps", "1",
        "--per-device-batch", "2", "--grad-accum", "1", "--device", "cpu", "--log-every", "0"]


def _cfg(T=C, **kw):
    return ModelConfig(**dict(get_model_config("mtiny", T).to_dict(), linear_attn=True, linear_attn_gate=True, **kw))


@pytest.mark.parametrize("D,Hq,Hkv,T", [(64, 2, 2, C), (64, 4, 1, 5 * C), (128, 4, 2, 2 * C)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_chunked_contract_against_float64(dtype, D, Hq, Hkv, T):
    check_case(F_, dtype, D, Hq, Hkv, T, "cpu")


@pytest.mark.parametrize("Hkv", [1, 2])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_gate_contract_against_float64(dtype, Hkv):
    check_gate_kernels(F_, dtype, Hkv, "cpu")


def test_zero_gate_is_the_fixed_schedule():
    check_zero_gate(F_, torch.bfloat16, 64, 4, 2, 2 * C, "cpu")


def test_flag_parses_is_refused_alone_and_lands_in_the_sidecar(tmp_path, capsys):
    os.environ.pop("WORLD_SIZE", None)
    assert build_parser().parse_args(BASE + ["--results-dir", "x"]).linear_attn_gate is False
    with pytest.raises(ValueError, match="--linear-attn-gate.*--linear-attn"):
        ModelConfig(**dict(get_model_config("mtiny", C).to_dict(), linear_attn_gate=True))
    with pytest.raises(SystemExit):
        main(BASE + ["--results-dir", str(tmp_path), "--linear-attn-gate"])
    assert "--linear-attn-gate needs --linear-attn" in capsys.readouterr().err
    for flag, res in ((["--linear-attn-gate"], tmp_path / "on"), ([], tmp_path / "off")):
        assert main(BASE + ["--results-dir", str(res), "--linear-attn"] + flag) == 0
        side = json.loads((res / [f for f in os.listdir(res) if f.endswith(".extended.json")][0]).read_text())
        assert side["linear_attn"] is True and side["linear_attn_gate"] is bool(flag)
        assert side["model"]["linear_attn_gate"] is bool(flag)


def test_parameter_count_flops_and_place_in_the_layer():
    on, off = _cfg(), ModelConfig(**dict(get_model_config("mtiny", C).to_dict(), linear_attn=True))
    assert on.num_params() - off.num_params() == on.n_layer * on.kv_heads * on.n_embd
    assert on.train_flops_per_token(C) - off.train_flops_per_token(C) == 6 * on.n_layer * on.n_embd * on.kv_heads
    m = build_model(on)
    assert m.num_params() == on.num_params()
    for layer in m.model.layers:
        name, w = layer.param_list()[-1]
        assert name == "self_attn.decay_gate.weight" and w.shape == (on.kv_heads, on.n_embd) and not w.any()


@pytest.mark.parametrize("kw", [{}, dict(qk_norm=True, sandwich_norm=True, ffn_act="geglu")], ids=["plain", "composed"])
def test_model_against_oracle_float64(kw):
    cfg = _cfg(2 * C, **kw)
    torch.manual_seed(0)
    m = build_model(cfg).double()
    with torch.no_grad():       # away from the zero initialisation, so the gate's own gradient path is exercised
        for layer in m.model.layers:
            layer.self_attn.decay_gate.weight.normal_(0.0, 0.5)
    o = OracleMistral(cfg).double()
    o.load_state_dict(m.state_dict())
    idx = torch.randint(0, cfg.vocab_size, (2, 2 * C), generator=torch.Generator().manual_seed(2))
    loss, lo = m(idx, idx.roll(-1, 1))[1], o(idx, idx.roll(-1, 1))[1]
    assert torch.allclose(loss, lo, atol=1e-10), (loss.item(), lo.item())
    loss.backward()
    lo.backward()
    got = dict(m.named_parameters())
    assert any(n.endswith("decay_gate.weight") and p.grad.abs().max() > 0 for n, p in o.named_parameters())
    for name, p in o.named_parameters():
        assert torch.allclose(got[name].grad, p.grad, atol=1e-9, rtol=1e-7), name
