"""--linear-attn-gate-rank without a GPU: ``ops/ref.py``'s contract under the bounds of tests/linear_attn_chgate_ref.py,
the flag, its refusals, the sidecar, the parameter and FLOP counts, and the mtiny model against ``models/oracle.py``
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

from linear_attn_chgate_ref import check_case, check_gate_kernels, check_zero_up

C = 64
BASE = ["--strategy", "zero3", "--tier", "mtiny", "--seq-len", str(C), "--steps", "2", "--warmup-steps", "1",
        "--per-device-batch", "2", "--grad-accum", "1", "--device", "cpu", "--log-every", "0"]
GATE = ["--linear-attn", "--linear-attn-gate"]


def _cfg(T=C, **kw):
    return ModelConfig(**dict(get_model_config("mtiny", T).to_dict(), linear_attn=True, linear_attn_gate=True,
                              **dict(dict(linear_attn_gate_rank=16), **kw)))


@pytest.mark.parametrize("dtype,D,Hq,Hkv,T", [(torch.bfloat16, 64, 4, 2, 2 * C), (torch.float16, 128, 2, 2, 3 * C)])
def test_contract_against_float64(dtype, D, Hq, Hkv, T):
    check_case(F_, dtype, D, Hq, Hkv, T, "cpu")


def test_gate_contract_and_zero_up_projection():
    check_gate_kernels(F_, torch.bfloat16, 8, 2, "cpu")
    check_zero_up(F_, torch.float16, 64, 4, 2, 2 * C, "cpu")


def test_flag_parses_and_lands_in_the_sidecar(tmp_path):
    os.environ.pop("WORLD_SIZE", None)
    assert build_parser().parse_args(BASE + ["--results-dir", "x"]).linear_attn_gate_rank == 0
    for flag, res in ((["--linear-attn-gate-rank", "16"], tmp_path / "on"), ([], tmp_path / "off")):
        assert main(BASE + ["--results-dir", str(res)] + GATE + flag) == 0
        side = json.loads((res / [f for f in os.listdir(res) if f.endswith(".extended.json")][0]).read_text())
        assert side["linear_attn_gate_rank"] == (16 if flag else 0) == side["model"]["linear_attn_gate_rank"]


@pytest.mark.parametrize("argv", [["--linear-attn", "--linear-attn-gate-rank", "16"],
                                  GATE + ["--linear-attn-gate-rank", "12"], GATE + ["--linear-attn-gate-rank", "72"],
                                  GATE + ["--linear-attn-gate-rank", "16", "--tier", "tiny"]],
                         ids=["no-gate", "not-multiple-of-8", "above-64", "tinygpt"])
def test_refusals_name_the_switch(argv, tmp_path, capsys):
    with pytest.raises(SystemExit):
        main(BASE + ["--results-dir", str(tmp_path)] + argv)
    assert "--linear-attn-gate-rank" in capsys.readouterr().err


def test_config_refusals():
    base = get_model_config("mtiny", C).to_dict()
    for kw in (dict(linear_attn=True, linear_attn_gate_rank=16),
               dict(linear_attn=True, linear_attn_gate=True, linear_attn_gate_rank=True),
               dict(linear_attn=True, linear_attn_gate=True, linear_attn_gate_rank=64, n_embd=2048, n_head=16)):
        with pytest.raises(ValueError, match="--linear-attn-gate-rank"):    # the last: 64 (2 * 2048 + 256) > 160 KiB
            ModelConfig(**dict(base, **kw))


def test_parameter_count_flops_and_place_in_the_layer():
    on, scalar = _cfg(), _cfg(linear_attn_gate_rank=0)
    off = ModelConfig(**dict(get_model_config("mtiny", C).to_dict(), linear_attn=True))
    kvd = on.kv_heads * on.head_dim
    assert on.num_params() - off.num_params() == on.n_layer * 16 * (on.n_embd + kvd)
    assert on.train_flops_per_token(C) - off.train_flops_per_token(C) == 6 * on.n_layer * 16 * (on.n_embd + kvd)
    m = build_model(on)
    assert m.num_params() == on.num_params() == sum(p.numel() for p in m.parameters())
    for layer in m.model.layers:
        (n1, w1), (n2, w2) = layer.param_list()[-2:]
        assert (n1, n2) == ("self_attn.decay_gate.weight", "self_attn.decay_gate.up.weight")
        assert w1.shape == (16, on.n_embd) and w1.any() and w2.shape == (kvd, 16) and not w2.any()
    names = [n for n, _ in build_model(scalar).model.layers[0].param_list()]
    assert names[-1] == "self_attn.decay_gate.weight" and not any(".up." in n for n in names)


@pytest.mark.parametrize("kw", [{}, dict(qk_norm=True, sandwich_norm=True, ffn_act="geglu")], ids=["plain", "composed"])
def test_model_against_oracle_float64(kw):
    cfg = _cfg(2 * C, **kw)
    torch.manual_seed(0)
    m = build_model(cfg).double()
    with torch.no_grad():       # away from the zero initialisation, so the gate's own gradient path is exercised
        for layer in m.model.layers:
            layer.self_attn.decay_gate.up.weight.normal_(0.0, 0.5)
    o = OracleMistral(cfg).double()
    o.load_state_dict(m.state_dict())
    idx = torch.randint(0, cfg.vocab_size, (2, 2 * C), generator=torch.Generator().manual_seed(2))
    loss, lo = m(idx, idx.roll(-1, 1))[1], o(idx, idx.roll(-1, 1))[1]
    assert torch.allclose(loss, lo, atol=1e-10), (loss.item(), lo.item())
    loss.backward()
    lo.backward()
    got = dict(m.named_parameters())
    assert all(p.grad.abs().max() > 0 for n, p in o.named_parameters() if ".decay_gate." in n)
    for name, p in o.named_parameters():
        assert torch.allclose(got[name].grad, p.grad, atol=1e-9, rtol=1e-7), name
