"""--linear-attn without a GPU: ``ops/ref.py``'s chunked contract under the bound of tests/linear_attn_ref.py, the
refusals, the flag and the sidecar, the FLOP count, and the mtiny model against ``models/oracle.py`` (tolerances of
tests/test_attn_softcap_cpu.py: loss atol 1e-10, gradients atol 1e-9 / rtol 1e-7)."""
import json
import os
from types import SimpleNamespace

import pytest
import torch

import dltb  # noqa: F401
from dltb.harness import build_parser, check_linear_attn, main
from dltb.models import build_model, get_model_config
from dltb.models.config import ModelConfig
from dltb.models.oracle import OracleMistral
from dltb.ops import functional as F_
from dltb.parallel.context import ContextParallel

from linear_attn_ref import check_case

C = 64
BASE = ["--strategy", "zero3", "--tier", "mtiny", "--seq-len", str(C), "--steps", "2", "--warmup-steps", "1",
        "--per-device-batch", "2", "--grad-accum", "1", "--device", "cpu", "--log-every", "0"]


def _cfg(T=C, **kw):
    return ModelConfig(**dict(get_model_config("mtiny", T).to_dict(), linear_attn=True, **kw))


@pytest.mark.parametrize("D,Hq,Hkv,T", [(64, 2, 2, C), (64, 4, 1, 5 * C), (128, 4, 2, 2 * C)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_chunked_contract_against_float64(dtype, D, Hq, Hkv, T):
    check_case(F_, dtype, D, Hq, Hkv, T, "cpu")


def test_decay_schedule_and_refused_decays():
    want = torch.log2(1 - torch.exp2(-torch.arange(5, 13).double()))       # RetNet's eight, written out
    assert torch.allclose(F_.linear_attn_log2_gamma(8).double(), want, rtol=1e-6, atol=0)
    x = torch.zeros(C, 3 * 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="strictly negative"):
        F_.linear_attn_fwd(x[:, :64], x[:, 64:128], x[:, 128:], 1, C, 1, 1, torch.zeros(1))


@pytest.mark.parametrize("kw", [dict(arch="tinygpt"), dict(causal=False), dict(dropout=0.1), dict(sliding_window=16),
                                dict(doc_eos_id=3), dict(attn_sinks=True), dict(attn_softcap=50.0),
                                dict(n_embd=192, n_head=2)],
                         ids=["arch", "causal", "dropout", "window", "doc", "sinks", "softcap", "head_dim"])
def test_config_refusals_name_the_switch(kw):
    with pytest.raises(ValueError, match="--linear-attn"):
        _cfg(**kw)


@pytest.mark.parametrize("more", [["--sliding-window", "16"], ["--doc-len", "16"], ["--attn-sinks"],
                                  ["--attn-softcap", "50"]])
def test_main_refuses_before_training(more, capsys, tmp_path):
    with pytest.raises(SystemExit):
        main(BASE + ["--results-dir", str(tmp_path), "--linear-attn"] + more)
    assert "--linear-attn" in (err := capsys.readouterr().err) and "is not supported together" in err, err


def test_context_parallel_and_tinygpt_tiers_are_refused():
    for cfg, tier, cp in ((get_model_config("mtiny", C), "mtiny", 2), (get_model_config("tiny", C), "tiny", 1)):
        with pytest.raises(ValueError, match="--linear-attn"):
            check_linear_attn(True, cfg, tier, cp)
    with pytest.raises(ValueError, match="--linear-attn"):
        ContextParallel.attach(SimpleNamespace(cp=2), build_model(_cfg()))


def test_no_parameter_and_flops_independent_of_T():
    on, off = _cfg(), get_model_config("mtiny", C)
    assert on.num_params() == off.num_params()
    assert on.train_flops_per_token(C) == on.train_flops_per_token(512 * C)
    assert off.train_flops_per_token(C) != off.train_flops_per_token(512 * C)


def test_flag_parses_and_lands_in_the_sidecar(tmp_path):
    os.environ.pop("WORLD_SIZE", None)
    assert build_parser().parse_args(BASE + ["--results-dir", "x"]).linear_attn is False
    for flag, res in ((["--linear-attn"], tmp_path / "on"), ([], tmp_path / "off")):
        assert main(BASE + ["--results-dir", str(res)] + flag) == 0
        side = json.loads((res / [f for f in os.listdir(res) if f.endswith(".extended.json")][0]).read_text())
        assert side["linear_attn"] is bool(flag) and side["model"]["linear_attn"] is bool(flag)


@pytest.mark.parametrize("kw", [{}, dict(qk_norm=True, sandwich_norm=True, ffn_act="geglu")], ids=["plain", "composed"])
def test_model_against_oracle_float64(kw):
    cfg = _cfg(2 * C, **kw)
    torch.manual_seed(0)
    m = build_model(cfg).double()
    o = OracleMistral(cfg).double()
    o.load_state_dict(m.state_dict())
    idx = torch.randint(0, cfg.vocab_size, (2, 2 * C), generator=torch.Generator().manual_seed(2))
    loss, lo = m(idx, idx.roll(-1, 1))[1], o(idx, idx.roll(-1, 1))[1]
    assert torch.allclose(loss, lo, atol=1e-10), (loss.item(), lo.item())
    loss.backward()
    lo.backward()
    got = dict(m.named_parameters())
    for name, p in o.named_parameters():
        assert torch.allclose(got[name].grad, p.grad, atol=1e-9, rtol=1e-7), name
