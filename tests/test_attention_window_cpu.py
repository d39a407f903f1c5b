"""Sliding-window causal attention (``window = W``: query i sees key j iff ``i - W < j <= i``) on the
CPU: the reference ops against a dense fp64 masked softmax and its autograd gradients, the Mistral-shape
model against the stock-op oracle, the FLOP count, and the harness flag."""
import json
import math
import os

import pytest
import torch

import dltb
from dltb.models import ModelConfig, get_model_config
from dltb.models.mistral import MistralLM
from dltb.models.oracle import OracleMistral
from dltb.ops import functional as F_
from dltb.ops import ref
from dltb.ops.rng import StepSeed

B, T, HQ, HKV, D = 2, 32, 4, 2, 8
SCALE = 1.0 / math.sqrt(D)
SITE = 11


def _seed():
    s = StepSeed(1234, 0)
    s.next()
    return s


def _inputs():
    g = torch.Generator().manual_seed(0)
    q = torch.randn(B * T, HQ * D, generator=g, dtype=torch.float64)
    k = torch.randn(B * T, HKV * D, generator=g, dtype=torch.float64)
    v = torch.randn(B * T, HKV * D, generator=g, dtype=torch.float64)
    do = torch.randn(B * T, HQ * D, generator=g, dtype=torch.float64)
    return q, k, v, do


def _dense(q, k, v, window, p, sd):
    """softmax over the band i - W < j <= i, written out densely in fp64 (dropout after the softmax)."""
    heads = lambda t, H: t.reshape(B, T, H, D).transpose(1, 2)
    qh = heads(q, HQ)
    kh = heads(k, HKV).repeat_interleave(HQ // HKV, 1)
    vh = heads(v, HKV).repeat_interleave(HQ // HKV, 1)
    i = torch.arange(T)
    band = (i[None, :] <= i[:, None]) & (i[None, :] > i[:, None] - window)
    s = (qh @ kh.transpose(-1, -2)) * SCALE
    s = torch.where(band, s, torch.full_like(s, float("-inf")))
    lse = torch.logsumexp(s, -1)
    pr = torch.softmax(s, -1)
    if p > 0:
        keep = ref._attn_keep(B, HQ, T, p, sd, SITE, q.device)
        pr = pr * keep.to(pr.dtype) / (1.0 - p)
    o = (pr @ vh).transpose(1, 2).reshape(B * T, HQ * D)
    return o, lse, band


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("window", [1, 5, 31, 32, 40])
def test_ref_window_matches_dense_fp64(window, p):
    q, k, v, do = _inputs()
    sd = _seed()
    o, lse = ref.attn_fwd(q, k, v, B, T, HQ, HKV, SCALE, True, p, sd, SITE, window=window)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    ro, rlse, band = _dense(qa, ka, va, window, p, sd)
    assert int(band[T - 1].sum()) == min(window, T) and int(band[0].sum()) == 1
    assert torch.allclose(o, ro.detach(), atol=1e-12, rtol=1e-10)
    assert torch.allclose(lse.double(), rlse.detach(), atol=1e-5)         # ref returns lse in fp32
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ref.attn_bwd(q, k, v, o, do, rlse.detach(), dq, dk, dv, B, T, HQ, HKV, SCALE, True, p, sd, SITE, window=window)
    ro.backward(do)
    for name, a, r in (("dq", dq, qa.grad), ("dk", dk, ka.grad), ("dv", dv, va.grad)):
        assert torch.allclose(a, r, atol=1e-10, rtol=1e-8), (name, (a - r).abs().max().item())
    # the public op takes the same keyword on the CPU path
    fo, flse, _ = F_.attn_fwd(q, k, v, B, T, HQ, HKV, SCALE, True, p, sd, SITE, window=window)
    assert torch.equal(fo, o) and torch.equal(flse, lse)
    fdq, fdk, fdv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    F_.attn_bwd(q, k, v, o, do, rlse.detach(), None, fdq, fdk, fdv, B, T, HQ, HKV, SCALE, True, p, sd, SITE,
                window=window)
    assert torch.equal(fdq, dq) and torch.equal(fdk, dk) and torch.equal(fdv, dv)


@pytest.mark.parametrize("window", [32, 40])
def test_window_of_t_or_more_is_plain_causal(window):
    q, k, v, do = _inputs()
    sd = _seed()
    o0, l0 = ref.attn_fwd(q, k, v, B, T, HQ, HKV, SCALE, True, 0.1, sd, SITE)
    o1, l1 = ref.attn_fwd(q, k, v, B, T, HQ, HKV, SCALE, True, 0.1, sd, SITE, window=window)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    g0 = [torch.empty_like(t) for t in (q, k, v)]
    g1 = [torch.empty_like(t) for t in (q, k, v)]
    ref.attn_bwd(q, k, v, o0, do, l0, *g0, B, T, HQ, HKV, SCALE, True, 0.1, sd, SITE)
    ref.attn_bwd(q, k, v, o0, do, l0, *g1, B, T, HQ, HKV, SCALE, True, 0.1, sd, SITE, window=window)
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))


def test_window_needs_causal():
    q, k, v, do = _inputs()
    sd = _seed()
    g = [torch.empty_like(t) for t in (q, k, v)]
    with pytest.raises(ValueError, match="causal"):
        ref.attn_fwd(q, k, v, B, T, HQ, HKV, SCALE, False, 0.0, sd, SITE, window=8)
    with pytest.raises(ValueError, match="causal"):
        ref.attn_bwd(q, k, v, q, do, torch.zeros(B, HQ, T), *g, B, T, HQ, HKV, SCALE, False, 0.0, sd, SITE, window=8)
    with pytest.raises(ValueError, match="causal"):
        F_.attn_fwd(q, k, v, B, T, HQ, HKV, SCALE, False, 0.0, sd, SITE, window=8)
    with pytest.raises(ValueError, match="causal"):
        F_.attn_bwd(q, k, v, q, do, torch.zeros(B, HQ, T), None, *g, B, T, HQ, HKV, SCALE, False, 0.0, sd, SITE,
                    window=8)
    with pytest.raises(ValueError, match=">= 0"):
        F_.attn_fwd(q, k, v, B, T, HQ, HKV, SCALE, True, 0.0, sd, SITE, window=-1)


def test_config_validates_window():
    assert get_model_config("M7B", 4096).sliding_window is None          # no tier's default changes
    assert get_model_config("mtiny", 32).sliding_window is None
    with pytest.raises(ValueError, match="causal"):
        ModelConfig(causal=False, sliding_window=8)
    with pytest.raises(ValueError, match=">= 1"):
        ModelConfig(arch="mistral", causal=True, sliding_window=0)
    cfg = get_model_config("tiny", 32)
    cfg.sliding_window = 8
    with pytest.raises(ValueError, match="causal"):
        cfg.validate()
    # a config saved before the key existed (no "sliding_window" entry) still loads: no window
    old = get_model_config("mtiny", 32).to_dict()
    del old["sliding_window"]
    assert ModelConfig(**old).sliding_window is None
    assert ModelConfig(**dict(old, sliding_window=8)).to_dict()["sliding_window"] == 8


def _pair(window, T_=32):
    cfg = get_model_config("mtiny", T_)
    cfg.sliding_window = window
    cfg.validate()
    torch.manual_seed(0)
    m = MistralLM(cfg).double()
    o = OracleMistral(cfg).double()
    o.load_state_dict(m.state_dict())
    return cfg, m, o


def test_mistral_window_matches_oracle():
    cfg, m, o = _pair(8)
    idx = torch.randint(0, cfg.vocab_size, (2, 32))
    tgt = idx.roll(-1, 1)
    tgt[1, -5:] = -1
    _, loss = m(idx, tgt)
    _, lo = o(idx, tgt)
    assert torch.allclose(loss, lo, atol=1e-10), (loss.item(), lo.item())
    loss.backward()
    lo.backward()
    got = dict(m.named_parameters())
    for name, p in o.named_parameters():
        assert got[name].grad is not None, name
        assert torch.allclose(got[name].grad, p.grad, atol=1e-9, rtol=1e-7), name
    # the window is really applied: the same weights without it give another loss
    _, m_full, _ = _pair(None)
    _, l_full = m_full(idx, tgt)
    assert abs(l_full.item() - loss.item()) > 1e-6, (l_full.item(), loss.item())


def test_train_flops_follow_the_window():
    T_, W = 16384, 4096
    base = get_model_config("M7B", T_)
    full = base.train_flops_per_token(T_)
    L, d = base.n_layer, base.n_embd
    cfg = get_model_config("M7B", T_)
    cfg.sliding_window = W
    want = full - 12 * L * d * (T_ / 2) + 12 * L * d * (W * (T_ - W) + W * W / 2) / T_
    assert cfg.train_flops_per_token(T_) == pytest.approx(want, rel=1e-12)
    assert cfg.train_flops_per_token(T_) < full
    for w in (T_, T_ + 1, 10 * T_):                       # W >= T: today's number exactly
        cfg.sliding_window = w
        assert cfg.train_flops_per_token(T_) == full


def _harness_args(tier, res):
    return ["--strategy", "ddp", "--tier", tier, "--seq-len", "32", "--steps", "2", "--warmup-steps", "1",
            "--per-device-batch", "1", "--grad-accum", "1", "--results-dir", str(res), "--device", "cpu",
            "--sliding-window", "16"]


def test_harness_records_the_window(tmp_path):
    from dltb.harness import main
    os.environ.pop("WORLD_SIZE", None)
    assert main(_harness_args("mtiny", tmp_path / "res")) == 0
    ext = [f for f in os.listdir(tmp_path / "res") if f.endswith(".extended.json")]
    side = json.loads((tmp_path / "res" / ext[0]).read_text())
    assert side["model"]["sliding_window"] == 16
    plain = [f for f in os.listdir(tmp_path / "res") if f.endswith(".json") and not f.endswith(".extended.json")]
    assert "sliding_window" not in json.loads((tmp_path / "res" / plain[0]).read_text())


def test_harness_refuses_window_on_noncausal_tier(tmp_path, capsys):
    from dltb.harness import main
    with pytest.raises(SystemExit) as e:
        main(_harness_args("tiny", tmp_path / "res"))
    assert e.value.code == 2                              # argparse's argument error
    assert "--sliding-window" in capsys.readouterr().err
    assert not (tmp_path / "res").exists()
