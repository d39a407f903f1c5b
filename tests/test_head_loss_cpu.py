"""Final-logit soft-capping and the LM-head z-loss (``--final-softcap C`` / ``--lm-z-loss-coef B``) without a GPU: the
torch references of the three loss ops against float64 autograd on the defining expression
``logsumexp(C tanh(z / C)) - c_t + B lse^2``, the config fields, the harness's flags / refusals / printout / sidecar,
the CPU model against the stock-op oracle, the head in row chunks against the unchunked head, and a config with both
options 0 against one that never heard of the fields.

Inputs: the recipe of tests/test_head_chunk_gpu.py (``randn * 2``, one row of +-80, a target of -1 every 7th row,
targets 0 and V - 1), 70 rows.  Options: (30, 0) Gemma's cap; (2, 0) most logits on the curved part of tanh and the
+-80 row saturated exactly; (0, 0.1) and (2, 0.1) a z-loss large enough to move dlogits past the output's rounding.
Tolerances: loss and lse 1e-3 + 1e-3 rel, dlogits 1e-4 + 2e-2 rel (tests/test_head_chunk_gpu.py).
"""
import copy
import json
import math
import os

import pytest
import torch

import dltb  # noqa: F401
from dltb.harness import build_parser, check_final_softcap, check_lm_z_loss
from dltb.models import build_model, get_model_config
from dltb.models.config import ModelConfig
from dltb.models.oracle import OracleMistral
from dltb.ops import functional as F_
from dltb.ops import ref
from dltb.parallel import ParamRuntime
from test_head_chunk_cpu import _head_ctx

F64 = torch.float64
OPTS = [(30.0, 0.0), (2.0, 0.0), (0.0, 0.1), (2.0, 0.1)]
OPT_IDS = ["cap30", "cap2", "z0.1", "cap2_z0.1"]
EPS32 = 2.0 ** -23


def logits_case(N, V, dtype, seed=0, device="cpu"):
    """tests/test_head_chunk_gpu.py::_logits on any device (generated on the CPU, so one recipe serves both files)."""
    g = torch.Generator().manual_seed(seed + V)
    z = (torch.randn(N, V, generator=g) * 2.0).to(dtype)
    if N > 5:
        z[5] = 80.0
        z[5, 1::2] = -80.0                                  # one row of +-80
    t = torch.randint(0, V, (N,), generator=g)
    t[::7] = -1
    if N > 2:
        t[1], t[2] = 0, V - 1
    return z.to(device), t.to(device)


def reference64(z, t, C, B):
    """(loss rows, lse rows, dz) in float64 by autograd on the defining expression, from the 16-bit ``z`` itself;
    ignored rows are 0 in loss and dz.  Independent of ops/ref.py's closed form."""
    z64 = z.detach().double().requires_grad_()
    c = C * torch.tanh(z64 / C) if C else z64
    lse = torch.logsumexp(c, -1)
    valid = t != -1
    ct = c.gather(-1, t.clamp(min=0)[:, None])[:, 0]
    rows = torch.where(valid, lse - ct + B * lse * lse, torch.zeros_like(lse))
    dz, = torch.autograd.grad(rows.sum(), z64)
    return rows.detach(), lse.detach(), dz


def close(a, b, atol, rtol, what=""):
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    err = (a.double() - b.double()).abs()
    tol = atol + rtol * b.double().abs()
    print(f"{what}: worst error/tolerance {float((err / tol).max()):.3f}")
    bad = (err > tol).double().mean().item()
    assert bad == 0.0, f"{what}: {bad * 100:.3f}% elements out of tolerance, max err {err.max().item():.4g}"


# ------------------------------------------------------------------------------------------- reference ops
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("V", [8, 256, 1000])
@pytest.mark.parametrize("C,B", OPTS, ids=OPT_IDS)
def test_ref_ops_against_float64_autograd(C, B, V, dtype):
    z, t = logits_case(70, V, dtype)
    loss64, lse64, dz64 = reference64(z, t, C, B)
    for mod in (ref, F_):
        fused = z.clone()
        loss = mod.xent_fwd_bwd_(fused, t, -1, softcap=C, z_coef=B)
        assert loss.dtype == torch.float32 and fused.dtype == dtype
        close(loss, loss64, 1e-3, 1e-3, "loss")
        close(fused, dz64, 1e-4, 2e-2, "dlogits")
        assert (loss[t == -1] == 0).all() and (fused[t == -1] == 0).all()
        keep = z.clone()
        loss2, lse = mod.xent_lse(keep, t, -1, softcap=C, z_coef=B)
        assert torch.equal(keep, z)                         # read only
        assert torch.equal(loss2, loss)                     # the fused op's loss rows
        close(lse, lse64, 1e-3, 1e-3, "lse")
        back = z.clone()
        assert mod.xent_bwd_lse_(back, t, lse, -1, softcap=C, z_coef=B) is back
        close(back, dz64, 1e-4, 2e-2, "dlogits from lse")
        assert (back[t == -1] == 0).all()
        if C == 2.0:                                        # tanh(+-40) is exactly +-1: the gradient is exactly 0
            assert (fused[5] == 0).all() and (back[5] == 0).all()
    # the options are in the comparison: the plain loss is another one
    plain = ref.xent_fwd_bwd_(z.clone(), t, -1)
    assert (plain - loss).abs().max() > 1e-3


def test_ref_ops_with_both_options_zero_are_the_plain_ops():
    z, t = logits_case(70, 256, torch.bfloat16)
    a, b = z.clone(), z.clone()
    assert torch.equal(ref.xent_fwd_bwd_(a, t, -1), F_.xent_fwd_bwd_(b, t, -1, softcap=0.0, z_coef=0.0))
    assert torch.equal(a, b)
    l0, s0 = ref.xent_lse(z, t, -1)
    l1, s1 = F_.xent_lse(z, t, -1, softcap=0.0, z_coef=0.0)
    assert torch.equal(l0, l1) and torch.equal(s0, s1)
    assert torch.equal(ref.xent_bwd_lse_(z.clone(), t, s0, -1), F_.xent_bwd_lse_(z.clone(), t, s0, -1, 0.0, 0.0))


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), True, "30"])
def test_ops_refuse_bad_options(bad):
    z, t = logits_case(8, 64, torch.float32)
    _, lse = ref.xent_lse(z, t, -1)
    for kw in (dict(softcap=bad), dict(z_coef=bad)):
        name = next(iter(kw))
        with pytest.raises(ValueError, match=name):
            F_.xent_fwd_bwd_(z.clone(), t, -1, **kw)
        with pytest.raises(ValueError, match=name):
            F_.xent_lse(z, t, -1, **kw)
        with pytest.raises(ValueError, match=name):
            F_.xent_bwd_lse_(z.clone(), t, lse, -1, **kw)


# ------------------------------------------------------------------------------------------- config, flags
def _cfg(T_=32, **kw):
    return ModelConfig(**dict(get_model_config("mtiny", T_).to_dict(), **kw))


@pytest.mark.parametrize("field", ["final_softcap", "lm_z_loss_coef"])
def test_config_validation(field):
    assert getattr(get_model_config("mtiny", 32), field) == 0.0
    assert getattr(_cfg(**{field: 30.0}), field) == 30.0
    assert getattr(_cfg(**{field: 30}), field) == 30
    with pytest.raises(ValueError, match=field):
        ModelConfig(**dict(get_model_config("tiny", 32).to_dict(), **{field: 30.0}))
    for bad in (-1.0, float("nan"), float("inf"), True, "30"):
        with pytest.raises(ValueError, match=field):
            _cfg(**{field: bad})
    cfg = get_model_config("tiny", 32)
    setattr(cfg, field, 1e-4)
    with pytest.raises(ValueError, match=field):
        cfg.validate()
    old = {k: v for k, v in get_model_config("mtiny", 32).to_dict().items() if k != field}
    assert getattr(ModelConfig(**old), field) == 0.0


def test_no_parameter_and_flops_unchanged():
    on, off = _cfg(final_softcap=30.0, lm_z_loss_coef=1e-4), _cfg()
    assert on.num_params() == off.num_params()
    assert on.train_flops_per_token(32) == off.train_flops_per_token(32)
    torch.manual_seed(0)
    a = build_model(on)
    torch.manual_seed(0)
    b = build_model(off)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    assert [n for u in a.units() for n in u.names] == [n for u in b.units() for n in u.names]
    assert list(OracleMistral(on).state_dict().keys()) == list(b.state_dict().keys())


def _base(res, tier="mtiny"):
    return ["--strategy", "zero3", "--tier", tier, "--seq-len", "32", "--steps", "2", "--warmup-steps", "1",
            "--per-device-batch", "2", "--grad-accum", "1", "--results-dir", str(res), "--device", "cpu",
            "--log-every", "0"]


def test_flags_parse_and_refusals(tmp_path, capsys):
    from dltb.harness import main
    base = _base(tmp_path / "res")
    a = build_parser().parse_args(base)
    assert a.final_softcap == 0.0 and a.lm_z_loss_coef == 0.0
    a = build_parser().parse_args(base + ["--final-softcap", "30", "--lm-z-loss-coef", "1e-4"])
    assert a.final_softcap == 30.0 and a.lm_z_loss_coef == 1e-4
    for check, flag, field in ((check_final_softcap, "--final-softcap", "final_softcap"),
                               (check_lm_z_loss, "--lm-z-loss-coef", "lm_z_loss_coef")):
        cfg = get_model_config("mtiny", 32)
        check(0.0, cfg, "mtiny")
        assert getattr(cfg, field) == 0.0
        check(0.5, cfg, "mtiny")
        assert getattr(cfg, field) == 0.5
        check(0.0, get_model_config("tiny", 32), "tiny")               # off is accepted on every tier
        with pytest.raises(ValueError, match=f"{flag} needs a causal tier"):
            check(0.5, get_model_config("tiny", 32), "tiny")
        for bad in (-3.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=f"{flag} must be"):
                check(bad, get_model_config("mtiny", 32), "mtiny")
        for tier in ("tiny", "A"):
            with pytest.raises(SystemExit) as e:
                main(_base(tmp_path / "res", tier) + [flag, "0.5"])
            assert e.value.code == 2                                   # argparse's argument error
            assert f"{flag} needs a causal tier" in capsys.readouterr().err
        with pytest.raises(SystemExit) as e:
            main(base + [flag, "-1"])
        assert e.value.code == 2
        assert f"{flag} must be" in capsys.readouterr().err
    assert not (tmp_path / "res").exists()


def _side(res):
    ext = [f for f in os.listdir(res) if f.endswith(".extended.json")]
    plain = [f for f in os.listdir(res) if f.endswith(".json") and not f.endswith(".extended.json")]
    return json.loads((res / plain[0]).read_text()), json.loads((res / ext[0]).read_text())


def test_harness_sidecar_lines_and_total_loss(tmp_path, capsys):
    from dltb.harness import main
    os.environ.pop("WORLD_SIZE", None)
    assert main(_base(tmp_path / "on") + ["--final-softcap", "30", "--lm-z-loss-coef", "0.1"]) == 0
    out = capsys.readouterr().out
    assert "final-logit soft-capping: the loss is formed from 30 * tanh(logits / 30)" in out
    assert "LM-head z-loss: 0.1 * mean(logsumexp(logits)^2)" in out
    rec_on, side = _side(tmp_path / "on")
    assert side["final_softcap"] == 30.0 and side["lm_z_loss_coef"] == 0.1
    assert side["model"]["final_softcap"] == 30.0 and side["model"]["lm_z_loss_coef"] == 0.1
    assert "final_softcap" not in rec_on and "lm_z_loss_coef" not in rec_on    # the reference-format record
    assert main(_base(tmp_path / "off")) == 0
    out = capsys.readouterr().out
    assert "final-logit soft-capping" not in out and "LM-head z-loss" not in out
    rec_off, side2 = _side(tmp_path / "off")
    assert side2["final_softcap"] == 0.0 and side2["lm_z_loss_coef"] == 0.0
    assert side["train_flops_per_token"] == side2["train_flops_per_token"] and side["params"] == side2["params"]
    # the reported loss is the total: at initialisation lse ~ log V, so the z-term adds about 0.1 log(256)^2 = 3.1
    assert rec_on["mean_loss"] - rec_off["mean_loss"] > 0.5 * 0.1 * math.log(256) ** 2


# ------------------------------------------------------------------------------------------- whole model
def _scaled_up(m, mul=200.0):
    """A larger head, so that the logits (N(0, about 0.45^2) at the initialisation) reach past the cap of 2."""
    with torch.no_grad():
        m.lm_head.weight.mul_(mul)
    return m


def _batch(cfg, T_=32):
    idx = torch.randint(0, cfg.vocab_size, (2, T_), generator=torch.Generator().manual_seed(2))
    tgt = idx.roll(-1, 1).clone()
    tgt[:, ::9] = -1
    return idx, tgt


@pytest.mark.parametrize("kw", [dict(), dict(qk_norm=True), dict(attn_softcap=50.0),
                                dict(n_experts=4, moe_top_k=2, moe_aux_loss_coef=0.01, moe_z_loss_coef=0.001)],
                         ids=["dense", "qknorm", "attn_softcap", "moe_aux"])
@pytest.mark.parametrize("C,B", [(30.0, 0.0), (2.0, 0.0), (0.0, 0.1), (2.0, 0.1)], ids=OPT_IDS)
def test_model_against_oracle_float64(C, B, kw):
    """The CPU model path (ops/ref.py's closed form, the fused head Function) against autograd through the stock-op
    oracle, in float64; the same weights without the options give another loss."""
    cfg = _cfg(final_softcap=C, lm_z_loss_coef=B, **kw)
    torch.manual_seed(0)
    m = _scaled_up(build_model(cfg), 20.0).double()
    o = OracleMistral(cfg).double()
    o.load_state_dict(m.state_dict())
    idx, tgt = _batch(cfg)
    _, loss = m(idx, tgt)
    _, lo = o(idx, tgt)
    assert torch.allclose(loss, lo, atol=1e-10), (loss.item(), lo.item())
    loss.backward()
    lo.backward()
    got = dict(m.named_parameters())
    for name, p in o.named_parameters():
        if p.grad is None:          # an expert without a token
            continue
        assert got[name].grad is not None, name
        assert torch.allclose(got[name].grad, p.grad, atol=1e-9, rtol=1e-7), name
    off = OracleMistral(_cfg(**kw)).double()
    off.load_state_dict(m.state_dict())
    _, l_off = off(idx, tgt)
    assert abs(l_off.item() - lo.item()) > 1e-4, (l_off.item(), lo.item())


def test_returned_logits_are_the_capped_ones():
    cfg = _cfg(final_softcap=2.0)
    torch.manual_seed(0)
    m = _scaled_up(build_model(cfg), 20.0)
    idx, tgt = _batch(cfg)
    raw_model = copy.deepcopy(m)
    raw_model.cfg = _cfg()
    raw, _ = raw_model(idx, tgt, return_logits=True)
    assert raw.abs().max() > 2.0                             # the cap bites
    want = 2.0 * torch.tanh(raw.float() / 2.0)
    for chunk in (None, 16):
        m.head_chunk = chunk
        got, loss = m(idx, tgt, return_logits=True)
        only, none = m(idx)
        assert none is None and torch.equal(only, got)
        assert got.shape == raw.shape and torch.equal(got, want)
        assert got.abs().max() <= 2.0
    o = OracleMistral(cfg)
    o.load_state_dict(m.state_dict())
    lo_logits, lo = o(idx, tgt)
    assert torch.allclose(got, lo_logits, atol=1e-5) and torch.allclose(loss, lo, atol=1e-5)


def _head_run(cfg, base, chunk, idx, tgt):
    m = copy.deepcopy(base)
    m.cfg = cfg
    m.rt = ParamRuntime()
    m.head_chunk = chunk
    _, loss = m(idx, tgt)
    ctx = _head_ctx(loss)
    saved = [t for t in ctx.saved if torch.is_tensor(t)]
    x = ctx.saved[0]
    loss.backward()
    return dict(loss=loss.detach(), grads={n: p.grad for n, p in m.named_parameters()},
                saved=[(tuple(t.shape), t.dtype) for t in saved], x=x.detach(), model=m, tgt=tgt.reshape(-1))


def _head64(run_, C, B):
    """tests/test_head_chunk_cpu.py::_head64 with the options: the head in float64 on the run's own input: the loss,
    the head's weight gradient, and sum_r |dz[r, v]| |h[r, k]| / count, the size of the terms that gradient sums."""
    m = run_["model"]
    x = run_["x"].double()
    wn = m.model.norm.weight.detach().double()
    wh = m.lm_head.weight.detach().double().requires_grad_()
    h = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + m.cfg.norm_eps) * wn
    z = h @ wh.t()
    c = C * torch.tanh(z / C) if C else z
    lse = torch.logsumexp(c, -1)
    tg = run_["tgt"]
    rows = torch.where(tg != -1, lse - c.gather(-1, tg.clamp(min=0)[:, None])[:, 0] + B * lse * lse,
                       torch.zeros_like(lse))
    count = (tg != -1).sum().clamp(min=1)
    dz, dw = torch.autograd.grad(rows.sum() / count, (z, wh))
    return (rows.sum() / count).detach(), dw, dz.abs().t() @ h.abs()


@pytest.mark.parametrize("chunk", [128, 384])
@pytest.mark.parametrize("C,B", [(30.0, 0.1), (2.0, 0.1)], ids=["cap30_z0.1", "cap2_z0.1"])
def test_model_chunked_head_against_unchunked(C, B, chunk):
    """fp32 on the CPU, 512 rows.  The loss as tests/test_head_chunk_cpu.py compares it: the chunked error against
    float64 at most the unchunked one plus one fp32 rounding.  The head's weight gradient of either path against
    float64, element by element, within K 2^-23 sum_r |dz[r, v] h[r, k]| / count with K = 64.  Per term: the exponent
    c - lse (|c| <= 9, lse about 7 here) carries the tanh's and the log-sum-exp's two roundings each and its own,
    2 * 9 + 2 * 7 + 9 = 41 roundings of size 2^-23 at the very most, in practice a handful; the factors 1 + 2 B lse,
    the one-hot and 1 - t^2 add 6; the sum over 512 rows in blocks of the product adds log2(512) = 9, a chunk's
    accumulation into the slot one per chunk (4), the 1 / count scale 2: 62.  A wrong factor anywhere is an error of
    the size of the terms themselves, 2^23 / 64 times the bound."""
    cfg = _cfg(256, final_softcap=C, lm_z_loss_coef=B)
    torch.manual_seed(0)
    base = _scaled_up(build_model(cfg), 20.0)
    idx, tgt = _batch(cfg, 256)
    off, chk = _head_run(cfg, base, None, idx, tgt), _head_run(cfg, base, chunk, idx, tgt)
    R, V = 512, cfg.vocab_size
    assert [s for s, _ in off["saved"]].count((R, V)) == 1 and (R, V) not in [s for s, _ in chk["saved"]]
    assert max(math.prod(s) for s, _ in chk["saved"]) == R * cfg.n_embd     # nothing larger than x and h is kept
    assert torch.equal(off["x"], chk["x"])
    loss64, dw64, terms = _head64(chk, C, B)
    e_u, e_c = (abs(r["loss"].double() - loss64).item() for r in (off, chk))
    print(f"chunk {chunk}: loss error vs float64 unchunked {e_u:.3e} chunked {e_c:.3e}")
    assert e_c <= e_u + EPS32 * abs(loss64.item())
    for what, r in (("unchunked", off), ("chunked", chk)):
        err = (r["grads"]["lm_head.weight"].double() - dw64).abs()
        print(f"chunk {chunk}: head dW {what}: worst error / bound {(err / (64 * EPS32 * terms)).max().item():.3f}")
        assert (err <= 64 * EPS32 * terms).all(), what
    for n, g in chk["grads"].items():
        assert g is not None and torch.isfinite(g).all(), n


@pytest.mark.parametrize("chunk", [None, 16])
def test_both_options_zero_is_a_config_without_the_fields(chunk, monkeypatch):
    """Parameters, saved tensors, the ops' calls and a step's results with ``final_softcap = lm_z_loss_coef = 0``
    against a model whose config has no such fields at all."""
    cfg = _cfg(final_softcap=0.0, lm_z_loss_coef=0.0)
    torch.manual_seed(0)
    base = build_model(cfg)
    idx, tgt = _batch(cfg)

    class Bare:
        """cfg without the two fields: reading either raises AttributeError."""

        def __getattr__(self, name):
            if name in ("final_softcap", "lm_z_loss_coef"):
                raise AttributeError(name)
            return getattr(cfg, name)

    calls = []
    for name in ("xent_fwd_bwd_", "xent_lse", "xent_bwd_lse_"):
        real = getattr(F_, name)
        monkeypatch.setattr(F_, name, (lambda real, name: lambda *a, **kw: (calls.append((name, len(a), sorted(kw))),
                                                                           real(*a, **kw))[1])(real, name))
    on = _head_run(cfg, base, chunk, idx, tgt)
    n_on = len(calls)
    assert n_on > 0 and all(kw == [] for _, _, kw in calls), calls      # today's calls: no option is passed
    # the head as it was before the fields existed: the same calls, spelled without the helper
    from dltb.models import mistral
    monkeypatch.setattr(mistral, "_head_loss_opts", lambda c: {})
    monkeypatch.setattr(mistral, "_capped_logits", lambda logits, cap, copy_: logits.clone() if copy_ else logits)
    bare = _head_run(Bare(), base, chunk, idx, tgt)
    assert calls[n_on:] == calls[:n_on]
    assert on["saved"] == bare["saved"]
    assert torch.equal(on["loss"], bare["loss"])
    assert list(on["grads"]) == list(bare["grads"])
    for n, g in on["grads"].items():
        assert torch.equal(g, bare["grads"][n]), n
