"""Attention logit soft-capping (``ModelConfig.attn_softcap`` / ``--attn-softcap``) on the CPU: the reference
definitions ``ops/ref.py attn_fwd`` / ``attn_bwd`` with ``softcap=`` against a direct float64 computation from the
definition -- z = cap * tanh(x / cap) on the raw scores, the masks after the cap, softmax over the visible z -- and
its autograd gradients, ``softcap=0`` against the call without the argument, the refusals, configuration, the flag,
the sidecar, and the mtiny model against ``models/oracle.py`` and against ``ref``.
The GPU kernels: tests/test_attn_softcap_gpu.py.

Tolerances: those tests/test_attn_sinks_cpu.py uses for the same quantities -- the reference against the explicit
float64 formulation and its autograd gradients within 1e-9 of the larger of 1 and the largest wanted value; the model
against the oracle with loss atol 1e-10, gradients atol 1e-9 / rtol 1e-7.
"""
import math

import pytest
import torch

import dltb  # noqa: F401
from dltb.harness import build_parser, check_attn_softcap
from dltb.models import build_model, get_model_config
from dltb.models.config import ModelConfig
from dltb.models.oracle import OracleMistral
from dltb.ops import ref

F64 = torch.float64
B, T, Hq, Hkv, D = 2, 512, 4, 2, 16


def _doc_bounds(seed=5):
    """Bounds of a seeded packed row: documents of random lengths, EOS = 1."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.zeros(B, T, dtype=torch.int64)
    for b in range(B):
        pos = 0
        while pos < T:
            pos += int(torch.randint(1, 150, (1,), generator=g))
            if pos - 1 < T:
                idx[b, pos - 1] = 1
    return ref.doc_bounds(idx, 1, 0)


CASES = {"causal": dict(), "window100": dict(window=100), "doc": dict(bounds=True), "qrange": dict(q_range=(128, 384))}
# cap 50 (Gemma-2) barely bends N(0, 1) scores; cap 1.5 saturates a good share of them
CAPS = [50.0, 1.5]


def _case(name):
    kw = dict(CASES[name])
    if kw.get("bounds"):
        kw["bounds"] = _doc_bounds()
    return kw


def _inputs(seed, q_range=None, qmul=1.0):
    g = torch.Generator().manual_seed(seed)
    Tq = T if q_range is None else q_range[1] - q_range[0]
    q = torch.randn(B * Tq, Hq * D, generator=g, dtype=F64) * qmul
    k = torch.randn(B * T, Hkv * D, generator=g, dtype=F64)
    v = torch.randn(B * T, Hkv * D, generator=g, dtype=F64)
    do = torch.randn(B * Tq, Hq * D, generator=g, dtype=F64)
    return q, k, v, do


def _explicit(q, k, v, cap, scale, window=0, bounds=None, q_range=None):
    """x = scale q.k, z = cap tanh(x / cap), masked after the cap, softmax over the visible z.  Returns
    (o [B * Tq, Hq * D], lse [B, Hq, Tq]); written from the definition, not from ref's helpers."""
    qb, qe = q_range or (0, T)
    Tq = qe - qb
    qh = q.view(B, Tq, Hq, D).transpose(1, 2)
    kh = k.view(B, T, Hkv, D).transpose(1, 2).repeat_interleave(Hq // Hkv, 1)
    vh = v.view(B, T, Hkv, D).transpose(1, 2).repeat_interleave(Hq // Hkv, 1)
    x = (qh @ kh.transpose(-1, -2)) * scale
    z = cap * torch.tanh(x / cap)
    i = torch.arange(qb, qe)[:, None]
    j = torch.arange(T)[None, :]
    vis = (j <= i).expand(B, Tq, T)
    if window:
        vis = vis & (j > i - window)
    if bounds is not None:
        vis = vis & (j[None] >= bounds[0][:, qb:qe, None].long())
    z = z.masked_fill(~vis[:, None], float("-inf"))
    lse = torch.logsumexp(z, -1)
    p = torch.exp(z - lse[..., None])
    o = (p @ vh).transpose(1, 2).reshape(B * Tq, Hq * D)
    return o, lse


def _close(got, want, what):
    err = float((got - want).abs().max())
    assert err <= 1e-9 * max(1.0, float(want.abs().max())), (what, err)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name", list(CASES))
def test_reference_against_the_definition_float64(name, cap):
    kw = _case(name)
    q, k, v, do = _inputs(3, kw.get("q_range"), qmul=2.0)
    scale = 1.0 / math.sqrt(D)
    o, lse = ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.0, None, 0, softcap=cap, **kw)
    assert o.dtype == F64 and lse.dtype == F64
    qe, ke, ve = (t.clone().requires_grad_() for t in (q, k, v))
    want_o, want_lse = _explicit(qe, ke, ve, cap, scale, **kw)
    _close(o, want_o.detach(), "o")
    _close(lse, want_lse.detach(), "lse")
    # the cap is visible: no capped score exceeds it, and the uncapped call gives another lse
    assert float(lse.max()) <= cap + math.log(T)
    _, plain = ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.0, None, 0, **kw)
    assert float((plain - lse).abs().max()) > (1e-3 if cap == 50.0 else 0.5)
    # ---- backward against autograd through the explicit formulation
    (want_o * do).sum().backward()
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    assert ref.attn_bwd(q, k, v, o, do, lse, dq, dk, dv, B, T, Hq, Hkv, scale, True, 0.0, None, 0, softcap=cap,
                        **kw) is None
    _close(dq, qe.grad, "dq")
    _close(dk, ke.grad, "dk")
    _close(dv, ve.grad, "dv")


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, F64], ids=["fp32", "bf16", "fp64"])
def test_softcap_zero_is_the_call_without_the_argument(name, dtype):
    kw = _case(name)
    q, k, v, do = (t.to(dtype) for t in _inputs(4, kw.get("q_range")))
    scale = 1.0 / math.sqrt(D)
    o0, lse0 = ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.0, None, 0, **kw)
    o1, lse1 = ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.0, None, 0, softcap=0.0, **kw)
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1)
    g0 = [torch.empty_like(t) for t in (q, k, v)]
    g1 = [torch.empty_like(t) for t in (q, k, v)]
    ref.attn_bwd(q, k, v, o0, do, lse0, *g0, B, T, Hq, Hkv, scale, True, 0.0, None, 0, **kw)
    ref.attn_bwd(q, k, v, o1, do, lse1, *g1, B, T, Hq, Hkv, scale, True, 0.0, None, 0, softcap=0.0, **kw)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    # the functional layer's CPU path too, and through it softcap=0 with non-causal attention and dropout is allowed
    from dltb.ops import functional as F_
    o2, lse2, _ = F_.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.0, None, 0, softcap=0.0, **kw)
    assert torch.equal(o0, o2) and torch.equal(lse0, lse2)


def test_check_softcap_refusals():
    ref.check_softcap(0, False, 0.1, object())          # off: nothing else is looked at
    ref.check_softcap(0.0, True, 0.0, None)
    ref.check_softcap(50.0, True, 0.0, None)
    ref.check_softcap(50, True, 0.0, None)
    for bad in (-1.0, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="softcap must be"):
            ref.check_softcap(bad, True, 0.0, None)
    with pytest.raises(ValueError, match="causal"):
        ref.check_softcap(50.0, False, 0.0, None)
    with pytest.raises(ValueError, match="dropout"):
        ref.check_softcap(50.0, True, 0.1, None)
    with pytest.raises(ValueError, match="sink"):
        ref.check_softcap(50.0, True, 0.0, torch.zeros(Hq))
    q, k, v, do = _inputs(1)
    scale = 1.0 / math.sqrt(D)
    with pytest.raises(ValueError, match="causal"):
        ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, False, 0.0, None, 0, softcap=50.0)
    with pytest.raises(ValueError, match="sink"):
        ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.0, None, 0, sink=torch.zeros(Hq, dtype=F64), softcap=50.0)
    with pytest.raises(ValueError, match="softcap must be"):
        ref.attn_bwd(q, k, v, q, do, torch.zeros(B, Hq, T, dtype=F64), q.clone(), k.clone(), v.clone(), B, T, Hq, Hkv,
                     scale, True, 0.0, None, 0, softcap=-2.0)


# ------------------------------------------------------------------------------------------- config, flag
def _cfg(T_=32, **kw):
    return ModelConfig(**dict(get_model_config("mtiny", T_).to_dict(), **kw))


def test_config_validation():
    assert get_model_config("mtiny", 32).attn_softcap == 0.0
    assert _cfg(attn_softcap=50.0).attn_softcap == 50.0
    assert _cfg(attn_softcap=30).attn_softcap == 30
    with pytest.raises(ValueError, match="attn_softcap"):
        ModelConfig(**dict(get_model_config("tiny", 32).to_dict(), attn_softcap=50.0))
    for bad in (-1.0, float("nan"), float("inf"), True, "50"):
        with pytest.raises(ValueError, match="attn_softcap"):
            _cfg(attn_softcap=bad)
    with pytest.raises(ValueError, match="attn_sinks"):
        _cfg(attn_softcap=50.0, attn_sinks=True)
    cfg = get_model_config("tiny", 32)
    cfg.attn_softcap = 50.0
    with pytest.raises(ValueError, match="attn_softcap"):
        cfg.validate()
    old = {k: v for k, v in get_model_config("mtiny", 32).to_dict().items() if k != "attn_softcap"}
    assert ModelConfig(**old).attn_softcap == 0.0


def test_no_parameter_and_flops_unchanged():
    on, off = _cfg(attn_softcap=50.0), _cfg()
    assert on.num_params() == off.num_params()
    assert on.train_flops_per_token(32) == off.train_flops_per_token(32)
    assert on.train_flops_per_token(32, 100) == off.train_flops_per_token(32, 100)
    torch.manual_seed(0)
    a = build_model(on)
    torch.manual_seed(0)
    b = build_model(off)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    assert [n for u in a.units() for n in u.names] == [n for u in b.units() for n in u.names]
    assert list(OracleMistral(on).state_dict().keys()) == list(b.state_dict().keys())


def test_flag_parses_and_refusals(tmp_path, capsys):
    base = ["--strategy", "zero3", "--tier", "mtiny", "--seq-len", "32", "--steps", "1", "--per-device-batch", "1",
            "--grad-accum", "1", "--results-dir", str(tmp_path / "res"), "--device", "cpu"]
    assert build_parser().parse_args(base).attn_softcap == 0.0
    assert build_parser().parse_args(base + ["--attn-softcap", "50"]).attn_softcap == 50.0
    cfg = get_model_config("mtiny", 32)
    check_attn_softcap(0.0, False, cfg, "mtiny")
    assert cfg.attn_softcap == 0.0
    check_attn_softcap(50.0, False, cfg, "mtiny")
    assert cfg.attn_softcap == 50.0
    with pytest.raises(ValueError, match="--attn-softcap needs a causal tier"):
        check_attn_softcap(50.0, False, get_model_config("tiny", 32), "tiny")
    with pytest.raises(ValueError, match="--attn-softcap together with --attn-sinks"):
        check_attn_softcap(50.0, True, get_model_config("mtiny", 32), "mtiny")
    for bad in (-3.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="--attn-softcap must be"):
            check_attn_softcap(bad, False, get_model_config("mtiny", 32), "mtiny")
    from dltb.harness import main
    args = base + ["--attn-softcap", "50"]
    args[args.index("mtiny")] = "tiny"
    with pytest.raises(SystemExit) as e:
        main(args)
    assert e.value.code == 2
    assert "--attn-softcap needs a causal tier" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        main(base + ["--attn-softcap", "50", "--attn-sinks"])
    assert e.value.code == 2
    assert "--attn-softcap together with --attn-sinks" in capsys.readouterr().err
    assert not (tmp_path / "res").exists()


# ------------------------------------------------------------------------------------------- whole model
def _scaled_up(m, mul=6.0):
    """Larger query / key projections, so that the scores reach the cap at the model's initialisation scale."""
    with torch.no_grad():
        for layer in m.model.layers:
            layer.self_attn.qkv_proj.weight.mul_(mul)
    return m


@pytest.mark.parametrize("kw", [dict(), dict(sliding_window=20), dict(qk_norm=True), dict(doc_eos_id=7),
                                dict(n_experts=4, moe_top_k=2)],
                         ids=["causal", "window", "qknorm", "doc", "moe"])
@pytest.mark.parametrize("cap", [50.0, 2.0])
def test_model_against_oracle_float64(kw, cap):
    """The CPU model path runs ``ref.attn_fwd`` / ``ref.attn_bwd`` with the cap (ops/functional.py); the oracle is
    autograd through its explicit softmax.  The run without the cap gives another loss."""
    cfg = _cfg(attn_softcap=cap, **kw)
    torch.manual_seed(0)
    m = _scaled_up(build_model(cfg)).double()
    o = OracleMistral(cfg).double()
    o.load_state_dict(m.state_dict())
    idx = torch.randint(0, cfg.vocab_size if "doc_eos_id" not in kw else 16, (2, 32),
                        generator=torch.Generator().manual_seed(2))
    tgt = idx.roll(-1, 1)
    tgt[1, -5:] = -1
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
    # the cap changes the model: the same weights without it
    off = OracleMistral(_cfg(**kw)).double()
    off.load_state_dict(m.state_dict())
    _, l_off = off(idx, tgt)
    assert abs(l_off.item() - lo.item()) > (1e-6 if cap == 50.0 else 1e-3), (l_off.item(), lo.item())


@pytest.mark.parametrize("mode", ["selective", "full"])
def test_recompute_equals_off_bit_for_bit(mode):
    import copy
    from dltb.parallel import ParamRuntime
    cfg = _cfg(attn_softcap=2.0)
    torch.manual_seed(0)
    m = _scaled_up(build_model(cfg))
    idx = torch.randint(0, cfg.vocab_size, (2, 32), generator=torch.Generator().manual_seed(4))
    out = []
    for md in ("off", mode):
        mm = copy.deepcopy(m)
        mm.rt = ParamRuntime()
        mm.activation_recompute = md
        loss = mm(idx, idx.roll(-1, 1))[1]
        loss.backward()
        out.append((loss.detach(), {n: p.grad.clone() for n, p in mm.named_parameters()}))
    assert torch.equal(out[0][0], out[1][0])
    for n in out[0][1]:
        assert torch.equal(out[0][1][n], out[1][1][n]), n


def test_world2_cp2_equals_world1_cpu(tmp_path):
    """Two gloo ranks as one context-parallel group (zigzag ranges, the query-range calls with the cap) against the
    one-rank whole-row run; the comparison of tests/test_attn_sinks_cpu.py."""
    from multirank_util import compare, run
    extra = ("--cases", "cp_zero3", "--attn-softcap", "2", "--seq-len", "512", "--windows", "2")
    ws1 = run(tmp_path / "ws1.pt", 1, "cpu", extra=extra)
    ws2 = run(tmp_path / "ws2.pt", 2, "cpu", extra=extra + ("--context-parallel", "2"))
    bad = compare(ws1, ws2, loss_tol=1e-4, upd_tol=1e-3, cos_min=0.99999, param_tol=1e-3)
    assert not bad, bad
    # the cap reached the run: without it the same case trains other losses
    ws0 = run(tmp_path / "ws0.pt", 1, "cpu", extra=("--cases", "cp_zero3", "--seq-len", "512", "--windows", "2"))
    assert ws0["cp_zero3"]["losses"] != ws1["cp_zero3"]["losses"]


# ------------------------------------------------------------------------------------------- harness
def test_harness_sidecar_and_line(tmp_path, capsys):
    import json
    import os
    from dltb.harness import main
    os.environ.pop("WORLD_SIZE", None)

    def args(res, *more):
        return ["--strategy", "zero3", "--tier", "mtiny", "--seq-len", "32", "--steps", "2", "--warmup-steps", "1",
                "--per-device-batch", "2", "--grad-accum", "1", "--results-dir", str(res), "--device", "cpu",
                "--log-every", "0", *more]
    res = tmp_path / "res"
    assert main(args(res, "--attn-softcap", "50")) == 0
    assert "attention soft-capping: scores capped to 50 * tanh(x / 50)" in capsys.readouterr().out
    ext = [f for f in os.listdir(res) if f.endswith(".extended.json")]
    side = json.loads((res / ext[0]).read_text())
    assert side["attn_softcap"] == 50.0 and side["model"]["attn_softcap"] == 50.0
    assert main(args(tmp_path / "res2")) == 0
    assert "attention soft-capping" not in capsys.readouterr().out
    ext = [f for f in os.listdir(tmp_path / "res2") if f.endswith(".extended.json")]
    side2 = json.loads((tmp_path / "res2" / ext[0]).read_text())
    assert side2["attn_softcap"] == 0.0 and side2["model"]["attn_softcap"] == 0.0
    assert side["train_flops_per_token"] == side2["train_flops_per_token"]
    assert side["params"] == side2["params"]
