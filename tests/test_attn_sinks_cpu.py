"""Learned attention sinks (``ModelConfig.attn_sinks`` / ``--attn-sinks``) on the CPU: the reference definitions
``ops/ref.py attn_fwd`` / ``attn_bwd`` with ``sink=`` against the explicit formulation -- softmax over [scores | sink],
last column dropped -- and its autograd gradients in float64, a sink of -30000 against the sink-less reference,
configuration, parameter order, the flag, and the mtiny model against ``models/oracle.py``.
The GPU kernels: tests/test_attn_sinks_gpu.py.

Tolerances: the manual backward against autograd uses the comparison of tests/test_qknorm_cpu.py (1e-9 of the larger of
1 and the largest wanted value, both sides float64); the model against the oracle uses tests/test_mistral_cpu.py's
(loss atol 1e-10, gradients atol 1e-9 / rtol 1e-7).
"""
import math

import pytest
import torch

import dltb  # noqa: F401
from dltb.harness import build_parser, check_attn_sinks
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


def _case(name):
    kw = dict(CASES[name])
    if kw.get("bounds"):
        kw["bounds"] = _doc_bounds()
    return kw


def _inputs(seed, q_range=None):
    g = torch.Generator().manual_seed(seed)
    Tq = T if q_range is None else q_range[1] - q_range[0]
    q = torch.randn(B * Tq, Hq * D, generator=g, dtype=F64)
    k = torch.randn(B * T, Hkv * D, generator=g, dtype=F64)
    v = torch.randn(B * T, Hkv * D, generator=g, dtype=F64)
    do = torch.randn(B * Tq, Hq * D, generator=g, dtype=F64)
    sink = 2.0 * torch.randn(Hq, generator=g, dtype=F64)
    return q, k, v, do, sink


def _explicit(q, k, v, sink, scale, window=0, bounds=None, q_range=None):
    """softmax over [scores | sink] of every query row, the sink column dropped before the product with v.
    Returns (o [B * Tq, Hq * D], lse [B, Hq, Tq]); written from the definition, not from ref's helpers."""
    qb, qe = q_range or (0, T)
    Tq = qe - qb
    qh = q.view(B, Tq, Hq, D).transpose(1, 2)
    kh = k.view(B, T, Hkv, D).transpose(1, 2).repeat_interleave(Hq // Hkv, 1)
    vh = v.view(B, T, Hkv, D).transpose(1, 2).repeat_interleave(Hq // Hkv, 1)
    s = (qh @ kh.transpose(-1, -2)) * scale
    i = torch.arange(qb, qe)[:, None]
    j = torch.arange(T)[None, :]
    vis = (j <= i).expand(B, Tq, T)
    if window:
        vis = vis & (j > i - window)
    if bounds is not None:
        vis = vis & (j[None] >= bounds[0][:, qb:qe, None].long())
    s = s.masked_fill(~vis[:, None], float("-inf"))
    ext = torch.cat([s, sink.view(1, Hq, 1, 1).expand(B, Hq, Tq, 1)], -1)
    p = torch.softmax(ext, -1)[..., :T]
    o = (p @ vh).transpose(1, 2).reshape(B * Tq, Hq * D)
    return o, torch.logsumexp(ext, -1)


def _close(got, want, what):
    err = float((got - want).abs().max())
    assert err <= 1e-9 * max(1.0, float(want.abs().max())), (what, err)


@pytest.mark.parametrize("name", list(CASES))
def test_reference_against_explicit_softmax_float64(name):
    kw = _case(name)
    q, k, v, do, sink = _inputs(3, kw.get("q_range"))
    scale = 1.0 / math.sqrt(D)
    o, lse = ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.0, None, 0, sink=sink, **kw)
    assert o.dtype == F64 and lse.dtype == F64
    qe, ke, ve, se = (t.clone().requires_grad_() for t in (q, k, v, sink))
    want_o, want_lse = _explicit(qe, ke, ve, se, scale, **kw)
    _close(o, want_o.detach(), "o")
    _close(lse, want_lse.detach(), "lse")
    # the rows' probabilities sum to less than one: the sink takes its share
    assert bool((lse > torch.logsumexp(ref._attn_probs(q, k, B, T, Hq, Hkv, D, scale, True, kw.get("window", 0),
                                                       kw.get("bounds"), *(kw.get("q_range") or (0, T))), -1)).all())
    # ---- backward against autograd through the explicit formulation
    (want_o * do).sum().backward()
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ds = ref.attn_bwd(q, k, v, o, do, lse, dq, dk, dv, B, T, Hq, Hkv, scale, True, 0.0, None, 0, sink=sink, **kw)
    assert tuple(ds.shape) == (1, Hq) and ds.dtype == F64
    _close(dq, qe.grad, "dq")
    _close(dk, ke.grad, "dk")
    _close(dv, ve.grad, "dv")
    _close(ds[0], se.grad, "dsink")
    assert float(se.grad.abs().min()) > 0


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, F64], ids=["fp32", "bf16", "fp64"])
def test_very_negative_sink_is_the_sinkless_reference(name, dtype):
    kw = _case(name)
    q, k, v, do, _ = (t.to(dtype) for t in _inputs(4, kw.get("q_range")))
    sink = torch.full((Hq,), -30000.0, dtype=dtype)
    scale = 1.0 / math.sqrt(D)
    o0, lse0 = ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.0, None, 0, **kw)
    o1, lse1 = ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.0, None, 0, sink=sink, **kw)
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1)
    g0 = [torch.empty_like(t) for t in (q, k, v)]
    g1 = [torch.empty_like(t) for t in (q, k, v)]
    assert ref.attn_bwd(q, k, v, o0, do, lse0, *g0, B, T, Hq, Hkv, scale, True, 0.0, None, 0, **kw) is None
    ds = ref.attn_bwd(q, k, v, o1, do, lse1, *g1, B, T, Hq, Hkv, scale, True, 0.0, None, 0, sink=sink, **kw)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    assert bool((ds == 0).all())


def test_reference_refuses_a_bad_sink():
    q, k, v, _, sink = _inputs(1)
    scale = 1.0 / math.sqrt(D)
    with pytest.raises(ValueError, match="causal"):
        ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, False, 0.0, None, 0, sink=sink)
    with pytest.raises(ValueError, match="dropout"):
        ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.1, None, 0, sink=sink)
    with pytest.raises(ValueError, match="Hq"):
        ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.0, None, 0, sink=sink[:-1])
    with pytest.raises(ValueError, match="dtype"):
        ref.attn_fwd(q, k, v, B, T, Hq, Hkv, scale, True, 0.0, None, 0, sink=sink.float())


# ------------------------------------------------------------------------------------------- config, parameters, flag
DENSE = ["input_layernorm.weight", "self_attn.qkv_proj.weight", "self_attn.o_proj.weight",
         "post_attention_layernorm.weight", "mlp.gate_up_proj.weight", "mlp.down_proj.weight"]
QK = ["self_attn.q_norm.weight", "self_attn.k_norm.weight"]


def _cfg(T_=32, **kw):
    return ModelConfig(**dict(get_model_config("mtiny", T_).to_dict(), **kw))


def test_config_validation():
    assert get_model_config("mtiny", 32).attn_sinks is False
    assert _cfg(attn_sinks=True).attn_sinks is True
    with pytest.raises(ValueError, match="attn_sinks"):
        ModelConfig(**dict(get_model_config("tiny", 32).to_dict(), attn_sinks=True))
    with pytest.raises(ValueError, match="attn_sinks"):
        _cfg(attn_sinks=1)
    cfg = get_model_config("tiny", 32)
    cfg.attn_sinks = True
    with pytest.raises(ValueError, match="attn_sinks"):
        cfg.validate()
    old = {k: v for k, v in get_model_config("mtiny", 32).to_dict().items() if k != "attn_sinks"}
    assert ModelConfig(**old).attn_sinks is False


@pytest.mark.parametrize("qk", [False, True], ids=["plain", "qknorm"])
@pytest.mark.parametrize("experts", [None, 4], ids=["dense", "moe"])
def test_num_params_and_parameter_order(qk, experts):
    cfg = _cfg(attn_sinks=True, qk_norm=qk, n_experts=experts)
    off = _cfg(qk_norm=qk, n_experts=experts)
    model = build_model(cfg)
    assert cfg.num_params() == sum(p.numel() for p in model.parameters()) == model.num_params()
    assert cfg.num_params() - off.num_params() == cfg.n_layer * cfg.n_head
    assert cfg.train_flops_per_token(32) == off.train_flops_per_token(32)
    block = DENSE
    if experts:
        block = DENSE[:4] + ["mlp.router.weight"]
        for e in range(experts):
            block = block + [f"mlp.experts.{e}.gate_up_proj.weight", f"mlp.experts.{e}.down_proj.weight"]
    for i, layer in enumerate(model.model.layers):
        names = [n for n, _ in layer.param_list()]
        assert names == block + (QK if qk else []) + ["self_attn.sinks"]       # ..., q_norm, k_norm, sinks
        assert model.unit_blocks[i].names == [f"model.layers.{i}.{n}" for n in names]
        p = layer.param_list()[-1][1]
        assert tuple(p.shape) == (cfg.n_head,) and bool((p == 0).all())
    assert "model.layers.1.self_attn.sinks" in model.state_dict()


def test_flag_off_is_todays_model():
    cfg = get_model_config("mtiny", 32)
    torch.manual_seed(0)
    model = build_model(cfg)
    for i, layer in enumerate(model.model.layers):
        assert [n for n, _ in layer.param_list()] == DENSE
        assert not hasattr(layer.self_attn, "sinks")
    keys = ["model.embed_tokens.weight"]
    for i in range(cfg.n_layer):        # the registration order of the modules, as ever
        keys += [f"model.layers.{i}.{n}" for n in DENSE]
    keys += ["model.norm.weight", "lm_head.weight"]
    assert list(model.state_dict().keys()) == keys
    assert [n for u in model.units() for n in u.names] == keys
    assert list(OracleMistral(cfg).state_dict().keys()) == keys


def test_flag_parses_and_tinygpt_is_refused(tmp_path, capsys):
    base = ["--strategy", "zero3", "--tier", "mtiny", "--seq-len", "32", "--steps", "1", "--per-device-batch", "1",
            "--grad-accum", "1", "--results-dir", str(tmp_path / "res"), "--device", "cpu"]
    assert build_parser().parse_args(base).attn_sinks is False
    assert build_parser().parse_args(base + ["--attn-sinks"]).attn_sinks is True
    cfg = get_model_config("mtiny", 32)
    check_attn_sinks(False, cfg, "mtiny")
    assert cfg.attn_sinks is False
    check_attn_sinks(True, cfg, "mtiny")
    assert cfg.attn_sinks is True
    with pytest.raises(ValueError, match="--attn-sinks needs a causal tier"):
        check_attn_sinks(True, get_model_config("tiny", 32), "tiny")
    from dltb.harness import main
    args = base + ["--attn-sinks"]
    args[args.index("mtiny")] = "tiny"
    with pytest.raises(SystemExit) as e:
        main(args)
    assert e.value.code == 2
    assert "--attn-sinks needs a causal tier" in capsys.readouterr().err
    assert not (tmp_path / "res").exists()


# ------------------------------------------------------------------------------------------- whole model
def _perturb_sinks(m, seed=11):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in m.model.layers:
            layer.self_attn.sinks.add_(torch.randn(layer.self_attn.sinks.numel(), generator=g))


@pytest.mark.parametrize("kw", [dict(), dict(sliding_window=20), dict(qk_norm=True), dict(doc_eos_id=7)],
                         ids=["causal", "window", "qknorm", "doc"])
def test_model_against_oracle_float64(kw):
    cfg = _cfg(attn_sinks=True, **kw)
    torch.manual_seed(0)
    m = build_model(cfg)
    _perturb_sinks(m)
    m = m.double()
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
    n_sinks = 0
    for name, p in o.named_parameters():
        assert got[name].grad is not None, name
        assert torch.allclose(got[name].grad, p.grad, atol=1e-9, rtol=1e-7), name
        if name.endswith("sinks"):
            n_sinks += p.numel()
            assert float(p.grad.abs().min()) > 0, name
    assert n_sinks == cfg.n_layer * cfg.n_head


@pytest.mark.parametrize("mode", ["selective", "full"])
def test_recompute_equals_off_bit_for_bit(mode):
    import copy
    from dltb.parallel import ParamRuntime
    cfg = _cfg(attn_sinks=True)
    torch.manual_seed(0)
    m = build_model(cfg)
    _perturb_sinks(m)
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


# ------------------------------------------------------------------------------------------- engines
@pytest.mark.parametrize("case", ["ddp", "zero3_cp2"])
def test_world2_equals_world1_cpu(tmp_path, case):
    """Two gloo ranks against the one-rank run on the concatenated batch, mtiny with sinks (the comparison of
    tests/test_qknorm_cpu.py): the [2]-element parameters go through the flat layout (ddp); zero3_cp2: the two ranks
    are one context-parallel group, each range's call writes its row of one sink-gradient partial matrix."""
    from multirank_util import compare, run
    spec = {"ddp": "cp_ddp", "zero3_cp2": "cp_zero3"}[case]
    extra = ("--cases", spec, "--attn-sinks", "--seq-len", "512" if case == "zero3_cp2" else "64", "--windows", "2")
    ws1 = run(tmp_path / "ws1.pt", 1, "cpu", extra=extra)
    ws2 = run(tmp_path / "ws2.pt", 2, "cpu", extra=extra + (("--context-parallel", "2") if case == "zero3_cp2" else ()))
    names = [n for n in ws1[spec]["init"] if n.endswith("sinks")]
    assert len(names) == 2 and all(ws1[spec]["init"][n].numel() == 2 for n in names)
    bad = compare(ws1, ws2, loss_tol=1e-4, upd_tol=1e-3, cos_min=0.99999, param_tol=1e-3)
    assert not bad, bad
    for n in names:         # compare() skips small updates: the sinks are checked here
        u1 = ws1[spec]["final"][n] - ws1[spec]["init"][n]
        u2 = ws2[spec]["final"][n] - ws2[spec]["init"][n]
        assert float(u1.norm()) > 0, n
        assert float((u1 - u2).norm()) <= 1e-3 * float(u1.norm()), n


# ------------------------------------------------------------------------------------------- harness
def test_harness_sidecar_checkpoint_resume_export(tmp_path, capsys):
    import json
    import os
    from dltb.harness import main
    from safetensors.torch import load_file
    os.environ.pop("WORLD_SIZE", None)

    def args(res, *more):
        return ["--strategy", "zero3", "--tier", "mtiny", "--seq-len", "32", "--steps", "2", "--warmup-steps", "1",
                "--per-device-batch", "2", "--grad-accum", "1", "--results-dir", str(res), "--device", "cpu",
                "--log-every", "0", *more]
    res = tmp_path / "res"
    assert main(args(res, "--attn-sinks", "--save-dir", str(tmp_path / "ck"), "--export-model",
                     str(tmp_path / "m.safetensors"))) == 0
    assert "attention sinks: one learned logit per query head" in capsys.readouterr().out
    ext = [f for f in os.listdir(res) if f.endswith(".extended.json")]
    side = json.loads((res / ext[0]).read_text())
    assert side["attn_sinks"] is True and side["model"]["attn_sinks"] is True
    sd = load_file(str(tmp_path / "m.safetensors"))
    for i in range(2):
        s = sd[f"model.layers.{i}.self_attn.sinks"]
        assert tuple(s.shape) == (2,) and bool((s != 0).any())        # trained away from zero
    assert main(args(tmp_path / "res2", "--attn-sinks", "--resume", str(tmp_path / "ck"))) == 0
    with pytest.raises(Exception):      # a checkpoint of the flag-on model does not load into the flag-off model
        main(args(tmp_path / "res3", "--resume", str(tmp_path / "ck")))
    assert main(args(tmp_path / "res4")) == 0
    ext = [f for f in os.listdir(tmp_path / "res4") if f.endswith(".extended.json")]
    side = json.loads((tmp_path / "res4" / ext[0]).read_text())
    assert side["attn_sinks"] is False and side["model"]["attn_sinks"] is False
