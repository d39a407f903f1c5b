"""Sandwich norms (``ModelConfig.sandwich_norm`` / ``--sandwich-norm``) and the GeGLU FFN (``ModelConfig.ffn_act`` /
``--ffn-act geglu``) on the CPU: configuration, parameter order, the reference definitions ``ops/ref.py sandwich_fwd`` /
``sandwich_bwd`` / ``swiglu_*(act="geglu")`` against the float64 references of tests/sandwich_ref.py and torch
autograd, the mtiny model against ``models/oracle.py``, the zero-weight identity, the recompute modes, checkpoints and
the engines.  The GPU kernels: tests/test_sandwich_norm_gpu.py.

Tolerances.  The references run the same expressions in the tensors' own precision, so in float64 they match the
float64 references to a few 1e-13 relative; in a 16-bit format every output is one rounding (``half_ulp``) away from
the float64 value plus the fp32 evaluation, for which the GPU test's bounds (tests/sandwich_ref.py) are used as they
are -- torch's fp32 rsqrt / tanh are at least as accurate as the H = 2^-20 assumed for the hardware's.
"""
import copy
import json
import os

import pytest
import torch

import dltb  # noqa: F401
from dltb.harness import build_parser, check_ffn_act, check_sandwich_norm
from dltb.models import build_model, get_model_config
from dltb.models.config import ModelConfig
from dltb.models.oracle import OracleMistral
from dltb.ops import functional as F_
from dltb.ops import ref
from dltb.parallel import ParamRuntime, engine_config, make_engine

from multirank_util import compare, run
from rowwise_ref import half_ulp, rmsnorm64
from sandwich_ref import (MARGIN, U, fwd_bounds, geglu64, geglu_bounds, geglu_grad64, gelu_tanh64, gelu_tanh_grad64,
                          norm_y_bounds, rms_dx_bound, sandwich64, sandwich_autograd64, sandwich_bwd64)

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
FORMATS = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
EPS = 1e-5
DENSE = ["input_layernorm.weight", "self_attn.qkv_proj.weight", "self_attn.o_proj.weight",
         "post_attention_layernorm.weight", "mlp.gate_up_proj.weight", "mlp.down_proj.weight"]
QK = ["self_attn.q_norm.weight", "self_attn.k_norm.weight"]
OUT = ["self_attn.out_norm.weight", "mlp.out_norm.weight"]
SINK = ["self_attn.sinks"]


def _cfg(T=32, **kw):
    return ModelConfig(**dict(get_model_config("mtiny", T).to_dict(), **kw))


FLAG_SETS = [dict(sandwich_norm=True), dict(ffn_act="geglu"), dict(sandwich_norm=True, ffn_act="geglu")]
FLAG_IDS = ["sandwich", "geglu", "both"]


# ------------------------------------------------------------------------------------------- config and flags
def test_tinygpt_refuses_both_flags():
    for kw, word in ((dict(sandwich_norm=True), "sandwich_norm"), (dict(ffn_act="geglu"), "ffn_act")):
        with pytest.raises(ValueError, match=word):
            ModelConfig(**dict(get_model_config("tiny", 32).to_dict(), **kw))
    with pytest.raises(ValueError, match="sandwich_norm must be a bool"):
        _cfg(sandwich_norm=1)
    with pytest.raises(ValueError, match="ffn_act must be one of"):
        _cfg(ffn_act="relu")
    for tier in ("A", "B", "tiny"):
        with pytest.raises(ValueError, match="--sandwich-norm needs a causal tier"):
            check_sandwich_norm(True, get_model_config(tier, 32), tier)
        with pytest.raises(ValueError, match="--ffn-act geglu needs a causal tier"):
            check_ffn_act("geglu", get_model_config(tier, 32), tier)
        check_sandwich_norm(False, get_model_config(tier, 32), tier)
        check_ffn_act("swiglu", get_model_config(tier, 32), tier)


def test_flags_parse_and_set_the_fields():
    base = ["--strategy", "zero3", "--tier", "mtiny", "--seq-len", "32", "--steps", "1", "--per-device-batch", "1",
            "--grad-accum", "1", "--results-dir", "x"]
    a = build_parser().parse_args(base)
    assert a.sandwich_norm is False and a.ffn_act == "swiglu"
    a = build_parser().parse_args(base + ["--sandwich-norm", "--ffn-act", "geglu"])
    assert a.sandwich_norm is True and a.ffn_act == "geglu"
    cfg = get_model_config("mtiny", 32)
    assert cfg.sandwich_norm is False and cfg.ffn_act == "swiglu"
    check_sandwich_norm(True, cfg, "mtiny")
    check_ffn_act("geglu", cfg, "mtiny")
    assert cfg.sandwich_norm is True and cfg.ffn_act == "geglu"
    old = {k: v for k, v in cfg.to_dict().items() if k not in ("sandwich_norm", "ffn_act")}
    assert ModelConfig(**old).sandwich_norm is False and ModelConfig(**old).ffn_act == "swiglu"


@pytest.mark.parametrize("sinks", [False, True], ids=["", "sinks"])
@pytest.mark.parametrize("qk", [False, True], ids=["", "qk"])
@pytest.mark.parametrize("on", [False, True], ids=["off", "on"])
def test_num_params_and_tail_order(on, qk, sinks):
    """All eight flag combinations: the tail is the QK-norm pair, the out-norm pair, the sinks."""
    for experts in (None, 4):
        cfg = _cfg(sandwich_norm=on, qk_norm=qk, attn_sinks=sinks, n_experts=experts)
        model = build_model(cfg)
        assert cfg.num_params() == sum(p.numel() for p in model.parameters()) == model.num_params()
        plain = ModelConfig(**dict(cfg.to_dict(), sandwich_norm=False))
        assert cfg.num_params() - plain.num_params() == (2 * cfg.n_embd * cfg.n_layer if on else 0)
        assert cfg.train_flops_per_token(32) == plain.train_flops_per_token(32)
        head = DENSE
        if experts:
            head = DENSE[:4] + ["mlp.router.weight"]
            for e in range(experts):
                head = head + [f"mlp.experts.{e}.gate_up_proj.weight", f"mlp.experts.{e}.down_proj.weight"]
        want = head + (QK if qk else []) + (OUT if on else []) + (SINK if sinks else [])
        for i, layer in enumerate(model.model.layers):
            names = [n for n, _ in layer.param_list()]
            assert names == want
            assert model.unit_blocks[i].names == [f"model.layers.{i}.{n}" for n in names]
            ws = [p for _, p in layer.param_list()]
            from dltb.models import mistral
            nb, qkn, sink = mistral._attn_tail(cfg, ws)
            assert nb == len(head)
            assert (qkn is None) is (not qk) and (qk is False or (qkn[0] is ws[nb] and qkn[1] is ws[nb + 1]))
            assert (sink is None) is (not sinks) and (sinks is False or sink is ws[-1])
            jo = mistral._out_norm_index(cfg, ws)
            if on:
                assert names[jo:jo + 2] == OUT
                for p in ws[jo:jo + 2]:
                    assert tuple(p.shape) == (cfg.n_embd,) and bool((p == 1).all())
            else:
                assert jo is None and not hasattr(layer.self_attn, "out_norm") and not hasattr(layer.mlp, "out_norm")
        sd = model.state_dict()
        assert ("model.layers.0.self_attn.out_norm.weight" in sd) is on
        assert ("model.layers.1.mlp.out_norm.weight" in sd) is on


def test_flags_off_keep_the_parents_names():
    cfg = _cfg()
    m = build_model(cfg)
    keys = ["model.embed_tokens.weight"]
    for i in range(cfg.n_layer):
        keys += [f"model.layers.{i}.{n}" for n in
                 ("input_layernorm.weight", "self_attn.qkv_proj.weight", "self_attn.o_proj.weight",
                  "post_attention_layernorm.weight", "mlp.gate_up_proj.weight", "mlp.down_proj.weight")]
    keys += ["model.norm.weight", "lm_head.weight"]
    assert list(m.state_dict().keys()) == keys
    assert [n for u in m.units() for n in u.names] == keys
    assert list(OracleMistral(cfg).state_dict().keys()) == keys


# ------------------------------------------------------------------------------------------- kernel references
def _rows(dtype, N, d, seed):
    """As tests/test_qknorm_gpu.py ``inputs``: an all-zero a row, an all-zero x row, in fp16 an a row scaled to 2^14;
    weights 1 + 0.5 randn."""
    g = torch.Generator().manual_seed(seed)
    x, a = torch.randn(N, d, generator=g), torch.randn(N, d, generator=g)
    if N > 4:
        a[1] = 0.0
        x[2] = 0.0
        if dtype == F16:
            a[3] *= 2.0 ** 14 / float(a[3].abs().max())
    w_out = (1.0 + 0.5 * torch.randn(d, generator=g)).to(dtype)
    w_next = (1.0 + 0.5 * torch.randn(d, generator=g)).to(dtype)
    dy, dres = torch.randn(N, d, generator=g).to(dtype), torch.randn(N, d, generator=g).to(dtype)
    return x.to(dtype), a.to(dtype), w_out, w_next, dy, dres


def _within(what, got, want, bound):
    got, want = got.double(), want.double()
    assert bool(torch.isfinite(want).all()), f"{what}: the float64 reference is not finite"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    err = (got - want).abs()
    nbad = int((err > bound).sum())
    assert nbad == 0, f"{what}: {nbad} of {got.numel()} outside their bound, worst {float((err / bound).max()):.3f}"


@FORMATS
@pytest.mark.parametrize("N,d", [(1, 8), (7, 128), (301, 520)])
def test_reference_in_both_formats_against_float64(dtype, N, d):
    """ref.sandwich_fwd / sandwich_bwd in bf16 and fp16, both variants, against the float64 reference with the bounds
    of the GPU test; every float64 reference value is finite on rows of the GPU test's kind (that test asserts it again for its own)."""
    x, a, w_out, w_next, dy, dres = _rows(dtype, N, d, 7 * d + N)
    for wn in (w_next, None):
        s, y, rstd_a, rstd_s = ref.sandwich_fwd(x, a, w_out, wn, EPS)
        s_exact, _, want_ra, _, _ = sandwich64(x, a, w_out, wn, EPS, dtype)
        b_ra, b_s = fwd_bounds(dtype, x, a, w_out, EPS, s_exact, want_ra)
        assert s.dtype == dtype and rstd_a.dtype == F32 and tuple(rstd_a.shape) == (N,)
        _within("rstd_a", rstd_a, want_ra, b_ra)
        _within("s", s, s_exact, b_s)
        if wn is None:
            assert y is None and rstd_s is None
            continue
        want_y, _, want_rs, _ = rmsnorm64(s, wn, EPS)       # of the stored s
        b_rs, b_y = norm_y_bounds(dtype, s, wn, EPS, want_y, want_rs)
        _within("rstd_s", rstd_s, want_rs, b_rs)
        _within("y", y, want_y, b_y)
        if N > 4:
            assert torch.equal(s[1], x[1]), "an all-zero a row leaves x as it is"
        dx, da, part = ref.sandwich_bwd(dy, s, wn, rstd_s, dres, a, w_out, rstd_a)
        assert tuple(part.shape) == (2, 1, d) and part.dtype == F32
        ds, _, want_da, g_next, g_out = sandwich_bwd64(dy, s, wn, rstd_s, dres, a, w_out, rstd_a, dtype, dx_stored=dx)
        _within("dx", dx, ds, rms_dx_bound(dtype, dy, s, wn, rstd_s, dres, ds))
        _within("da", da, want_da, rms_dx_bound(dtype, dx, a, w_out, rstd_a, None, want_da))
        xh, ah = s.double() * rstd_s.double()[:, None], a.double() * rstd_a.double()[:, None]
        for k, (want, mags) in enumerate(((g_next, (dy.double() * xh).abs().sum(0)),
                                          (g_out, (dx.double() * ah).abs().sum(0)))):
            # torch sums the N rows in some order: at most N roundings on a path, 2 in each term
            _within(f"part[{k}]", part[k, 0], want, MARGIN * (N + 2) * U * mags + 1e-30)


@pytest.mark.parametrize("N,d", [(1, 8), (7, 128), (33, 520)])
def test_reference_in_float64_against_autograd(N, d):
    """On float64 inputs nothing rounds, so the references equal torch autograd of the composition."""
    x, a, w_out, w_next, dy, dres = (t.double() for t in _rows(BF16, N, d, 3 * d + N))
    for wn in (w_next, None):
        s, y, rstd_a, rstd_s = ref.sandwich_fwd(x, a, w_out, wn, EPS)
        s_exact, _, want_ra, want_y, want_rs = sandwich64(x, a, w_out, wn, EPS, BF16)
        assert torch.allclose(s, s_exact, rtol=1e-12, atol=1e-12) and torch.allclose(rstd_a, want_ra, rtol=1e-12)
        if wn is None:
            dx, da, _, g_out = sandwich_autograd64(x, a, w_out, None, EPS, None, dres)
            got = ref.norm_bwd(dres, a, w_out, None, rstd_a, None, None, None, False, True)    # the FFN site's backward
            assert torch.equal(dx, dres) and torch.allclose(got, da, rtol=1e-10, atol=1e-12)
            continue
        y2 = s * rstd_s[:, None] * wn
        assert torch.allclose(y, y2, rtol=1e-12, atol=1e-12)
        dx, da, part = ref.sandwich_bwd(dy, s, wn, rstd_s, dres, a, w_out, rstd_a)
        wdx, wda, wgn, wgo = sandwich_autograd64(x, a, w_out, wn, EPS, dy, dres)
        assert torch.allclose(dx, wdx, rtol=1e-10, atol=1e-12) and torch.allclose(da, wda, rtol=1e-10, atol=1e-12)
        # the partials pass through fp32
        assert torch.allclose(part[0, 0].double(), wgn, rtol=1e-5, atol=1e-5)
        assert torch.allclose(part[1, 0].double(), wgo, rtol=1e-5, atol=1e-5)


def _gates(dtype, n, seed):
    """[n] gates: 3 randn, and first the extreme ones: 0, +-2^-20, +-8, +-2^14 and for bf16 +-2^100."""
    g = torch.Generator().manual_seed(seed)
    v = 3.0 * torch.randn(n, generator=g)
    sp = [0.0, 2.0 ** -20, -2.0 ** -20, 8.0, -8.0, 2.0 ** 14, -2.0 ** 14] + ([2.0 ** 100, -2.0 ** 100] if dtype == BF16 else [])
    v[:len(sp)] = torch.tensor(sp)
    up, dh = 2 * torch.rand(n, generator=g) - 1, 2 * torch.rand(n, generator=g) - 1
    return v.to(dtype), up.to(dtype), dh.to(dtype), len(sp)


@FORMATS
def test_geglu_reference_against_float64(dtype):
    gate, up, dh, nsp = _gates(dtype, 64, 5)
    gu = torch.cat([gate, up])[None]
    (wh, wdg, wdu), (bh, bdg, bdu) = geglu_bounds(dtype, gate, up, dh)
    h = ref.swiglu_fwd(gu, "geglu")[0]
    dgu = ref.swiglu_bwd(dh[None], gu, "geglu")[0]
    _within("h", h, wh, bh)
    _within("dgate", dgu[:64], wdg, bdg)
    _within("dup", dgu[64:], wdu, bdu)
    # saturated gates: gelu_tanh(g) = g or -0 and the derivative 1 or 0, exactly
    for i in range(5, nsp):
        pos = float(gate[i]) > 0
        assert float(h[i]) == (float(gate[i].float() * up[i].float()) if pos else 0.0)
        assert float(dgu[i]) == (float((dh[i].float() * up[i].float()).to(dtype)) if pos else 0.0)
    d2, h2 = ref.swiglu_bwd_h(dh[None], gu, "geglu")
    assert torch.equal(d2[0], dgu) and torch.equal(h2[0], h)
    # "silu", the config's "swiglu" and no argument are one function
    assert torch.equal(ref.swiglu_fwd(gu), ref.swiglu_fwd(gu, "silu")) and \
        torch.equal(ref.swiglu_fwd(gu), ref.swiglu_fwd(gu, "swiglu"))
    with pytest.raises(ValueError, match="activation must be one of"):
        ref.swiglu_fwd(gu, "relu")


def test_geglu_float64_reference_is_torch_gelu_tanh_and_its_autograd():
    g = torch.linspace(-12, 12, 4001, dtype=F64)
    g = torch.cat([g, torch.tensor([0.0, 2.0 ** -20, -2.0 ** -20, 2.0 ** 14, -2.0 ** 14, 2.0 ** 100, -2.0 ** 100], dtype=F64)])
    x = g.clone().requires_grad_()
    y = torch.nn.functional.gelu(x, approximate="tanh")
    y.sum().backward()
    assert bool(torch.isfinite(gelu_tanh64(g)).all()) and bool(torch.isfinite(gelu_tanh_grad64(g)).all())
    # torch's 0.5 x (1 + tanh) cancels for negative x: absolute 1e-16 |x| there
    assert float((gelu_tanh64(g) - y.detach()).abs().sub(1e-15 * g.abs()).max()) <= 1e-15
    fin = torch.isfinite(x.grad)          # torch's own derivative overflows to nan at 2^100
    assert int(fin.sum()) >= 4005
    assert float((gelu_tanh_grad64(g) - x.grad)[fin].abs().max()) <= 1e-12
    up, dh = torch.randn(g.numel(), dtype=F64), torch.randn(g.numel(), dtype=F64)
    gu = torch.cat([g, up])[None]
    assert torch.allclose(ref.swiglu_fwd(gu, "geglu")[0], geglu64(g, up), rtol=1e-12, atol=1e-15)
    wdg, wdu = geglu_grad64(dh, g, up)
    got = ref.swiglu_bwd(dh[None], gu, "geglu")[0]
    assert bool(torch.isfinite(got).all())
    assert torch.allclose(got[:g.numel()], wdg, rtol=1e-10, atol=1e-13)
    assert torch.allclose(got[g.numel():], wdu, rtol=1e-10, atol=1e-13)


# ------------------------------------------------------------------------------------------- whole model
def _perturbed(cfg, dtype=None):
    """A model whose out-norm weights are not all ones (so a swapped or missing weight shows)."""
    torch.manual_seed(0)
    m = build_model(cfg)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for layer in m.model.layers:
            if cfg.sandwich_norm:
                layer.self_attn.out_norm.weight.add_(0.3 * torch.randn(cfg.n_embd, generator=g))
                layer.mlp.out_norm.weight.add_(0.3 * torch.randn(cfg.n_embd, generator=g))
    return m if dtype is None else m.to(dtype)


@pytest.mark.parametrize("extra", [dict(), dict(n_experts=4), dict(n_experts=4, moe_dropless=True),
                                   dict(qk_norm=True, attn_softcap=50.0, final_softcap=30.0, sliding_window=8)],
                         ids=["dense", "moe", "moe_dropless", "gemma_block"])
@pytest.mark.parametrize("flags", FLAG_SETS, ids=FLAG_IDS)
def test_whole_model_against_the_oracle(flags, extra):
    """Loss and every gradient in float64 against models/oracle.py; comparison and tolerance of
    tests/test_qknorm_cpu.py's whole-model check (norm-weight slots pass through fp32)."""
    cfg = _cfg(**flags, **extra)
    m = _perturbed(cfg).double()
    o = OracleMistral(cfg).double()
    o.load_state_dict(m.state_dict())
    idx = torch.randint(0, cfg.vocab_size, (2, 32), generator=torch.Generator().manual_seed(2))
    tgt = idx.roll(-1, 1)
    l1, l2 = m(idx, tgt)[1], o(idx, tgt)[1]
    assert abs(l1.item() - l2.item()) <= 1e-12 * abs(l2.item())
    l1.backward()
    l2.backward()
    want = dict(o.named_parameters())
    assert sum("out_norm" in n for n in want) == (2 * cfg.n_layer if cfg.sandwich_norm else 0)
    for n, p in m.named_parameters():
        w = want[n].grad
        tol = 1e-7 if "norm" in n else 1e-11
        assert float(w.abs().max()) > 0 or "experts" in n, n
        assert float((p.grad - w).abs().max()) <= tol * max(1.0, float(w.abs().max())), n


@pytest.mark.parametrize("moe,dropless", [(None, False), (4, False), (4, True)], ids=["dense", "moe", "moe_dropless"])
def test_zero_out_norm_weights_make_the_layer_the_identity(moe, dropless):
    """Both out-norm weights zero: x1 = x + 0 and x2 = x1 + 0, so a layer returns its input and passes dres on, bit
    for bit."""
    from dltb.models.mistral import _LayerFn
    cfg = _cfg(sandwich_norm=True, ffn_act="geglu", n_experts=moe, moe_dropless=dropless)
    torch.manual_seed(0)
    m = build_model(cfg).to(BF16)
    m.rt = ParamRuntime()
    with torch.no_grad():
        for layer in m.model.layers:
            layer.self_attn.out_norm.weight.zero_()
            layer.mlp.out_norm.weight.zero_()
    m._cur_bt, m._cur_bounds = (2, 32), None
    x = torch.randn(64, cfg.n_embd, generator=torch.Generator().manual_seed(1)).to(BF16).requires_grad_()
    y = _LayerFn.apply(x, m, 0)
    assert torch.equal(y, x.detach())
    dres = torch.randn(64, cfg.n_embd, generator=torch.Generator().manual_seed(2)).to(BF16)
    y.backward(dres)
    assert torch.equal(x.grad, dres)


def _loss_and_grads(m, idx, mode):
    m = copy.deepcopy(m)
    m.rt = ParamRuntime()
    m.activation_recompute = mode
    loss = m(idx, idx.roll(-1, 1))[1]
    loss.backward()
    return loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("mode", ["selective", "full"])
@pytest.mark.parametrize("flags", FLAG_SETS, ids=FLAG_IDS)
def test_recompute_equals_off_bit_for_bit(flags, mode):
    cfg = _cfg(**flags)
    m = _perturbed(cfg)
    idx = torch.randint(0, cfg.vocab_size, (2, 32), generator=torch.Generator().manual_seed(4))
    l0, g0 = _loss_and_grads(m, idx, "off")
    l1, g1 = _loss_and_grads(m, idx, mode)
    assert torch.equal(l0, l1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_recompute_with_moe_is_still_refused():
    """Recomputation does not allow --moe-experts: the flags do not change that."""
    m = build_model(_cfg(sandwich_norm=True, ffn_act="geglu", n_experts=4))
    m.activation_recompute = "selective"
    idx = torch.randint(0, 256, (2, 32), generator=torch.Generator().manual_seed(4))
    with pytest.raises(ValueError, match="not supported together with --moe-experts"):
        m(idx, idx)


def test_flags_off_never_call_the_new_functions(monkeypatch):
    calls = {"n": 0, "acts": set()}

    def counted(fn):
        def f(*a, **k):
            calls["n"] += 1
            return fn(*a, **k)
        return f

    def act_seen(fn):
        def f(*a, **k):
            calls["acts"].add(a[-1] if isinstance(a[-1], str) else k.get("act", "silu"))
            return fn(*a, **k)
        return f

    for mod, name in ((F_, "sandwich_fwd"), (F_, "sandwich_bwd"), (ref, "sandwich_fwd"), (ref, "sandwich_bwd")):
        monkeypatch.setattr(mod, name, counted(getattr(mod, name)))
    for name in ("swiglu_fwd", "swiglu_bwd", "swiglu_bwd_h"):
        monkeypatch.setattr(ref, name, act_seen(getattr(ref, name)))
    idx = torch.randint(0, 256, (2, 32), generator=torch.Generator().manual_seed(6))
    for kw in (dict(), dict(n_experts=4), dict(n_experts=4, moe_dropless=True)):
        torch.manual_seed(0)
        m = build_model(_cfg(**kw))
        for mode in (("off",) if kw else ("off", "selective", "full")):
            m.activation_recompute = mode
            m(idx, idx)[1].backward()
    assert calls["n"] == 0 and calls["acts"] == {"swiglu"}
    for kw in (dict(), dict(n_experts=4), dict(n_experts=4, moe_dropless=True)):
        calls["n"], calls["acts"] = 0, set()
        torch.manual_seed(0)
        m = build_model(_cfg(sandwich_norm=True, ffn_act="geglu", **kw))
        m(idx, idx)[1].backward()
        # per layer two forward calls (attention site, FFN site) and one fused backward, in F_ and in ref
        assert calls["n"] == m.cfg.n_layer * 6 and calls["acts"] == {"geglu"}


# ------------------------------------------------------------------------------------------- engines, checkpoints
def _train(strategy, accum, flags, steps=3):
    cfg = _cfg(**flags)
    torch.manual_seed(0)
    m = build_model(cfg)
    ecfg = engine_config(strategy, accum, "reference", bucket_mb=0.05)
    ecfg.lr = 1e-3
    eng = make_engine(m, ecfg, "cpu")
    eng.train()
    g = torch.Generator().manual_seed(7)
    losses = []
    for _ in range(steps):
        b = torch.randint(0, 256, (2, 32), generator=g)
        micro = b.shape[0] // accum
        for k in range(accum):
            x = b[k * micro:(k + 1) * micro]
            loss = eng(x, x.roll(-1, 1))[1]
            eng.backward(loss)
            eng.step()
            losses.append(float(loss.detach()))
    return eng.full_state_dict(), losses, eng


@pytest.mark.parametrize("strategy", ["zero3", "fsdp"])
def test_the_four_engines_train_and_agree(strategy):
    """As tests/test_mistral_cpu.py: ZeRO-3 against ZeRO-2 (accumulating) and FSDP against DDP, both flags on."""
    flags = dict(sandwich_norm=True, ffn_act="geglu")
    accum = 2 if strategy == "zero3" else 1
    base, l0, _ = _train("zero2" if strategy == "zero3" else "ddp", accum, flags)
    got, l1, _ = _train(strategy, accum, flags)
    assert all(l == l for l in l0 + l1)
    names = [n for n in base if "out_norm" in n]
    assert len(names) == 4
    for n in base:
        assert torch.allclose(got[n].float(), base[n].float(), atol=1e-6), (strategy, n)
    for n in names:
        assert not bool((base[n].float() == 1).all()), f"{n} was not trained"


@pytest.mark.parametrize("case", ["cp_ddp", "cp_zero2"])
def test_world2_equals_world1_cpu(tmp_path, case):
    """Two gloo ranks against the one-rank run on the concatenated batch, mtiny with both flags (the comparison of
    tests/test_qknorm_cpu.py): the DDP and the ZeRO-2 update are the ones the global batch defines."""
    extra = ("--cases", case, "--sandwich-norm", "--ffn-act", "geglu", "--seq-len", "64", "--windows", "2")
    ws1 = run(tmp_path / "ws1.pt", 1, "cpu", extra=extra)
    ws2 = run(tmp_path / "ws2.pt", 2, "cpu", extra=extra)
    names = [n for n in ws1[case]["init"] if "out_norm" in n]
    assert len(names) == 4 and all(ws1[case]["init"][n].numel() == 128 for n in names)
    bad = compare(ws1, ws2, loss_tol=1e-4, upd_tol=1e-3, cos_min=0.99999, param_tol=1e-3)
    assert not bad, bad
    for n in names:         # compare() skips small updates: the new weights are checked here
        u1 = ws1[case]["final"][n] - ws1[case]["init"][n]
        u2 = ws2[case]["final"][n] - ws2[case]["init"][n]
        assert float(u1.norm()) > 0, n
        assert float((u1 - u2).norm()) <= 1e-3 * float(u1.norm()), n


def _harness_args(res, *more):
    return ["--strategy", "zero3", "--tier", "mtiny", "--seq-len", "32", "--steps", "2", "--warmup-steps", "1",
            "--per-device-batch", "2", "--grad-accum", "1", "--results-dir", str(res), "--device", "cpu",
            "--log-every", "0", *more]


def test_harness_refuses_tinygpt(tmp_path, capsys):
    from dltb.harness import main
    for flag, msg in ((("--sandwich-norm",), "--sandwich-norm needs a causal tier"),
                      (("--ffn-act", "geglu"), "--ffn-act geglu needs a causal tier")):
        args = _harness_args(tmp_path / "res", *flag)
        args[args.index("mtiny")] = "tiny"
        with pytest.raises(SystemExit) as e:
            main(args)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err
        assert not (tmp_path / "res").exists()


def test_harness_sidecar_checkpoint_resume_export(tmp_path, capsys):
    from dltb.harness import main
    from safetensors.torch import load_file
    os.environ.pop("WORLD_SIZE", None)
    res = tmp_path / "res"
    on = ("--sandwich-norm", "--ffn-act", "geglu")
    assert main(_harness_args(res, *on, "--save-dir", str(tmp_path / "ck"), "--export-model",
                              str(tmp_path / "m.safetensors"))) == 0
    assert "sandwich norms on" in capsys.readouterr().out
    ext = [f for f in os.listdir(res) if f.endswith(".extended.json")]
    side = json.loads((res / ext[0]).read_text())
    assert side["model"]["sandwich_norm"] is True and side["model"]["ffn_act"] == "geglu"
    plain = [f for f in os.listdir(res) if f.endswith(".json") and not f.endswith(".extended.json")]
    for f in plain:         # the reference-format record keeps its keys
        assert "sandwich_norm" not in json.loads((res / f).read_text())
    sd = load_file(str(tmp_path / "m.safetensors"))
    for i in range(2):
        for n in OUT:
            assert tuple(sd[f"model.layers.{i}.{n}"].shape) == (128,)
    assert main(_harness_args(tmp_path / "res2", *on, "--resume", str(tmp_path / "ck"))) == 0
    with pytest.raises(Exception):      # a checkpoint of the flag-on model does not load into the flag-off model
        main(_harness_args(tmp_path / "res3", "--resume", str(tmp_path / "ck")))
    assert main(_harness_args(tmp_path / "res4")) == 0
    ext = [f for f in os.listdir(tmp_path / "res4") if f.endswith(".extended.json")]
    side = json.loads((tmp_path / "res4" / ext[0]).read_text())
    assert side["model"]["sandwich_norm"] is False and side["model"]["ffn_act"] == "swiglu"


def test_state_dict_round_trip():
    cfg = _cfg(sandwich_norm=True, ffn_act="geglu")
    a = _perturbed(cfg)
    torch.manual_seed(5)
    b = build_model(cfg)
    b.load_state_dict(copy.deepcopy(a.state_dict()))
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p, q), n
    with pytest.raises(RuntimeError, match="out_norm"):
        build_model(_cfg()).load_state_dict(a.state_dict())
