"""QK-norm fused with RoPE (``ModelConfig.qk_norm`` / ``--qk-norm``) on the CPU: configuration and flag, the
reference definitions ``ops/ref.py qknorm_rope_fwd`` / ``qknorm_rope_bwd_`` against float64 autograd of "RMSNorm per
head, then rotate-half RoPE" (tests/qknorm_ref.py), the whole model against a float64 autograd model written here,
the recompute modes, two engines on two ranks, and the flag-off path, which must not reach the new functions.
The GPU kernels: tests/test_qknorm_gpu.py.

Bounds of the kernel-reference comparison (item 2).  ``ref`` computes in fp32 what the float64 reference computes
exactly, then rounds once.  With U = 2^-24 one fp32 rounding and MARGIN = 2 the one allowance on the fp32 part (both
as in tests/test_rowwise_gpu.py; torch's CPU rsqrt / mean get no separate term: the allowance covers them):

    var = mean(x^2):  D squares and a sum of D positive terms in whatever order: at most (D + 1) U var, + eps: U
    rstd = rsqrt(.):  half of that relative error, plus U                      -> rho = ((D + 2) / 2 + 1) U
    y = x rstd w:     2 multiplies                                             -> |y| (rho + 2 U)
    o1 = y1 c - y2 s: a rounding per product and one for the difference, on the magnitudes added
                      Tm = |y1 c| + |y2 s|                                     -> Tm (rho + 4 U)
    output:           half_ulp(want) + MARGIN * Tm (rho + 4 U)

    backward, g = R(-theta) dy: 3 U Tg with Tg = |d1 c| + |d2 s|;  xh = x rstd: |xh| (rho + U);  gw = g w: 3 U Tg |w|
    + U |gw|;  m = mean(gw xh): per term the two factors' errors and the product's rounding, then D adds:
    dm = mean(3 U Tg |w xh|) + (rho + (D + 3) U) mean|gw xh|;  inner = gw - xh m: dgw + |xh| dm + |xh m| (rho + 2 U)
    + U (|gw| + |xh m|);  dx = rstd inner: rstd (that) + rstd (|gw| + |xh m|) (rho + U);  all times MARGIN, plus
    half_ulp(want).  The weight-gradient sums stay fp32 here: N heads terms g xh, each 3 U Tg |xh| + |g xh| (rho +
    2 U), summed in any order: + N heads U sum|g xh|.
"""
import copy
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

import dltb  # noqa: F401
from dltb.harness import build_parser, check_qk_norm
from dltb.models import build_model, get_model_config, mistral
from dltb.models.config import ModelConfig
from dltb.ops import functional as F_
from dltb.ops import ref
from dltb.parallel import ParamRuntime

from multirank_util import compare, run
from qknorm_ref import bwd_bounds, fwd_bound, qknorm_rope64, qknorm_rope_autograd64, qknorm_rope_bwd64
from rowwise_ref import half_ulp

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
FORMATS = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
U = 2.0 ** -24
MARGIN = 2.0
EPS = 1e-5


def _qk_cfg(T=32, **kw):
    return ModelConfig(**dict(get_model_config("mtiny", T).to_dict(), qk_norm=True, **kw))


# ------------------------------------------------------------------------------------------- 1. config and flag
DENSE = ["input_layernorm.weight", "self_attn.qkv_proj.weight", "self_attn.o_proj.weight",
         "post_attention_layernorm.weight", "mlp.gate_up_proj.weight", "mlp.down_proj.weight"]
QK = ["self_attn.q_norm.weight", "self_attn.k_norm.weight"]


def _moe_names(E):
    out = DENSE[:4] + ["mlp.router.weight"]
    for e in range(E):
        out += [f"mlp.experts.{e}.gate_up_proj.weight", f"mlp.experts.{e}.down_proj.weight"]
    return out


def test_tinygpt_config_refuses_qk_norm():
    with pytest.raises(ValueError, match="qk_norm"):
        ModelConfig(**dict(get_model_config("tiny", 32).to_dict(), qk_norm=True))
    cfg = get_model_config("tiny", 32)
    cfg.qk_norm = True
    with pytest.raises(ValueError, match="qk_norm"):
        cfg.validate()
    with pytest.raises(ValueError, match="qk_norm"):
        ModelConfig(**dict(get_model_config("mtiny", 32).to_dict(), qk_norm=1))
    with pytest.raises(ValueError, match="--qk-norm needs a causal tier"):
        check_qk_norm(True, get_model_config("tiny", 32), "tiny")


def test_flag_parses_and_sets_the_field():
    base = ["--strategy", "zero3", "--tier", "mtiny", "--seq-len", "32", "--steps", "1", "--per-device-batch", "1",
            "--grad-accum", "1", "--results-dir", "x"]
    assert build_parser().parse_args(base).qk_norm is False
    assert build_parser().parse_args(base + ["--qk-norm"]).qk_norm is True
    cfg = get_model_config("mtiny", 32)
    assert cfg.qk_norm is False
    check_qk_norm(False, cfg, "mtiny")
    assert cfg.qk_norm is False
    check_qk_norm(True, cfg, "mtiny")
    assert cfg.qk_norm is True
    old = {k: v for k, v in cfg.to_dict().items() if k != "qk_norm"}
    assert ModelConfig(**old).qk_norm is False


@pytest.mark.parametrize("on", [False, True], ids=["off", "on"])
@pytest.mark.parametrize("experts", [None, 4], ids=["dense", "moe"])
def test_num_params_and_param_list(on, experts):
    cfg = ModelConfig(**dict(get_model_config("mtiny", 32).to_dict(), qk_norm=on, n_experts=experts))
    model = build_model(cfg)
    assert cfg.num_params() == sum(p.numel() for p in model.parameters()) == model.num_params()
    plain = ModelConfig(**dict(cfg.to_dict(), qk_norm=False))
    assert cfg.num_params() - plain.num_params() == (cfg.n_layer * 2 * cfg.head_dim if on else 0)
    assert cfg.train_flops_per_token(32) == plain.train_flops_per_token(32)
    want = _moe_names(4) if experts else DENSE
    for i, layer in enumerate(model.model.layers):
        names = [n for n, _ in layer.param_list()]
        assert names == want + (QK if on else [])
        assert model.unit_blocks[i].names == [f"model.layers.{i}.{n}" for n in names]
        if on:
            for n, p in layer.param_list()[-2:]:
                assert tuple(p.shape) == (cfg.head_dim,) and bool((p == 1).all()), n
        else:
            assert not hasattr(layer.self_attn, "q_norm") and not hasattr(layer.self_attn, "k_norm")
    sd = model.state_dict()
    assert ("model.layers.0.self_attn.q_norm.weight" in sd) is on
    assert ("model.layers.1.self_attn.k_norm.weight" in sd) is on


# ------------------------------------------------------------------------------------------- 2. kernel references
def _inputs(dtype, N, Hq, Hkv, D, seed, special=True):
    g = torch.Generator().manual_seed(seed)
    heads = Hq + Hkv
    x = torch.randn(N, heads, D, generator=g)
    if special and N > 4:
        x[1, 0] = 0.0                                                   # an all-zero head row: rstd = 1 / sqrt(eps)
        x[2, heads - 1] = 0.0
        if dtype == F16:                                                # the squares reach 2^28: fp32 squares
            x[3, 0] = x[3, 0] * (2.0 ** 14 / float(x[3, 0].abs().max()))
            x[4, heads - 1] = x[4, heads - 1] * (2.0 ** 14 / float(x[4, heads - 1].abs().max()))
    v = torch.randn(N, Hkv * D, generator=g)
    wq = (1.0 + 0.5 * torch.randn(D, generator=g)).to(dtype)
    wk = (1.0 + 0.5 * torch.randn(D, generator=g)).to(dtype)
    dy = torch.randn(N, heads, D, generator=g).to(dtype)
    dv = torch.randn(N, Hkv * D, generator=g).to(dtype)
    return x.to(dtype), v.to(dtype), wq, wk, dy, dv


@FORMATS
@pytest.mark.parametrize("N,T", [(1, 1), (7 * 43, 43)])
@pytest.mark.parametrize("Hq,Hkv", [(2, 1), (8, 2)])
@pytest.mark.parametrize("D", [64, 128])
def test_reference_against_float64_autograd(dtype, D, Hq, Hkv, N, T):
    heads = Hq + Hkv
    x, v, wq, wk, dy, dv = _inputs(dtype, N, Hq, Hkv, D, 7 * D + Hq + N)
    cos, sin = ref.rope_tables(T, D, 10000.0)
    want_y, want_dx, want_dwq, want_dwk = qknorm_rope_autograd64(dy, x, wq, wk, cos, sin, T, Hq, EPS)
    # the hand-written float64 formulas are the autograd result
    y64, _ = qknorm_rope64(x, wq, wk, cos, sin, T, Hq, EPS)
    dx64, dwq64, dwk64 = qknorm_rope_bwd64(dy, x, wq, wk, cos, sin, T, Hq, EPS)
    for a, b in ((y64, want_y), (dx64, want_dx), (dwq64, want_dwq), (dwk64, want_dwk)):
        assert float((a - b).abs().max()) <= 1e-9 * max(1.0, float(b.abs().max()))
    # ---- forward
    qkv = torch.cat([x.reshape(N, heads * D), v], 1)
    before = qkv.clone()
    raw = ref.qknorm_rope_fwd(qkv, wq, wk, cos, sin, T, Hq, Hkv, D, EPS)
    assert raw.is_contiguous() and raw.dtype == dtype and tuple(raw.shape) == (N, heads * D)
    assert torch.equal(raw.view(torch.int16), before[:, :heads * D].contiguous().view(torch.int16)), "raw"
    assert torch.equal(qkv[:, heads * D:].contiguous().view(torch.int16),
                       before[:, heads * D:].contiguous().view(torch.int16)), "V columns touched"
    got = qkv[:, :heads * D].reshape(N, heads, D)
    assert bool(torch.isfinite(got).all())
    err = (got.double() - want_y).abs()
    bound = fwd_bound(dtype, x, wq, wk, cos, sin, T, Hq, EPS, want_y, D + 1)
    assert bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())
    if N > 4:
        assert bool((got[1, 0] == 0).all()) and bool((got[2, heads - 1] == 0).all())      # zero rows stay zero
    # ---- backward
    dqkv = torch.cat([dy.reshape(N, heads * D), dv], 1)
    dbefore = dqkv.clone()
    pq, pk = ref.qknorm_rope_bwd_(dqkv, raw, wq, wk, cos, sin, T, Hq, Hkv, D, EPS)
    assert torch.equal(dqkv[:, heads * D:].contiguous().view(torch.int16),
                       dbefore[:, heads * D:].contiguous().view(torch.int16)), "V columns of dqkv touched"
    gdx = dqkv[:, :heads * D].reshape(N, heads, D)
    assert bool(torch.isfinite(gdx).all())
    bdx, term, mags = bwd_bounds(dtype, dy, x, wq, wk, cos, sin, T, Hq, EPS, want_dx, D + 1, D)
    err = (gdx.double() - want_dx).abs()
    assert bool((err <= bdx).all()), float((err / bdx.clamp(min=1e-300)).max())
    assert pq.dtype == F32 and pk.dtype == F32 and pq.shape[-1] == D and pk.shape[-1] == D
    for part, want, sl in ((pq, want_dwq, slice(0, Hq)), (pk, want_dwk, slice(Hq, heads))):
        n_terms = N * (sl.stop - sl.start)
        b = term[:, sl].sum((0, 1)) + MARGIN * n_terms * U * mags[:, sl].sum((0, 1))
        err = (part.double().sum(0) - want).abs()
        assert bool((err <= b).all()), float((err / b.clamp(min=1e-300)).max())


# ------------------------------------------------------------------------------------------- 3. whole model
class _Model64(torch.nn.Module):
    """The dense Mistral-shape decoder with QK-norm in stock float64 ops, differentiated by autograd alone; reads
    the weights of a ``MistralLM`` by name."""

    def __init__(self, cfg, sd):
        super().__init__()
        self.cfg = cfg
        self.p = torch.nn.ParameterDict({k.replace(".", "/"): torch.nn.Parameter(v.double().clone())
                                         for k, v in sd.items()})

    def w(self, name):
        return self.p[name.replace(".", "/")]

    def rms(self, x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.cfg.norm_eps) * w

    def forward(self, idx, targets):
        cfg = self.cfg
        B, T = idx.shape
        H, Hkv, hd = cfg.n_head, cfg.kv_heads, cfg.head_dim
        cos, sin = ref.rope_tables(T, hd, cfg.rope_theta)
        cos, sin = cos.double()[None, None], sin.double()[None, None]

        def rope(t):
            t1, t2 = t[..., :hd // 2], t[..., hd // 2:]
            return torch.cat([t1 * cos - t2 * sin, t2 * cos + t1 * sin], -1)

        x = self.w("model.embed_tokens.weight")[idx]
        for i in range(cfg.n_layer):
            L = f"model.layers.{i}."
            h = self.rms(x, self.w(L + "input_layernorm.weight"))
            qkv = h @ self.w(L + "self_attn.qkv_proj.weight").t()
            q = qkv[..., :H * hd].view(B, T, H, hd).transpose(1, 2)
            k = qkv[..., H * hd:(H + Hkv) * hd].view(B, T, Hkv, hd).transpose(1, 2)
            v = qkv[..., (H + Hkv) * hd:].view(B, T, Hkv, hd).transpose(1, 2)
            q = rope(self.rms(q, self.w(L + "self_attn.q_norm.weight")))
            k = rope(self.rms(k, self.w(L + "self_attn.k_norm.weight")))
            k, v = k.repeat_interleave(H // Hkv, 1), v.repeat_interleave(H // Hkv, 1)
            att = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
            mask = torch.ones(T, T, dtype=torch.bool).tril()
            att = torch.softmax(att.masked_fill(~mask, float("-inf")), -1)
            o = (att @ v).transpose(1, 2).reshape(B, T, H * hd)
            x = x + o @ self.w(L + "self_attn.o_proj.weight").t()
            gu = self.rms(x, self.w(L + "post_attention_layernorm.weight")) @ self.w(L + "mlp.gate_up_proj.weight").t()
            g, u = gu.chunk(2, -1)
            x = x + (F.silu(g) * u) @ self.w(L + "mlp.down_proj.weight").t()
        logits = self.rms(x, self.w("model.norm.weight")) @ self.w("lm_head.weight").t()
        return F.cross_entropy(logits.view(-1, logits.size(-1)), targets.reshape(-1))


def _perturbed_model(cfg, dtype=None):
    """A model whose QK-norm weights are not all ones (so a swapped or missing weight shows)."""
    torch.manual_seed(0)
    m = build_model(cfg)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for layer in m.model.layers:
            layer.self_attn.q_norm.weight.add_(0.3 * torch.randn(cfg.head_dim, generator=g))
            layer.self_attn.k_norm.weight.add_(0.3 * torch.randn(cfg.head_dim, generator=g))
    return m if dtype is None else m.to(dtype)


def test_whole_model_against_float64_autograd():
    cfg = _qk_cfg(32)
    m = _perturbed_model(cfg).double()
    o = _Model64(cfg, m.state_dict())
    g = torch.Generator().manual_seed(2)
    idx = torch.randint(0, cfg.vocab_size, (2, 32), generator=g)
    tgt = idx.roll(-1, 1)
    l1 = m(idx, tgt)[1]
    l2 = o(idx, tgt)
    assert abs(l1.item() - l2.item()) <= 1e-12 * abs(l2.item())
    l1.backward()
    l2.backward()
    names = [n for n, _ in m.named_parameters()]
    assert sum("q_norm" in n or "k_norm" in n for n in names) == 2 * cfg.n_layer
    for n, p in m.named_parameters():
        want = o.w(n).grad
        # norm-weight slots pass through fp32 (ref._write_slot), the QK-norm pair included
        tol = 1e-7 if "norm" in n else 1e-11
        assert float(want.abs().max()) > 0, n
        assert float((p.grad - want).abs().max()) <= tol * max(1.0, float(want.abs().max())), n


# ------------------------------------------------------------------------------------------- 4. recompute
def _loss_and_grads(m, idx, mode):
    m = copy.deepcopy(m)
    m.rt = ParamRuntime()
    m.activation_recompute = mode
    loss = m(idx, idx.roll(-1, 1))[1]
    loss.backward()
    return loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("mode", ["selective", "full"])
def test_recompute_equals_off_bit_for_bit(mode):
    cfg = _qk_cfg(32)
    m = _perturbed_model(cfg)
    idx = torch.randint(0, cfg.vocab_size, (2, 32), generator=torch.Generator().manual_seed(4))
    l0, g0 = _loss_and_grads(m, idx, "off")
    l1, g1 = _loss_and_grads(m, idx, mode)
    assert torch.equal(l0, l1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


# ------------------------------------------------------------------------------------------- 5. engines
@pytest.mark.parametrize("case", ["ddp", "zero3", "zero3_cp2"])
def test_world2_equals_world1_cpu(tmp_path, case):
    """Two gloo ranks against the one-rank run on the concatenated batch, mtiny with QK-norm: the [64]-element
    parameters go through the flat layout (ddp) and through sharding with release + re-gather (zero3).  zero3_cp2:
    the two ranks are one context-parallel group, so each runs the fused calls per zigzag range with that range's
    cos / sin rows, and both ranges' partials meet in one gradient slot."""
    spec = {"ddp": "cp_ddp", "zero3": "zero3_mistral", "zero3_cp2": "cp_zero3"}[case]          # all the mtiny shape
    # the zigzag layout over two ranks needs a multiple of 512 positions
    extra = ("--cases", spec, "--qk-norm", "--seq-len", "512" if case == "zero3_cp2" else "64", "--windows", "2")
    ws1 = run(tmp_path / "ws1.pt", 1, "cpu", extra=extra)
    ws2 = run(tmp_path / "ws2.pt", 2, "cpu", extra=extra + (("--context-parallel", "2") if case == "zero3_cp2" else ()))
    names = [n for n in ws1[spec]["init"] if "q_norm" in n or "k_norm" in n]
    assert len(names) == 4 and all(ws1[spec]["init"][n].numel() == 64 for n in names)
    bad = compare(ws1, ws2, loss_tol=1e-4, upd_tol=1e-3, cos_min=0.99999, param_tol=1e-3)
    assert not bad, bad
    for n in names:         # compare() skips small updates: the new weights are checked here
        u1 = ws1[spec]["final"][n] - ws1[spec]["init"][n]
        u2 = ws2[spec]["final"][n] - ws2[spec]["init"][n]
        assert float(u1.norm()) > 0, n
        assert float((u1 - u2).norm()) <= 1e-3 * float(u1.norm()), n


# ------------------------------------------------------------------------------------------- 6. flag off
def test_flag_off_never_calls_the_new_functions(monkeypatch):
    calls = {"n": 0}

    def counted(fn):
        def f(*a, **k):
            calls["n"] += 1
            return fn(*a, **k)
        return f

    for mod, name in ((F_, "qknorm_rope_fwd"), (F_, "qknorm_rope_bwd_"), (F_, "qknorm_partials"),
                      (F_, "reduce_partials"), (ref, "qknorm_rope_fwd"), (ref, "qknorm_rope_bwd_")):
        monkeypatch.setattr(mod, name, counted(getattr(mod, name)))
    idx = torch.randint(0, 256, (2, 32), generator=torch.Generator().manual_seed(6))
    for kw in (dict(), dict(n_experts=4), dict(n_experts=4, moe_dropless=True)):
        cfg = ModelConfig(**dict(get_model_config("mtiny", 32).to_dict(), **kw))
        torch.manual_seed(0)
        m = build_model(cfg)
        for mode in (("off",) if kw else ("off", "selective", "full")):
            m.activation_recompute = mode
            m(idx, idx)[1].backward()
    assert calls["n"] == 0
    torch.manual_seed(0)
    m = build_model(_qk_cfg(32))
    m(idx, idx)[1].backward()
    # the flag on does reach them: per layer one forward, one backward and two reductions, in F_ and (fwd, bwd) in ref
    assert calls["n"] == cfg.n_layer * (4 + 2)


# ------------------------------------------------------------------------------------------- harness
def _harness_args(res, *more):
    return ["--strategy", "zero3", "--tier", "mtiny", "--seq-len", "32", "--steps", "2", "--warmup-steps", "1",
            "--per-device-batch", "2", "--grad-accum", "1", "--results-dir", str(res), "--device", "cpu",
            "--log-every", "0", *more]


def test_harness_refuses_tinygpt(tmp_path, capsys):
    from dltb.harness import main
    args = _harness_args(tmp_path / "res", "--qk-norm")
    args[args.index("mtiny")] = "tiny"
    with pytest.raises(SystemExit) as e:
        main(args)
    assert e.value.code == 2
    assert "--qk-norm needs a causal tier" in capsys.readouterr().err
    assert not (tmp_path / "res").exists()


def test_harness_sidecar_checkpoint_resume_export(tmp_path, capsys):
    from dltb.harness import main
    from safetensors.torch import load_file
    os.environ.pop("WORLD_SIZE", None)
    res = tmp_path / "res"
    assert main(_harness_args(res, "--qk-norm", "--save-dir", str(tmp_path / "ck"), "--export-model",
                              str(tmp_path / "m.safetensors"))) == 0
    assert "QK-norm: RMSNorm over head_dim 64" in capsys.readouterr().out
    ext = [f for f in os.listdir(res) if f.endswith(".extended.json")]
    side = json.loads((res / ext[0]).read_text())
    assert side["model"]["qk_norm"] is True
    sd = load_file(str(tmp_path / "m.safetensors"))
    for i in range(2):
        for n in QK:
            assert tuple(sd[f"model.layers.{i}.{n}"].shape) == (64,)
    assert main(_harness_args(tmp_path / "res2", "--qk-norm", "--resume", str(tmp_path / "ck"))) == 0
    # a checkpoint of the flag-on model does not load into the flag-off model
    with pytest.raises(Exception):
        main(_harness_args(tmp_path / "res3", "--resume", str(tmp_path / "ck")))
    assert main(_harness_args(tmp_path / "res4")) == 0
    ext = [f for f in os.listdir(tmp_path / "res4") if f.endswith(".extended.json")]
    assert json.loads((tmp_path / "res4" / ext[0]).read_text())["model"]["qk_norm"] is False
