"""Final-logit soft-capping and the LM-head z-loss on the MI355X: the option-taking kernels of csrc/xent.hip (fused
forward + backward, ``xent_lse``, ``xent_bwd_lse_``; bf16 and fp16) against float64 autograd on the defining expression
``logsumexp(C tanh(z / C)) - c_t + B lse^2`` from the same 16-bit logits; both options 0 against the extension's plain
entry points; refused operands; and the Mistral-shape model under the options against the stock-op oracle, with the head
in row chunks, under HIP-graph replay, on two host-staged ranks, and the logits it returns.

Inputs: ``_logits`` of tests/test_head_chunk_gpu.py (``randn * 2``, one row of +-80, a target of -1 every 7th row,
targets 0 and V - 1), 70 rows.  Options (C, B): (30, 0) Gemma's cap; (2, 0) most logits on the curved part of tanh
and the +-80 row saturated exactly; (0, 0.1), (2, 0.1): at lse about 12 a coefficient of 0.1 changes dlogits by a
factor 3.4, where 1e-4 would change them by 0.25 %, below the 16-bit output rounding that the tolerance allows.
Tolerances, those tests/test_head_chunk_gpu.py applies to these kernels: loss and lse 1e-3 + 1e-3 rel, dlogits
1e-4 + 2e-2 rel.  The cap adds about C 2^-22 per capped logit (7e-6 at C = 30), far inside them.
"""
import copy
import functools
import math

import pytest
import torch

import dltb  # noqa: F401
from dltb.models import build_model, get_model_config
from dltb.models.config import ModelConfig
from dltb.models.oracle import OracleMistral
from dltb.ops import functional as F_
from dltb.ops._ext import ext
from dltb.parallel import GraphedStep, ParamRuntime, engine_config, make_engine
from multirank_util import compare, run
from test_head_chunk_cpu import _head_ctx
from test_head_chunk_gpu import _logits

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
FORMATS = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
OPTS = pytest.mark.parametrize("C,B", [(30.0, 0.0), (2.0, 0.0), (0.0, 0.1), (2.0, 0.1)],
                               ids=["cap30", "cap2", "z0.1", "cap2_z0.1"])
EPS16 = 2.0 ** -9
N = 70


def close(a, b, atol, rtol, what=""):
    """Every element of ``a`` finite and within ``atol + rtol |b|`` of the float64 ``b``; prints the worst ratio."""
    assert torch.isfinite(a).all(), f"{what}: non-finite values in the kernel output"
    err = (a.double() - b.double()).abs()
    tol = atol + rtol * b.double().abs()
    print(f"{what}: worst error/tolerance {float((err / tol).max()):.3f}")
    bad = (err > tol).double().mean().item()
    assert bad == 0.0, f"{what}: {bad * 100:.3f}% elements out of tolerance, max err {err.max().item():.4g}"


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert ext().arch() == "gfx950"


@functools.lru_cache(maxsize=None)
def case(rows, V, dtype, C, B):
    """(z, t, loss64, lse64, dz64) of one shape and option pair, computed once and only read by the tests that share
    it: float64 autograd on the defining expression, from the 16-bit z itself (independent of ops/ref.py's closed
    form); ignored rows are 0 in loss64 and dz64."""
    z, t = _logits(rows, V, dtype)
    z64 = z.double().requires_grad_()
    c = C * torch.tanh(z64 / C) if C else z64
    lse = torch.logsumexp(c, -1)
    ct = c.gather(-1, t.clamp(min=0)[:, None])[:, 0]
    loss = torch.where(t != -1, lse - ct + B * lse * lse, torch.zeros_like(lse))
    dz, = torch.autograd.grad(loss.sum(), z64)
    return z, t, loss.detach(), lse.detach(), dz


def guarded(z, fill=3.0):
    """z inside a buffer with one more row before and after it, as tests/test_head_chunk_gpu.py::test_xent_bwd_lse."""
    rows, V = z.shape
    guard = torch.full((rows + 2, V), fill, device=DEV, dtype=z.dtype)
    guard[1:rows + 1] = z
    return guard, guard[1:rows + 1]


def guards_intact(guard, fill=3.0):
    return bool((guard[0] == fill).all() and (guard[-1] == fill).all())


# ------------------------------------------------------------------------------------------- kernels
@FORMATS
@OPTS
@pytest.mark.parametrize("V", [8, 256, 4096, 32000, 131072])
def test_fused_kernel_against_float64(V, C, B, dtype):
    z, t, loss64, _, dz64 = case(N, V, dtype, C, B)
    guard, rows = guarded(z)
    loss = F_.xent_fwd_bwd_(rows, t, -1, softcap=C, z_coef=B)
    assert loss.dtype == torch.float32 and loss.shape == (N,)
    close(loss, loss64, 1e-3, 1e-3, "loss")
    close(rows, dz64, 1e-4, 2e-2, "dlogits")
    assert (loss[t == -1] == 0).all() and (rows[t == -1] == 0).all()      # ignored rows are exactly 0 in both
    assert torch.isfinite(loss[5]) and torch.isfinite(rows[5]).all()      # the +-80 row
    if C == 2.0:            # tanh(+-40) is exactly +-1 in the kernel's form, so 1 - t^2 and dz are exactly 0
        assert t[5] != -1 and (z[5].abs() == 80).all() and (rows[5] == 0).all()
    assert guards_intact(guard)                                           # nothing written outside the rows


@FORMATS
@OPTS
@pytest.mark.parametrize("V", [8, 256, 4096, 32000, 131072])
def test_xent_lse_with_options(V, C, B, dtype):
    z, t, _, lse64, _ = case(N, V, dtype, C, B)
    keep = z.clone()
    loss, lse = F_.xent_lse(z, t, -1, softcap=C, z_coef=B)
    assert loss.dtype == lse.dtype == torch.float32 and loss.shape == lse.shape == (N,)
    assert torch.equal(z, keep)                                           # the logits are only read
    fused = F_.xent_fwd_bwd_(keep.clone(), t, -1, softcap=C, z_coef=B)
    assert torch.equal(loss, fused)                                       # the fused kernel's loss rows, bit for bit
    assert (loss[t == -1] == 0).all()
    close(lse, lse64, 1e-3, 1e-3, "lse")
    lo = torch.full((100,), 7.0, device=DEV)
    ls = torch.full((100,), 7.0, device=DEV)
    F_.xent_lse(z, t, -1, loss_out=lo[16:86], lse_out=ls[16:86], softcap=C, z_coef=B)
    assert torch.equal(lo[16:86], loss) and torch.equal(ls[16:86], lse)
    for buf in (lo, ls):
        assert (buf[:16] == 7.0).all() and (buf[86:] == 7.0).all()


# the grid runs over 16-byte vectors: (70, 8) is 70 vectors in one workgroup; (70, 32000) rows of 4000 vectors that
# start anywhere inside a workgroup; (3, 131072) 192 workgroups; (2048, 256) 8 rows per workgroup
@FORMATS
@OPTS
@pytest.mark.parametrize("rows,V", [(70, 8), (70, 32000), (3, 131072), (2048, 256)])
def test_xent_bwd_lse_with_options(rows, V, C, B, dtype):
    z, t, _, _, dz64 = case(rows, V, dtype, C, B)
    _, lse = F_.xent_lse(z, t, -1, softcap=C, z_coef=B)
    guard, chunk = guarded(z)
    got = F_.xent_bwd_lse_(chunk, t, lse, -1, softcap=C, z_coef=B)
    assert got.data_ptr() == guard[1].data_ptr()
    close(got, dz64, 1e-4, 2e-2, "dlogits")
    assert (got[t == -1] == 0).all()                                      # ignored rows are exactly 0
    if C == 2.0 and rows > 5:
        assert (got[5] == 0).all()
    assert guards_intact(guard)


@FORMATS
@pytest.mark.parametrize("V", [256, 32000])
def test_both_options_zero_are_the_plain_entry_points(V, dtype):
    """``softcap = 0, z_coef = 0`` through ops/functional.py: the extension's existing entry points, called directly."""
    C_ = ext()
    z, t = _logits(N, V, dtype)
    a, b = z.clone(), z.clone()
    assert torch.equal(F_.xent_fwd_bwd_(a, t, -1, softcap=0.0, z_coef=0.0), C_.xent_fwd_bwd_(b, t, -1))
    assert torch.equal(a, b)
    l0, s0 = C_.xent_lse(z, t, -1)
    l1, s1 = F_.xent_lse(z, t, -1, softcap=0.0, z_coef=0.0)
    assert torch.equal(l0, l1) and torch.equal(s0, s1)
    a, b = z.clone(), z.clone()
    F_.xent_bwd_lse_(a, t, s0, -1, softcap=0.0, z_coef=0.0)
    C_.xent_bwd_lse_(b, t, s0, -1)
    assert torch.equal(a, b)


def test_flag_off_calls_no_option_kernel(monkeypatch):
    C_ = ext()
    seen = []
    for name in ("xent_fwd_bwd_opt_", "xent_lse_opt", "xent_bwd_lse_opt_"):
        real = getattr(C_, name)
        monkeypatch.setattr(C_, name, (lambda real, name: lambda *a, **kw: (seen.append(name), real(*a, **kw))[1])(
            real, name))
    z, t = _logits(N, 256, BF16)
    F_.xent_fwd_bwd_(z.clone(), t, -1)
    _, lse = F_.xent_lse(z, t, -1)
    F_.xent_bwd_lse_(z.clone(), t, lse, -1)
    assert seen == []
    F_.xent_fwd_bwd_(z.clone(), t, -1, softcap=30.0)
    _, lse = F_.xent_lse(z, t, -1, z_coef=0.1)
    F_.xent_bwd_lse_(z.clone(), t, lse, -1, z_coef=0.1)
    assert seen == ["xent_fwd_bwd_opt_", "xent_lse_opt", "xent_bwd_lse_opt_"]


def test_option_ops_refuse_bad_operands():
    C_ = ext()
    z, t = _logits(8, 64, BF16)
    _, lse = C_.xent_lse_opt(z, t, -1, 30.0, 0.1)
    for bad in (-1.0, float("nan"), float("inf")):
        for c, b in ((bad, 0.0), (0.0, bad)):
            with pytest.raises(RuntimeError, match="must be finite"):
                C_.xent_fwd_bwd_opt_(z.clone(), t, -1, c, b)
            with pytest.raises(RuntimeError, match="must be finite"):
                C_.xent_lse_opt(z, t, -1, c, b)
            with pytest.raises(RuntimeError, match="must be finite"):
                C_.xent_bwd_lse_opt_(z.clone(), t, lse, -1, c, b)
            for fn in (lambda: F_.xent_fwd_bwd_(z.clone(), t, -1, softcap=c, z_coef=b),
                       lambda: F_.xent_lse(z, t, -1, softcap=c, z_coef=b),
                       lambda: F_.xent_bwd_lse_(z.clone(), t, lse, -1, softcap=c, z_coef=b)):
                with pytest.raises(ValueError, match="must be a finite number"):
                    fn()
    # the shape and dtype cases the plain ops refuse
    with pytest.raises(RuntimeError):
        C_.xent_fwd_bwd_opt_(z[:, :56], t, -1, 30.0, 0.0)                 # not contiguous
    with pytest.raises(RuntimeError):
        C_.xent_fwd_bwd_opt_(z.clone(), t[:7], -1, 30.0, 0.0)
    with pytest.raises(RuntimeError):
        C_.xent_fwd_bwd_opt_(z.float(), t, -1, 30.0, 0.0)
    with pytest.raises(RuntimeError):
        C_.xent_fwd_bwd_opt_(torch.zeros(8, 12, device=DEV, dtype=BF16), t, -1, 30.0, 0.0)       # V % 8
    with pytest.raises(RuntimeError):
        C_.xent_lse_opt(z[:, :56], t, -1, 30.0, 0.0)
    with pytest.raises(RuntimeError):
        C_.xent_lse_opt(z, t[:7], -1, 30.0, 0.0)
    with pytest.raises(RuntimeError):
        C_.xent_lse_opt(z, t, -1, 30.0, 0.0, torch.empty(7, device=DEV))
    with pytest.raises(RuntimeError):
        C_.xent_lse_opt(torch.zeros(8, 12, device=DEV, dtype=BF16), t, -1, 30.0, 0.0)
    with pytest.raises(RuntimeError):
        C_.xent_bwd_lse_opt_(z.clone(), t, lse[:7], -1, 30.0, 0.0)
    with pytest.raises(RuntimeError):
        C_.xent_bwd_lse_opt_(z.clone(), t, lse.double(), -1, 30.0, 0.0)
    with pytest.raises(RuntimeError):
        C_.xent_bwd_lse_opt_(z.clone(), t.int(), lse, -1, 30.0, 0.0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- whole model
T_MODEL = 256
MODEL_OPTS = [(30.0, 0.0), (0.0, 0.1), (30.0, 0.1)]
MODEL_IDS = ["cap30", "z0.1", "cap30_z0.1"]


def _cfg(C=0.0, B=0.0, **kw):
    return ModelConfig(**dict(get_model_config("mtiny", T_MODEL).to_dict(), final_softcap=C, lm_z_loss_coef=B, **kw))


def _scaled_up(cfg, mul=20.0):
    """One initialisation with the head times ``mul``: at the initialisation's scale the logits (about N(0, 0.2^2))
    are far below a cap of 30, and a cap that bends nothing would check nothing."""
    torch.manual_seed(0)
    m = build_model(cfg)
    with torch.no_grad():
        m.lm_head.weight.mul_(mul)
    return m


def _batch(cfg, rows=2):
    idx = torch.randint(0, cfg.vocab_size, (rows, T_MODEL), generator=torch.Generator().manual_seed(3))
    tgt = idx.roll(-1, 1).clone()
    tgt[:, ::9] = -1
    return idx, tgt


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("C,B", MODEL_OPTS, ids=MODEL_IDS)
def test_model_one_step_against_oracle(C, B, dtype):
    """One mtiny step (2 layers, T = 256, V = 256) in bf16 and in fp16 (with a loss scale, as the engines seed it)
    against autograd through models/oracle.py in fp32 on the same initialisation: loss within 1e-2 relative, every
    gradient within 6e-2 in the relative 2-norm (tests/test_attn_softcap_gpu.py's model comparison).  The oracle
    without the options gives another loss, so the options are in the comparison."""
    cfg = _cfg(C, B)
    base = _scaled_up(cfg)
    idx, tgt = _batch(cfg)
    o = OracleMistral(cfg)
    o.load_state_dict(base.state_dict())
    _, lo = o(idx, tgt)
    lo.backward()
    m = copy.deepcopy(base).to(DEV, dtype)
    m.rt = ParamRuntime()
    _, loss = m(idx.to(DEV), tgt.to(DEV))
    scale = 1024.0 if dtype == F16 else 1.0
    loss.backward(torch.tensor(scale, device=DEV))
    print(f"C {C} B {B} {dtype}: loss oracle {lo.item():.6f} gpu {loss.item():.6f}")
    assert math.isfinite(loss.item())
    assert abs(lo.item() - loss.item()) < 1e-2 * abs(lo.item())
    got = dict(m.named_parameters())
    for n, p in o.named_parameters():
        assert torch.isfinite(got[n].grad).all(), n
        r = rel(got[n].grad.float() / scale, p.grad)
        assert r < 6e-2, (n, r)
    off = OracleMistral(_cfg())
    off.load_state_dict(base.state_dict())
    assert abs(off(idx, tgt)[1].item() - lo.item()) > 2e-2 * abs(lo.item())


class _Runs:
    """tests/test_head_chunk_gpu.py::_Runs under the options: one initialisation, every run from a copy of it, once."""

    def __init__(self):
        self.cache = {}

    def get(self, C, B, chunk):
        key = (C, B, chunk)
        if key in self.cache:
            return self.cache[key]
        cfg = _cfg(C, B)
        if "base" not in self.cache:
            self.cache["base"] = _scaled_up(cfg).to(DEV, BF16)
        m = copy.deepcopy(self.cache["base"])
        m.cfg = cfg
        m.rt = ParamRuntime()
        m.head_chunk = chunk
        idx, tgt = _batch(cfg)
        idx, tgt = idx.to(DEV), tgt.to(DEV)
        _, loss = m(idx, tgt)
        ctx = _head_ctx(loss)
        saved = [t.numel() for t in ctx.saved if torch.is_tensor(t)]
        x, h = ctx.saved[0].detach(), ctx.saved[1].detach().clone()
        loss.backward()
        torch.cuda.synchronize()
        self.cache[key] = dict(loss=loss.detach(), dW=m.lm_head.weight.grad, x=x, h=h, model=m, tgt=tgt.reshape(-1),
                               saved=saved, grads={n: p.grad for n, p in m.named_parameters()})
        return self.cache[key]


@pytest.fixture(scope="module")
def runs():
    return _Runs()


def _head64(r, bounds, C, B):
    """tests/test_head_chunk_gpu.py::_head64 with the options: the float64 loss of the head on the run's own input and
    the head's weight gradient summed over the rows before each boundary."""
    m = r["model"]
    x = r["x"].double()
    wn = m.model.norm.weight.detach().double()
    wh = m.lm_head.weight.detach().double().requires_grad_()
    h = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + m.cfg.norm_eps) * wn
    z = h @ wh.t()
    c = C * torch.tanh(z / C) if C else z
    lse = torch.logsumexp(c, -1)
    tg = r["tgt"]
    rows = torch.where(tg != -1, lse - c.gather(-1, tg.clamp(min=0)[:, None])[:, 0] + B * lse * lse,
                       torch.zeros_like(lse))
    count = (tg != -1).sum().clamp(min=1)
    partial = [torch.autograd.grad(rows[:r1].sum() / count, wh, retain_graph=True)[0] for r1 in bounds]
    return (rows.sum() / count).detach(), partial


@pytest.mark.parametrize("chunk", [128, 384])
@pytest.mark.parametrize("C,B", [(30.0, 0.1)], ids=["cap30_z0.1"])
def test_model_chunked_head_against_unchunked(runs, C, B, chunk):
    """mtiny in bf16 under both options, R = 512 rows in 4 chunks of 128 and a ragged 384 + 128, compared as
    tests/test_head_chunk_gpu.py::_check_against_unchunked compares the plain head: where the chunk product's rows
    carry the full product's bits the loss is the unchunked loss bit for bit (and ``xent_lse``'s rows are the fused
    kernel's); otherwise it is held to the float64 bound with bf16's 2^-9.  The head's weight gradient is held to
    that bound either way."""
    off, chk = runs.get(C, B, None), runs.get(C, B, chunk)
    R, V = 2 * T_MODEL, _cfg().vocab_size
    kw = dict(softcap=C, z_coef=B)
    assert off["saved"].count(R * V) == 1 and R * V not in chk["saved"]
    assert len(chk["saved"]) == len(runs.get(0.0, 0.0, chunk)["saved"])   # nothing more is kept under the options
    assert torch.equal(off["x"], chk["x"]) and torch.equal(off["h"], chk["h"])
    w = chk["model"].lm_head.weight.detach()
    full = F_.linear_fwd(chk["h"], w)
    tg = chk["tgt"]
    parts = [F_.linear_fwd(chk["h"][r0:r0 + chunk], w) for r0 in range(0, R, chunk)]
    rows_equal = torch.equal(torch.cat(parts), full)
    bounds = list(range(chunk, R, chunk)) + [R]
    loss64, partial = _head64(chk, bounds, C, B)
    e_u, e_c = (abs(r["loss"].double() - loss64).item() for r in (off, chk))
    print(f"R {R} chunk {chunk}: chunk product rows bit-equal to the full product's: {rows_equal}; "
          f"loss error vs float64 unchunked {e_u:.3e} chunked {e_c:.3e}")
    if rows_equal:
        mine = torch.cat([F_.xent_lse(p, tg[i * chunk:(i + 1) * chunk], -1, **kw)[0] for i, p in enumerate(parts)])
        assert torch.equal(mine, F_.xent_fwd_bwd_(full.clone(), tg, -1, **kw))
        assert torch.equal(chk["loss"], off["loss"])
    else:
        assert e_c <= e_u + EPS16 * abs(loss64.item())
    slack = (EPS16 * sum(p.abs() for p in partial)).max().item()
    e_u, e_c = ((r["dW"].double() - partial[-1]).abs().max().item() for r in (off, chk))
    print(f"R {R} chunk {chunk}: head dW max error vs float64 unchunked {e_u:.3e} chunked {e_c:.3e} "
          f"slack {slack:.3e}")
    assert e_c <= e_u + slack
    for n, g in chk["grads"].items():
        assert g is not None and torch.isfinite(g.float()).all(), n
    assert not torch.equal(chk["loss"], runs.get(0.0, 0.0, chunk)["loss"])          # the options reached the chunked head


def test_return_logits_are_the_capped_ones(runs):
    """``return_logits=True`` (and a call without targets) hands back C tanh(z / C) rounded to the model's format, z
    the raw product as the same weights give it without the cap; the loss is the run's without ``return_logits``."""
    C = 30.0
    m = copy.deepcopy(runs.get(C, 0.1, None)["model"])
    m.rt = ParamRuntime()
    cfg = m.cfg
    idx, tgt = _batch(cfg)
    idx, tgt = idx.to(DEV), tgt.to(DEV)
    raw_model = copy.deepcopy(m)
    raw_model.cfg = _cfg()
    raw, _ = raw_model(idx, tgt, return_logits=True)
    assert raw.dtype == BF16 and raw.float().abs().max() > 10.0          # the cap bends them
    want = C * torch.tanh(raw.double() / C)
    for chunk in (None, 128):
        m.head_chunk = chunk
        got, loss = m(idx, tgt, return_logits=True)
        assert got.dtype == BF16 and got.shape == raw.shape
        # one rounding to bf16 (8 significant bits: half a spacing is at most 2^-8 of the value) of a value formed
        # in fp32 (2^-22 beside it)
        assert ((got.double() - want).abs() <= (2.0 ** -8 + 2.0 ** -20) * want.abs()).all()
        assert (got.float().abs() <= C).all()
        assert torch.equal(loss.detach(), runs.get(C, 0.1, None)["loss"])
        only, none = m(idx)
        assert none is None and torch.equal(only, got)


# ------------------------------------------------------------------------------------------- graphs
def _train(graphed, accum=2, windows=2):
    torch.manual_seed(0)
    cfg = _cfg(30.0, 0.1)
    with torch.device(DEV):
        model = build_model(cfg)
    model.head_chunk = 128
    eng = make_engine(model, engine_config("zero3", accum, "reference"), "cuda:0")
    eng.train()
    g = torch.Generator(device=DEV).manual_seed(1)
    runner = GraphedStep(eng) if graphed else None
    losses = []
    for _ in range(accum * windows):
        idx = torch.randint(0, cfg.vocab_size, (2, T_MODEL), device=DEV, generator=g)
        if runner is None:
            loss = eng(idx, idx.roll(-1, 1))[1]
            eng.backward(loss)
            eng.step()
        else:
            loss = runner(idx, idx.roll(-1, 1))
        losses.append(loss.item())
    if runner is not None:
        assert len(runner.graphs) == eng.accum and not runner.disabled
    sd = {k: v.detach().clone() for k, v in eng.full_state_dict().items()}
    del eng, model, runner
    torch.cuda.empty_cache()
    return losses, sd


def test_graph_replay_equals_eager():
    """Two accumulation windows of two micro-steps under ZeRO-3, both options and a chunked head (512 rows in chunks
    of 128): the replayed graphs train the eager steps' model bit for bit."""
    l0, s0 = _train(False)
    l1, s1 = _train(True)
    assert all(l == l for l in l0) and l0 == l1, (l0, l1)
    # the z-term is in the reported loss: at the initialisation lse is about log(256), 0.1 lse^2 about 3
    assert l0[0] > math.log(256) + 0.5 * 0.1 * math.log(256) ** 2
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k


# ------------------------------------------------------------------------------------------- two ranks
def test_world2_host_staged_zero3_equals_world1(tmp_path):
    """Two ranks sharing the GPU (gloo, host-staged buffers) under ZeRO-3 against the one-rank run with the
    concatenated batch, the Mistral-shape case under both options; tests/test_multirank_gpu.py's tolerances.  Each
    rank forms the z-term on its own rows, as it forms its own mean loss."""
    args = ("--cases", "zero3_mistral", "--windows", "2", "--final-softcap", "30", "--lm-z-loss-coef", "0.1")
    ws1 = run(tmp_path / "ws1.pt", 1, "cuda", extra=args, timeout=300)
    ws2 = run(tmp_path / "ws2.pt", 2, "cuda", extra=args, env_extra={"DLTB_COMM": "host"}, timeout=300)
    assert set(ws1) == set(ws2) == {"zero3_mistral"}
    bad = compare(ws1, ws2, loss_tol=1e-3, upd_tol=0.02, cos_min=0.9998, param_tol=0.03)
    assert not bad, bad
    assert ws1["zero3_mistral"]["losses"][0] > math.log(256) + 0.5 * 0.1 * math.log(256) ** 2
