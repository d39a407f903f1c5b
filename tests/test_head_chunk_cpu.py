"""The chunked LM head of the Mistral-shape tiers (``--head-chunk N``) without a GPU: the torch references of the
two new ops against the fused one, the fp32 model with the head in row chunks against the unchunked head (both judged
against a float64 evaluation of the same head), what the head keeps for its backward, the refused values, the
harness's flag / refusals / sidecar keys, and two ranks on gloo with context parallelism and lazy collectives."""
import json
import os

import pytest
import torch

import dltb
from dltb.models import build_model, get_model_config
from dltb.models import mistral
from dltb.ops import functional as F_
from dltb.ops import ref
from dltb.parallel import ParamRuntime
from multirank_util import run

EPS32 = 2.0 ** -23


# ------------------------------------------------------------------------------------------- reference ops
def _xent_case(V, dtype, rows=37):
    g = torch.Generator().manual_seed(V)
    z = (torch.randn(rows, V, generator=g) * 4).to(dtype)
    z[3] = z[3] + 30.0                                      # rows far from 0
    z[4] = z[4] - 30.0
    t = torch.randint(0, V, (rows,), generator=g)
    t[0], t[1] = 0, V - 1                                   # the first and the last column
    t[::7] = -1                                             # ignored rows (row 0 among them)
    t[2] = 0
    return z, t


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [8, 256, 1000])
def test_ref_xent_lse_is_the_fused_loss(V, dtype):
    z, t = _xent_case(V, dtype)
    for fn in (ref.xent_lse, F_.xent_lse):
        keep = z.clone()
        loss, lse = fn(keep, t, -1)
        assert torch.equal(keep, z)                         # read only
        assert loss.dtype == lse.dtype == torch.float32
        assert torch.equal(loss, ref.xent_fwd_bwd_(z.clone(), t, -1))
        assert (loss[t == -1] == 0).all() and (loss[t != -1] > 0).all()
        want = torch.logsumexp(z.double(), -1)
        assert torch.allclose(lse.double(), want, rtol=1e-6, atol=1e-6)   # one fp32 logsumexp of |values| <= 50
    lo, ls = torch.full((37,), 9.0), torch.full((37,), 9.0)
    got = F_.xent_lse(z, t, -1, loss_out=lo, lse_out=ls)
    assert got[0] is lo and got[1] is ls and torch.equal(lo, loss) and torch.equal(ls, lse)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [8, 256, 1000])
def test_ref_xent_bwd_lse_is_the_fused_gradient(V, dtype):
    z, t = _xent_case(V, dtype)
    want = z.clone()
    ref.xent_fwd_bwd_(want, t, -1)
    _, lse = ref.xent_lse(z, t, -1)
    for fn in (ref.xent_bwd_lse_, F_.xent_bwd_lse_):
        got = z.clone()
        assert fn(got, t, lse, -1) is got
        assert (got[t == -1] == 0).all()
        # tests/test_ref_ops.py::test_xent_ref: allclose's defaults; a bf16 result is rounded once more (2^-8)
        tol = dict(rtol=1e-5, atol=1e-8) if dtype == torch.float32 else dict(rtol=2.0 ** -8, atol=1e-8)
        assert torch.allclose(got.float(), want.float(), **tol)
        v = t != -1
        assert torch.allclose(got[v].float().sum(-1), torch.zeros(int(v.sum())), atol=V * 2.0 ** -8)


# ------------------------------------------------------------------------------------------- model
R, T = 512, 256


def _cfg(layers=2):
    cfg = get_model_config("mtiny", T)
    cfg.n_layer = layers
    return cfg


def _head_ctx(loss):
    """The autograd node of the head's fused Function behind ``loss`` (tests/test_recompute_cpu.py::_layer_ctxs)."""
    seen, stack = set(), [loss.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if type(fn).__name__ == "_HeadFnBackward":
            return fn
        stack.extend(f for f, _ in fn.next_functions)
    raise AssertionError("no _HeadFnBackward behind the loss")


def _batch(cfg):
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, cfg.vocab_size, (2, T), generator=g)
    tgt = idx.roll(-1, 1).clone()
    tgt[:, ::9] = -1                                        # ignored rows in every chunk
    return idx, tgt


def _run_model(chunk):
    torch.manual_seed(0)
    cfg = _cfg()
    model = build_model(cfg)
    model.rt = ParamRuntime()
    assert model.head_chunk is None                         # the default
    model.head_chunk = chunk
    idx, tgt = _batch(cfg)
    _, loss = model(idx, tgt)
    ctx = _head_ctx(loss)
    saved = [t for t in ctx.saved if torch.is_tensor(t)]
    x = ctx.saved[0]
    got = {}
    x.register_hook(lambda g: got.__setitem__("x", g.detach().clone()))
    loss.backward()
    grads = {n: p.grad for n, p in model.named_parameters()}
    got["model.norm.weight"], got["lm_head.weight"] = grads["model.norm.weight"], grads["lm_head.weight"]
    return dict(loss=loss.detach(), grads=grads, head=got, saved_numel=[t.numel() for t in saved], x=x.detach(),
                model=model, tgt=tgt.reshape(-1))


def _head64(run_, bounds):
    """The head in float64 on the run's own input: the loss, and for every row boundary in ``bounds`` the gradient
    of the rows before it (the running sum a chunked backward holds after that chunk; the last is the gradient)."""
    m = run_["model"]
    x = run_["x"].double().requires_grad_()
    wn = m.model.norm.weight.detach().double().requires_grad_()
    wh = m.lm_head.weight.detach().double().requires_grad_()
    h = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + m.cfg.norm_eps) * wn
    rows = torch.nn.functional.cross_entropy(h @ wh.t(), run_["tgt"], ignore_index=-1, reduction="none")
    count = (run_["tgt"] != -1).sum().clamp(min=1)
    partial = []
    for r1 in bounds:
        g = torch.autograd.grad(rows[:r1].sum() / count, (x, wn, wh), retain_graph=True)
        partial.append(dict(zip(("x", "model.norm.weight", "lm_head.weight"), g)))
    return (rows.sum() / count).detach(), partial


@pytest.fixture(scope="module")
def unchunked():
    """The ``head_chunk = None`` run, computed once and left unchanged."""
    return _run_model(None)


def test_default_keeps_the_logits(unchunked):
    V = _cfg().vocab_size
    assert unchunked["saved_numel"].count(R * V) == 1       # dl, the overwritten logits
    assert mistral.head_chunks(R, None) == 1 and mistral.head_chunks(R, R) == 1 and mistral.head_chunks(R, 4 * R) == 1
    assert mistral.head_chunks(R, 128) == 4 and mistral.head_chunks(R, 384) == 2 and mistral.head_chunks(R, 511) == 2


@pytest.mark.parametrize("chunk", [128, 384, 512])
def test_model_chunked_head_against_float64(unchunked, chunk):
    """fp32 on the CPU.  The chunked head rounds differently in two places: dlogits are exp(z - lse) instead of the
    rescaled exp(z - max) / sum, and a gradient that sums over rows is rounded once more per accumulated chunk.  So
    its error against float64 may exceed the unchunked error by one fp32 rounding of every running sum."""
    V = _cfg().vocab_size
    run_ = _run_model(chunk)
    assert set(run_["grads"]) == set(unchunked["grads"]) and all(g is not None for g in run_["grads"].values())
    if chunk >= R:                                          # one chunk would hold every row: today's path, exactly
        assert run_["saved_numel"].count(R * V) == 1
        assert torch.equal(run_["loss"], unchunked["loss"])
        for n, g in unchunked["grads"].items():
            assert torch.equal(run_["grads"][n], g), n
        return
    assert R * V not in run_["saved_numel"]                 # no logits kept ...
    assert max(run_["saved_numel"]) == R * _cfg().n_embd    # ... nothing larger than x and h
    assert torch.equal(run_["x"], unchunked["x"])           # the layers do not know about the head's chunks
    bounds = list(range(chunk, R, chunk)) + [R]
    loss64, partial = _head64(run_, bounds)
    err_u, err_c = (abs(r["loss"].double() - loss64).item() for r in (unchunked, run_))
    print(f"chunk {chunk}: loss error vs float64 unchunked {err_u:.3e} chunked {err_c:.3e}")
    assert err_c <= err_u + EPS32 * abs(loss64.item())
    for n, g64 in partial[-1].items():
        slack = EPS32 * sum(p[n].abs() for p in partial)
        err_u = (unchunked["head"][n].double() - g64).abs().max().item()
        err_c = (run_["head"][n].double() - g64).abs().max().item()
        print(f"chunk {chunk}: {n} max error vs float64 unchunked {err_u:.3e} chunked {err_c:.3e} "
              f"slack {slack.max().item():.3e}")
        assert err_c <= err_u + slack.max().item(), n


# ------------------------------------------------------------------------------------------- value checks
@pytest.mark.parametrize("bad", [0, -16, 2.5, "128", True])
def test_bad_head_chunk_is_refused(bad):
    model = build_model(_cfg(1))
    model.head_chunk = bad
    idx = torch.zeros(1, T, dtype=torch.int64)
    with pytest.raises(ValueError, match="head_chunk"):
        model(idx, idx)


def test_return_logits_keeps_the_unchunked_path():
    cfg = _cfg(1)
    idx, tgt = _batch(cfg)
    outs = []
    for chunk in (None, 128):
        torch.manual_seed(0)
        model = build_model(cfg)
        model.head_chunk = chunk
        logits, loss = model(idx, tgt, return_logits=True)
        only, none = model(idx)                             # no targets: the caller wants the logits
        assert none is None and torch.equal(only, logits)
        outs.append((logits, loss.detach()))
    assert outs[0][0].shape == (2, T, cfg.vocab_size)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------- harness
def _harness_args(tier, res, chunk):
    return ["--strategy", "zero3", "--tier", tier, "--seq-len", "32", "--steps", "2", "--warmup-steps", "1",
            "--per-device-batch", "1", "--grad-accum", "1", "--results-dir", str(res), "--device", "cpu"] \
        + ([] if chunk is None else ["--head-chunk", str(chunk)])


def _sidecar(res):
    ext = [f for f in os.listdir(res) if f.endswith(".extended.json")]
    plain = [f for f in os.listdir(res) if f.endswith(".json") and not f.endswith(".extended.json")]
    return json.loads((res / plain[0]).read_text()), json.loads((res / ext[0]).read_text())


def test_harness_records_the_chunk(tmp_path, capsys):
    from dltb.harness import main
    os.environ.pop("WORLD_SIZE", None)
    recs = {}
    for chunk in (None, 16):
        res = tmp_path / str(chunk)
        assert main(_harness_args("mtiny", res, chunk)) == 0
        rec, side = _sidecar(res)
        assert side["head_chunk"] == chunk
        assert side["head_chunks"] == (2 if chunk else 1)
        assert "head_chunk" not in rec and "head_chunks" not in rec      # the reference-format record is unchanged
        recs[chunk] = rec
    assert "Head chunk: 16 rows, 2 chunk(s)" in capsys.readouterr().out
    assert abs(recs[16]["mean_loss"] - recs[None]["mean_loss"]) <= 1e-6 * abs(recs[None]["mean_loss"])


@pytest.mark.parametrize("tier", ["A", "tiny"])
def test_harness_refuses_head_chunk_on_noncausal_tier(tmp_path, capsys, tier):
    from dltb.harness import main
    with pytest.raises(SystemExit) as e:
        main(_harness_args(tier, tmp_path / "res", 16))
    assert e.value.code == 2                                           # argparse's argument error
    assert "--head-chunk" in capsys.readouterr().err
    assert not (tmp_path / "res").exists()


@pytest.mark.parametrize("chunk", [24, 0, -16])
def test_harness_refuses_a_chunk_that_is_no_positive_multiple_of_16(tmp_path, capsys, chunk):
    from dltb.harness import check_head_chunk, main
    with pytest.raises(SystemExit) as e:
        main(_harness_args("mtiny", tmp_path / "res", chunk))
    assert e.value.code == 2
    assert "multiple of 16" in capsys.readouterr().err
    assert not (tmp_path / "res").exists()
    check_head_chunk(None, get_model_config("A", 64), "A")             # off is accepted on every tier
    with pytest.raises(ValueError, match="causal tier"):
        check_head_chunk(16, get_model_config("A", 64), "A")


# ------------------------------------------------------------------------------------------- context parallel
def test_world2_cp2_chunked_head_lazy_cpu(tmp_path):
    """Two ranks on gloo, one context-parallel group, ZeRO-3, lazy collectives: each rank's head sees its 256 of
    the 512 tokens of a row and runs them in 4 chunks.  Every loss of the run, those after updates included, is
    held to the fp32 bound of the model test (no float64 run here, so against the unchunked loss, with one rounding
    for each of the two runs)."""
    args = ("--seq-len", "512", "--windows", "2", "--cases", "cp_zero3", "--context-parallel", "2")
    lazy = {"DLTB_COMM_LAZY": "1"}
    off = run(tmp_path / "off.pt", 2, "cpu", extra=args, env_extra=lazy)["cp_zero3"]
    chk = run(tmp_path / "chunk.pt", 2, "cpu", extra=args + ("--head-chunk", "64"), env_extra=lazy)["cp_zero3"]
    print("losses unchunked", off["losses"], "chunked", chk["losses"])
    assert len(off["losses"]) == len(chk["losses"]) == 4
    for a, b in zip(off["losses"], chk["losses"]):
        assert abs(a - b) <= 2 * EPS32 * abs(a), (off["losses"], chk["losses"])
    for n, t in chk["final"].items():
        assert torch.equal(off["init"][n], chk["init"][n]), n
        assert not torch.equal(t, chk["init"][n]) or t.numel() == 0, n          # it did train
