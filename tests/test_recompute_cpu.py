"""Activation recomputation of the Mistral-shape tiers (``--activation-recompute``) without a GPU: the two new
ops' torch references against the ops they rebuild, the fp32 model under ``selective`` / ``full`` against ``off``
bit for bit (the CPU path is deterministic and a re-run forward uses the same kernels on the same inputs), the
context-parallel re-gather on gloo with lazy collectives, and the harness's flag, refusal and sidecar key."""
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

SAVED = ("x", "h1", "rstd1", "qkv", "o", "lse", "aux", "x1", "h2", "rstd2", "gu", "hh")
KEPT = {"off": set(SAVED) - {"aux"},                    # aux: the dropout mask (None: no dropout) or the gathered K | V
        "selective": {"x", "rstd1", "qkv", "o", "lse", "x1", "rstd2", "gu"},
        "full": {"x", "o", "lse"}}


# ------------------------------------------------------------------------------------------- reference ops
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ref_swiglu_bwd_h_is_fwd_and_bwd(dtype):
    g = torch.Generator().manual_seed(0)
    gu = (torch.randn(5, 48, generator=g) * 8).to(dtype)
    dh = torch.randn(5, 24, generator=g).to(dtype)
    for fn in (ref.swiglu_bwd_h, F_.swiglu_bwd_h):
        dgu, h = fn(dh, gu)
        assert torch.equal(h, ref.swiglu_fwd(gu))
        assert torch.equal(dgu, ref.swiglu_bwd(dh, gu))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rms", [True, False])
@pytest.mark.parametrize("res", [False, True])
def test_ref_norm_apply_is_norm_fwd_y(dtype, rms, res):
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(2, 7, 40, generator=g) * 3 + 1).to(dtype)
    r = torch.randn(2, 7, 40, generator=g).to(dtype) if res else None
    w = (1 + 0.1 * torch.randn(40, generator=g)).to(dtype)
    b = None if rms else (0.1 * torch.randn(40, generator=g)).to(dtype)
    s, y, mean, rstd = ref.norm_fwd(x, r, w, b, 1e-5, rms, 0.0, None, 0)
    src = s if res else x
    assert torch.equal(ref.norm_apply(src, w, b, mean, rstd, rms), y)
    assert torch.equal(F_.norm_apply(src, w, b, mean, rstd, rms), y)
    out = torch.empty(14, 2, 40, dtype=dtype)[:, 1]                      # a strided view
    got = F_.norm_apply(src.reshape(14, 40), w, b, mean, rstd, rms, y_out=out)
    assert got is out and torch.equal(out, y.reshape(14, 40))


# ------------------------------------------------------------------------------------------- model
def _cfg(masked, layers=2):
    cfg = get_model_config("mtiny", 256)
    cfg.n_layer = layers
    if masked:
        cfg.sliding_window = 96
        cfg.doc_eos_id = cfg.vocab_size - 1
        cfg.validate()
    return cfg


def _layer_ctxs(loss):
    """The autograd nodes of the layers' fused Functions behind ``loss``."""
    seen, stack, out = set(), [loss.grad_fn], []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if type(fn).__name__ == "_LayerFnBackward":
            out.append(fn)
        stack.extend(f for f, _ in fn.next_functions)
    return out


def _run_model(mode, masked):
    torch.manual_seed(0)
    cfg = _cfg(masked)
    model = build_model(cfg)
    model.rt = ParamRuntime()
    if mode is not None:
        model.activation_recompute = mode
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, cfg.vocab_size, (2, 256), generator=g)
    if masked:                                                            # a few documents per row
        idx[:, [40, 41, 130, 255]] = cfg.doc_eos_id
    _, loss = model(idx, idx.roll(-1, 1))
    kept = [{n for n, t in zip(SAVED, c.saved) if t is not None} for c in _layer_ctxs(loss)]
    loss.backward()
    return loss.detach(), {n: p.grad for n, p in model.named_parameters()}, kept


@pytest.fixture(scope="module")
def off_runs():
    """The ``off`` run of each masking variant, computed once and left unchanged."""
    return {masked: _run_model(None, masked) for masked in (False, True)}


def test_default_is_off_and_keeps_todays_tuple(off_runs):
    assert build_model(_cfg(False)).activation_recompute == "off"
    assert mistral.RECOMPUTE_MODES == ("off", "selective", "full")
    _, grads, kept = off_runs[False]
    assert kept == [KEPT["off"]] * 2
    assert all(g is not None for g in grads.values())


@pytest.mark.parametrize("masked", [False, True], ids=["causal", "window_doc"])
@pytest.mark.parametrize("mode", ["selective", "full"])
def test_model_recompute_equals_off(off_runs, mode, masked):
    l0, g0, _ = off_runs[masked]
    l1, g1, kept = _run_model(mode, masked)
    assert kept == [KEPT[mode]] * 2
    assert torch.equal(l0, l1)
    assert set(g0) == set(g1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_unknown_mode_is_refused():
    model = build_model(_cfg(False, 1))
    model.activation_recompute = "everything"
    idx = torch.zeros(1, 256, dtype=torch.int64)
    with pytest.raises(ValueError, match="activation_recompute"):
        model(idx, idx)


# ------------------------------------------------------------------------------------------- context parallel
def test_world2_cp2_full_equals_off_lazy_cpu(tmp_path):
    """``full`` drops the gathered K | V and gathers again in the backward.  Eager, with DLTB_COMM_LAZY=1 (an
    asynchronous collective runs only when its work is waited for): a backward that read K | V without waiting for
    the re-gather would train another model.  Same ranks, same rows, same kernels: the runs must agree exactly."""
    args = ("--seq-len", "512", "--windows", "2", "--cases", "cp_zero3,cp_zero2_doc", "--context-parallel", "2")
    lazy = {"DLTB_COMM_LAZY": "1"}
    off = run(tmp_path / "off.pt", 2, "cpu", extra=args, env_extra=lazy)
    full = run(tmp_path / "full.pt", 2, "cpu", extra=args + ("--activation-recompute", "full"), env_extra=lazy)
    assert set(off) == set(full) == {"cp_zero3", "cp_zero2_doc"}
    for case in off:
        assert off[case]["losses"] == full[case]["losses"], case
        assert off[case]["rank_losses"] == full[case]["rank_losses"], case
        for n, t in off[case]["final"].items():
            assert torch.equal(t, full[case]["final"][n]), (case, n)
            assert not torch.equal(t, off[case]["init"][n]) or t.numel() == 0, (case, n)   # it did train


# ------------------------------------------------------------------------------------------- harness
def _harness_args(tier, res, mode):
    return ["--strategy", "zero3", "--tier", tier, "--seq-len", "32", "--steps", "2", "--warmup-steps", "1",
            "--per-device-batch", "1", "--grad-accum", "1", "--results-dir", str(res), "--device", "cpu"] \
        + ([] if mode is None else ["--activation-recompute", mode])


def _sidecar(res):
    ext = [f for f in os.listdir(res) if f.endswith(".extended.json")]
    plain = [f for f in os.listdir(res) if f.endswith(".json") and not f.endswith(".extended.json")]
    return json.loads((res / plain[0]).read_text()), json.loads((res / ext[0]).read_text())


def test_harness_records_the_mode(tmp_path):
    from dltb.harness import main
    os.environ.pop("WORLD_SIZE", None)
    recs = {}
    for mode in (None, "selective", "full"):
        res = tmp_path / str(mode)
        assert main(_harness_args("mtiny", res, mode)) == 0
        rec, side = _sidecar(res)
        assert side["activation_recompute"] == (mode or "off")
        assert "activation_recompute" not in rec                       # the reference-format record is unchanged
        recs[mode] = rec
    assert recs[None]["mean_loss"] == recs["selective"]["mean_loss"] == recs["full"]["mean_loss"]


@pytest.mark.parametrize("tier", ["A", "tiny"])
def test_harness_refuses_recompute_on_noncausal_tier(tmp_path, capsys, tier):
    from dltb.harness import main
    with pytest.raises(SystemExit) as e:
        main(_harness_args(tier, tmp_path / "res", "selective"))
    assert e.value.code == 2                                           # argparse's argument error
    assert "--activation-recompute" in capsys.readouterr().err
    assert not (tmp_path / "res").exists()


def test_harness_off_is_accepted_on_every_tier(tmp_path):
    from dltb.harness import build_parser, check_activation_recompute
    a = build_parser().parse_args(_harness_args("tiny", tmp_path, None))
    assert a.activation_recompute == "off"
    check_activation_recompute("off", get_model_config("A", 64), "A")
    with pytest.raises(ValueError, match="causal tier"):
        check_activation_recompute("full", get_model_config("A", 64), "A")
