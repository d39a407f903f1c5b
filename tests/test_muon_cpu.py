"""Muon (``--optimizer muon``) without a GPU: the contract of ``ops/ref.py`` (``muon_momentum`` /
``muon_newton_schulz`` / ``muon_update``), which parameters are Muon matrices, where the engines refuse it, and
``FlatMuon`` on the CPU."""
import pytest
import torch

import dltb  # noqa: F401
from dltb.models import build_model, get_model_config
from dltb.ops import ref
from dltb.optim.muon import FlatMuon, muon_matrices
from dltb.parallel.strategy import engine_config, make_engine
from multirank_util import compare, report, run


@pytest.mark.parametrize("shape", [(64, 192), (128, 320)])
@pytest.mark.parametrize("rounded", [False, True])
def test_newton_schulz_singular_values(shape, rounded):
    """Five steps take a Gaussian matrix's singular values into [0.6, 1.2], exactly and with the bf16 rounding points
    (both in float64)."""
    g = torch.randn(shape, generator=torch.Generator().manual_seed(shape[1]), dtype=torch.float64)
    U, s = ref.muon_momentum(torch.zeros(shape, dtype=torch.float64), g, dtype=torch.float64, round=rounded)
    sv = torch.linalg.svdvals(ref.muon_newton_schulz(U, s, dtype=torch.float64, round=rounded))
    print(f"[muon] {shape} rounded={rounded}: singular values {float(sv.min()):.3f} .. {float(sv.max()):.3f}")
    assert 0.6 <= float(sv.min()) and float(sv.max()) <= 1.2


def _model(tier="mtiny", **over):
    cfg = get_model_config(tier, 32)
    for k, v in over.items():
        setattr(cfg, k, v)
    torch.manual_seed(0)
    return build_model(cfg)


def test_matrix_selection():
    got = [(n.split(".", 3)[3], s) for _, _, n, s in muon_matrices(_model()) if ".layers.0." in n]
    assert got == [("self_attn.qkv_proj.weight", (256, 128)), ("self_attn.o_proj.weight", (128, 128)),
                   ("mlp.gate_up_proj.weight", (512, 128)), ("mlp.down_proj.weight", (128, 256))]
    assert len(muon_matrices(_model())) == 8
    gpt = muon_matrices(_model("tiny"))           # d = 64: in_proj [192, 64], out_proj, c_fc [256, 64], c_proj
    assert len(gpt) == 8 and all(len(s) == 2 and s[0] % 64 == 0 and s[1] % 64 == 0 for _, _, _, s in gpt)
    moe = [n for _, _, n, _ in muon_matrices(_model(n_experts=4, moe_top_k=2))]
    assert len(moe) == 4 and not any("router" in n or "experts" in n for n in moe)


def _cfg(strategy, **kw):
    return engine_config(strategy, 1, "reference", optimizer="muon", **kw)


def test_refusals():
    with pytest.raises(ValueError, match="adamw or muon"):
        engine_config("ddp", optimizer="lion")
    for strategy in ("zero3", "fsdp"):
        with pytest.raises(ValueError, match="--optimizer muon is not supported"):
            make_engine(_model(), _cfg(strategy), "cpu")
    with pytest.raises(ValueError, match="loss scaling"):
        make_engine(_model(), _cfg("ddp", compute_dtype=torch.float16), "cpu")
    cfg = _cfg("zero3")
    cfg.extra["sub_group_elems"] = 4096
    with pytest.raises(ValueError, match="sub_group"):
        make_engine(_model(), cfg, "cpu")
    for strategy in ("ddp", "zero2"):             # world size 1: the rank owns whole matrices at every stage
        eng = make_engine(_model(), _cfg(strategy), "cpu")
        assert isinstance(eng.opt, FlatMuon) and len(eng.opt.matrices) == 8 and not eng._ddp_pipe_wanted()


def _engine_step():
    eng = make_engine(_model(), _cfg("ddp"), "cpu")
    eng.train()
    idx = torch.randint(0, 256, (2, 32), generator=torch.Generator().manual_seed(1))
    before = eng.opt.master.clone()
    eng.backward(eng(idx, idx)[1])
    grad = eng.flat_grad.clone()
    eng.step()
    return eng, before, grad


def test_cpu_step_is_the_reference_by_hand():
    eng, before, grad = _engine_step()
    opt, L = eng.opt, eng.layout
    want = before.clone()
    covered = torch.zeros_like(want, dtype=torch.bool)
    for u, i, name, (r, c) in muon_matrices(eng.model):
        s = L.slot(u, i)
        sl = slice(s.offset, s.offset + r * c)
        U, sc = ref.muon_momentum(torch.zeros(r, c), grad[sl].view(r, c), 0.95)
        ref.muon_update(want[sl].view(r, c), ref.muon_newton_schulz(U, sc), eng.cfg.lr, eng.cfg.weight_decay)
        covered[sl] = True
        assert float((want[sl] - before[sl]).abs().max()) > 0
    rest = ~covered
    m, ea, es = before.clone(), torch.zeros_like(before), torch.zeros_like(before)
    ref.adamw_flat(m, ea, es, grad, eng.cfg.lr, 0.9, 0.999, eng.cfg.eps, eng.cfg.weight_decay, 1)
    want[rest] = m[rest]
    assert torch.equal(opt.master, want)
    assert torch.equal(eng.flat_param, want)      # CPU compute dtype is fp32: the copy is the master
    assert sorted(n for n, _ in opt.matrices) == sorted(n for _, _, n, _ in muon_matrices(eng.model))
    assert opt.state_bytes == 3 * want.numel() * 4 + int(covered.sum()) * 4
    assert eng.memory_report()["optimizer_bytes"] == opt.state_bytes


def test_state_dict_round_trip():
    a, _, _ = _engine_step()
    sd = a.state_dict()
    assert sd["optimizer"]["optimizer"] == "muon" and float(sd["optimizer"]["muon_momentum"].abs().max()) > 0
    sd["optimizer"] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd["optimizer"].items()}
    b = make_engine(_model(), _cfg("ddp"), "cpu")
    b.train()
    b.load_state_dict(sd)
    assert torch.equal(b.opt.mom, a.opt.mom) and torch.equal(b.flat_param, a.flat_param)
    idx = torch.randint(0, 256, (2, 32), generator=torch.Generator().manual_seed(2))
    for e in (a, b):                              # the resumed run continues bit for bit
        e.backward(e(idx, idx)[1])
        e.step()
    assert torch.equal(a.opt.master, b.opt.master) and torch.equal(a.opt.mom, b.opt.mom)
    sd["optimizer"].pop("muon_momentum")
    with pytest.raises(ValueError, match="Muon momentum"):
        b.load_state_dict(sd)


MULTI = ("--cases", "cp_ddp", "--optimizer", "muon", "--lr", "0.005")


def test_ddp_world2_trains_the_world1_model(tmp_path):
    """DDP at world 2 (gloo) against world 1 on the same global batch.  The gradients of the two runs differ by fp32
    rounding only, but a bf16 rounding point of the chain may then fall the other way: each run's update is within the
    rounded chain's own deviation from the exact one (at most 1.4 %, the first two tests' chain), so the two are within
    3 % of each other, a cosine of 1 - 0.03^2 / 2, and the losses within 3 % of what the updates moved them.  That
    deviation holds for non-square matrices only: a square matrix has singular values near zero, where the chain is
    ill-conditioned (the reason the GPU whole-step test leaves them out too), so the square o_proj matrices are left
    out of the comparison of updates (they measured 3.5 % here); the losses are those of the whole model."""
    one, two = run(tmp_path / "w1.pt", 1, "cpu", extra=MULTI), run(tmp_path / "w2.pt", 2, "cpu", extra=MULTI)
    print("[muon] ddp world 2 vs world 1 (cpu), every parameter:", report(one, two))
    for r in (one["cp_ddp"], two["cp_ddp"]):
        for n in [n for n, t in r["init"].items() if t.dim() == 2 and t.shape[0] == t.shape[1]]:
            del r["init"][n], r["final"][n]
    ls = one["cp_ddp"]["losses"]
    assert ls[-1] < ls[0], ls
    bad = compare(one, two, loss_tol=0.03 * (max(ls) - min(ls)) / min(ls), upd_tol=0.03, cos_min=1 - 0.03 ** 2 / 2,
                  param_tol=0.03)
    assert not bad, bad


def test_sharded_owners_refuse_at_world2(tmp_path):
    with pytest.raises(AssertionError, match="--optimizer muon needs whole matrices in the rank"):
        run(tmp_path / "z2.pt", 2, "cpu", extra=("--cases", "cp_zero2", "--optimizer", "muon"))
