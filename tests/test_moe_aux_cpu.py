"""The auxiliary router losses of the mixture-of-experts FFN (``moe_aux_loss_coef`` / ``moe_z_loss_coef``,
``--moe-aux-loss-coef`` / ``--moe-z-loss-coef``): the formulas of ops/ref.py against autograd in float64, their known
values, the model against the plain-torch oracle, the bit-for-bit defaults, validation and the harness record.
The GPU kernels: tests/test_moe_aux_gpu.py."""
import json
import math
import os
import socket
import subprocess
import sys

import pytest
import torch

import dltb
from dltb.models import build_model, get_model_config
from dltb.models import mistral
from dltb.models.config import ModelConfig
from dltb.models.oracle import OracleMistral
from dltb.ops import functional as F_
from dltb.ops import ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B = 0.01, 0.001


# ------------------------------------------------------------------------------------------- the formula
@pytest.mark.parametrize("N,E,K", [(37, 5, 2), (64, 64, 4)])
def test_backward_formula_against_autograd_float64(N, E, K):
    gen = torch.Generator().manual_seed(N + E)
    logits = (2.0 * torch.randn(N, E, generator=gen, dtype=torch.float64)).requires_grad_(True)
    w = torch.rand(E, generator=gen) + 0.05
    w[1] = 0.0                                               # an expert nobody chose
    counts = torch.bincount(torch.multinomial(w, N * K, replacement=True, generator=gen), minlength=E).to(torch.int32)
    assert int(counts.sum()) == N * K and int(counts[1]) == 0
    f = counts.double() / (N * K)                            # a constant
    p = torch.softmax(logits, -1)
    balance = E * (f * p.mean(0)).sum()
    lse = torch.logsumexp(logits, -1)
    z = lse.pow(2).mean()
    g = torch.tensor([0.7, -1.3], dtype=torch.float64)
    (g[0] * balance + g[1] * z).backward()
    r_lse, r_out = ref.moe_aux_fwd(logits.detach(), counts, K)
    assert float((r_lse - lse.detach()).abs().max()) <= 1e-12 * float(lse.detach().abs().max())
    assert abs(r_out[0].item() - balance.item()) <= 1e-12 * abs(balance.item())
    assert abs(r_out[1].item() - z.item()) <= 1e-12 * abs(z.item())
    got = ref.moe_aux_bwd_(torch.zeros(N, E, dtype=torch.float64), logits.detach(), r_lse, counts, g, K)
    assert float(logits.grad.abs().max()) > 0
    assert float((got - logits.grad).abs().max()) <= 1e-12 * float(logits.grad.abs().max())
    # in place, on top of what is there
    base = torch.randn(N, E, generator=gen, dtype=torch.float64)
    acc = base.clone()
    assert ref.moe_aux_bwd_(acc, logits.detach(), r_lse, counts, g, K) is acc
    assert torch.equal(acc, base + got)
    # the dispatcher takes the same path on the CPU and fills the record row
    row = torch.zeros(2)
    f_lse, f_out = F_.moe_aux_fwd(logits.detach(), counts, K, row)
    assert torch.equal(f_lse, r_lse) and torch.equal(f_out, r_out) and torch.equal(row, r_out.float())


@pytest.mark.parametrize("E,K", [(2, 1), (8, 2), (64, 4)])
def test_uniform_and_collapsed_router(E, K):
    N = 4 * E
    counts = torch.full((E,), N * K // E, dtype=torch.int32)
    lse, out = ref.moe_aux_fwd(torch.full((N, E), 0.375, dtype=torch.float64), counts, K)
    assert abs(out[0].item() - 1.0) <= 1e-12
    assert abs(out[1].item() - (0.375 + math.log(E)) ** 2) <= 1e-12 * (0.375 + math.log(E)) ** 2
    lse, out = ref.moe_aux_fwd(torch.zeros(N, E, dtype=torch.float64), counts, K)
    assert abs(out[0].item() - 1.0) <= 1e-12 and abs(out[1].item() - math.log(E) ** 2) <= 1e-12
    # everything on expert 2 (or the last), saturated probabilities
    e = min(2, E - 1)
    logits = torch.zeros(N, E, dtype=torch.float64)
    logits[:, e] = 40.0
    counts = torch.zeros(E, dtype=torch.int32)
    counts[e] = N * K
    lse, out = ref.moe_aux_fwd(logits, counts, K)
    assert abs(out[0].item() - E) <= 1e-6 and out[0].item() <= E
    assert abs(out[1].item() - 1600.0) <= 1e-6


@pytest.mark.parametrize("N,E", [(1, 2), (63, 64), (200, 5), (200, 8), (1030, 7), (4100, 64)])
def test_fp32_reference_is_inside_the_gpu_tests_forward_bound(N, E):
    """The fp32 CPU path on the inputs of tests/test_moe_aux_gpu.py, against float64 under the bound the kernel is held
    to there: the bound is not one that only wider-than-fp32 arithmetic could meet."""
    import test_moe_aux_gpu as gpu
    for shift in (0.0, 80.0, -80.0):
        logits, counts, K = gpu._inputs(N, E, shift)
        lse, out = ref.moe_aux_fwd(logits, counts, K)
        gpu.check_fwd(lse, out, logits, counts, K, f"ref fp32 N={N} E={E} shift={shift}")
        g = torch.tensor([0.7, -1.3])
        got = ref.moe_aux_bwd_(torch.zeros(N, E), logits, lse, counts, g, K)
        want, b = gpu.term64(logits, lse, counts, g, K)
        worst = ((got.double() - want).abs() / b.clamp(min=1e-300)).max().item()
        print(f"ref fp32 aux_bwd N={N} E={E} shift={shift}: max err / bound = {worst:.3f}")
        assert worst <= 1.0


# ------------------------------------------------------------------------------------------- model against the oracle
def _pair(K, a, b):
    cfg = get_model_config("mtiny", 32)
    cfg.n_experts, cfg.moe_top_k, cfg.moe_capacity_factor = 4, K, 1.0
    cfg.moe_aux_loss_coef, cfg.moe_z_loss_coef = a, b
    cfg.validate()
    torch.manual_seed(0)
    m = build_model(cfg).double()
    o = OracleMistral(cfg).double()
    o.load_state_dict(m.state_dict())
    idx = torch.randint(0, cfg.vocab_size, (2, 32))
    return cfg, m, o, idx


@pytest.mark.parametrize("K", [2, 1])
def test_model_against_oracle_float64(K):
    cfg, m, o, idx = _pair(K, A, B)
    l1, l2 = m(idx, idx)[1], o(idx, idx)[1]
    assert abs(l1.item() - l2.item()) <= 1e-12 * abs(l2.item())
    l1.backward()
    l2.backward()
    counts = m.moe_counts("cpu")
    assert int((counts - ref.moe_capacity(64, 4, K, 1.0)).clamp(min=0).sum()) > 0      # the run does drop
    for (n, p), (n2, p2) in zip(m.named_parameters(), o.named_parameters()):
        assert n == n2
        tol = 1e-8 if "layernorm" in n or n == "model.norm.weight" else 1e-12      # norm slots pass through fp32
        assert float((p.grad - p2.grad).abs().max()) <= tol * max(1.0, float(p2.grad.abs().max())), n
    # the loss does hold the two terms: the record rows, weighted, are the difference to the LM loss
    cfg0, m0, _, _ = _pair(K, 0.0, 0.0)
    lm = m0(idx, idx)[1].item()
    aux = m.moe_aux("cpu").double()
    assert aux.shape == (cfg.n_layer, 2) and (aux[:, 0] >= 1.0 - 1e-6).all() and (aux[:, 1] > 0).all()
    assert abs(l1.item() - (lm + A * aux[:, 0].sum().item() + B * aux[:, 1].sum().item())) <= 1e-6 * lm
    if K == 1:
        # top-1: the only gate is 1, so the router trains through the auxiliary terms alone
        m0.zero_grad()
        m0(idx, idx)[1].backward()
        for i in range(cfg.n_layer):
            assert float(m0.model.layers[i].mlp.router.weight.grad.abs().max()) == 0.0
            assert float(m.model.layers[i].mlp.router.weight.grad.abs().max()) > 0.0


def test_each_coefficient_alone_against_the_oracle():
    _, m0, _, idx0 = _pair(2, 0.0, 0.0)
    lm = m0(idx0, idx0)[1]
    lm.backward()
    g0 = m0.model.layers[0].mlp.router.weight.grad
    # the unweighted per-layer terms, from a run with both on (the routing does not depend on the coefficients)
    _, mb, _, idxb = _pair(2, A, B)
    assert torch.equal(idxb, idx0)
    mb(idxb, idxb)
    terms = mb.moe_aux("cpu").double().sum(0)
    assert terms[0].item() > 0 and terms[1].item() > 0
    for col, (a, b) in enumerate(((A, 0.0), (0.0, B))):
        cfg, m, o, idx = _pair(2, a, b)
        assert torch.equal(idx, idx0)
        l1, l2 = m(idx, idx)[1], o(idx, idx)[1]
        assert abs(l1.item() - l2.item()) <= 1e-12 * abs(l2.item())
        # the loss moved by exactly this coefficient's term, and by nothing of the other one
        added = (a, b)[col] * terms[col].item()
        assert added > 1e-4 and abs((l1.item() - lm.item()) - added) <= 1e-6 * added, (a, b, l1.item(), lm.item(), added)
        l1.backward()
        l2.backward()
        g1 = m.model.layers[0].mlp.router.weight.grad
        g2 = o.model.layers[0].mlp.router.weight.grad
        assert float((g1 - g2).abs().max()) <= 1e-12 * max(1.0, float(g2.abs().max()))
        assert float((g1 - g0).abs().max()) > 1e-6 * float(g0.abs().max())      # the router gradient did change


# ------------------------------------------------------------------------------------------- coefficients 0
def test_zero_coefficients_change_nothing():
    def run(**kw):
        cfg = get_model_config("mtiny", 32)
        cfg.n_experts, cfg.moe_capacity_factor = 4, 1.0
        for k, v in kw.items():
            setattr(cfg, k, v)
        cfg.validate()
        torch.manual_seed(0)
        m = build_model(cfg)
        idx = torch.randint(0, cfg.vocab_size, (2, 32), generator=torch.Generator().manual_seed(1))
        loss = m(idx, idx)[1]
        loss.backward()
        return m, loss, idx

    m0, l0, idx = run()
    m1, l1, _ = run(moe_aux_loss_coef=0.0, moe_z_loss_coef=0.0)
    assert torch.equal(l0, l1)
    for (n, p), (_, q) in zip(m0.named_parameters(), m1.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    assert m1._moe_aux is None
    # one output per layer, the nine saved entries, the sparse router gradient kernel
    x = torch.randn(64, m1.cfg.n_embd)
    m1._cur_bt, m1._cur_bounds = (2, 32), None
    out = mistral._LayerFn.apply(x.requires_grad_(True), m1, 0)
    assert isinstance(out, torch.Tensor)
    ws = m1.rt.acquire(m1.unit_blocks[0])
    assert len(mistral._moe_fwd(m1, 0, x.detach(), ws[4:])[1]) == 9
    # ... and two with a coefficient set
    m2, l2, _ = run(moe_z_loss_coef=B)
    assert not torch.equal(l2, l0)
    m2._cur_bt, m2._cur_bounds = (2, 32), None
    out = mistral._LayerFn.apply(x.detach().requires_grad_(True), m2, 0)
    assert isinstance(out, tuple) and len(out) == 2 and out[1].shape == (2,) and out[1].requires_grad


def test_router_wgrad_dense_flag_is_a_no_op_on_the_cpu():
    gen = torch.Generator().manual_seed(2)
    dl, h = torch.randn(24, 4, generator=gen), torch.randn(24, 64, generator=gen)
    a, b = torch.zeros(4, 64), torch.zeros(4, 64)
    F_.moe_router_wgrad(dl, h, a, False)
    F_.moe_router_wgrad(dl, h, b, False, dense=True)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------- validation
@pytest.mark.parametrize("name", ["moe_aux_loss_coef", "moe_z_loss_coef"])
@pytest.mark.parametrize("bad", [-0.01, float("nan"), float("inf"), True, "0.1"])
def test_bad_coefficients_are_refused(name, bad):
    base = get_model_config("mtiny", 64).to_dict()
    with pytest.raises(ValueError, match=name):
        ModelConfig(**dict(base, n_experts=4, **{name: bad}))


@pytest.mark.parametrize("name", ["moe_aux_loss_coef", "moe_z_loss_coef"])
def test_coefficient_without_experts_or_on_tinygpt_is_refused(name):
    base = get_model_config("mtiny", 64).to_dict()
    assert ModelConfig(**dict(base, n_experts=4, **{name: 0.5})).moe_aux_on
    assert not ModelConfig(**dict(base, n_experts=4)).moe_aux_on
    with pytest.raises(ValueError, match="n_experts"):
        ModelConfig(**dict(base, **{name: 0.5}))
    with pytest.raises(ValueError, match="moe_aux_loss_coef / moe_z_loss_coef"):
        ModelConfig(**{name: 0.5})                            # the TinyGPT arch
    cfg = get_model_config("tiny", 32)
    setattr(cfg, name, 0.5)
    with pytest.raises(ValueError):
        cfg.validate()
    with pytest.raises(ValueError, match="mistral"):
        ModelConfig(n_experts=4, **{name: 0.5})


def _harness_args(tier, res, *more):
    return ["--strategy", "zero3", "--tier", tier, "--seq-len", "32", "--steps", "2", "--warmup-steps", "1",
            "--per-device-batch", "2", "--grad-accum", "1", "--results-dir", str(res), "--device", "cpu",
            "--log-every", "0", *more]


@pytest.mark.parametrize("flag", ["--moe-aux-loss-coef", "--moe-z-loss-coef"])
def test_harness_refuses_the_flags_it_cannot_run(tmp_path, capsys, flag):
    from dltb.harness import main
    cases = [("A", (flag, "0.01")), ("B", (flag, "0.01")), ("A", ("--moe-experts", "4", flag, "0.01")),
             ("mtiny", (flag, "0.01")), ("mtiny", ("--moe-experts", "4", flag, "-1")),
             ("mtiny", ("--moe-experts", "4", flag, "nan")), ("mtiny", ("--moe-experts", "4", flag, "inf"))]
    for tier, more in cases:
        with pytest.raises(SystemExit) as e:
            main(_harness_args(tier, tmp_path / "res", *more))
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert flag in err, (tier, more, err)
        if tier in ("A", "B"):
            assert "causal tier" in err
        elif len(more) == 2:
            assert "together with --moe-experts" in err
    assert not (tmp_path / "res").exists()


# ------------------------------------------------------------------------------------------- the record
def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_world2_zero3_harness_writes_the_loss_keys(tmp_path):
    """Two gloo ranks, ZeRO-3, two steps on the CPU with both flags: the ``moe`` block names the coefficients and holds
    the last micro-step's per-layer losses of rank 0's rows; the start-up line names the coefficients."""
    res = tmp_path / "res"
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", "--max-restarts=0",
           os.path.join(ROOT, "benchmarking", "train_harness.py"),
           *_harness_args("mtiny", res, "--moe-experts", "4", "--moe-capacity-factor", "1.0",
                          "--moe-aux-loss-coef", "0.01", "--moe-z-loss-coef", "0.001")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "load-balancing loss coefficient 0.01, router z-loss coefficient 0.001" in r.stdout
    ext = [f for f in os.listdir(res) if f.endswith(".extended.json")]
    side = json.loads((res / ext[0]).read_text())
    moe = side["moe"]
    assert (moe["aux_loss_coef"], moe["z_loss_coef"]) == (0.01, 0.001)
    assert len(moe["balance_loss"]) == len(moe["z_loss"]) == 2
    assert all(v >= 0 and math.isfinite(v) for v in moe["balance_loss"] + moe["z_loss"])
    assert all(v >= 1.0 - 1e-5 for v in moe["balance_loss"])           # E sum f P >= ... 1 at balance; top-2 of 4
    assert "total" in moe["scope"]
    assert (moe["experts"], moe["top_k"], moe["capacity"], moe["capacity_factor"]) == (4, 2, 32, 1.0)
    assert len(moe["counts"]) == 2 and all(len(c) == 4 and sum(c) == 2 * 64 for c in moe["counts"])
    assert side["model"]["moe_aux_loss_coef"] == 0.01 and side["model"]["moe_z_loss_coef"] == 0.001


def test_sidecar_without_the_flags(tmp_path):
    from dltb.harness import main
    os.environ.pop("WORLD_SIZE", None)
    assert main(_harness_args("mtiny", tmp_path / "res", "--moe-experts", "4", "--moe-capacity-factor", "1.0")) == 0
    ext = [f for f in os.listdir(tmp_path / "res") if f.endswith(".extended.json")]
    moe = json.loads((tmp_path / "res" / ext[0]).read_text())["moe"]
    assert moe["balance_loss"] is None and moe["z_loss"] is None
    assert (moe["aux_loss_coef"], moe["z_loss_coef"]) == (0.0, 0.0)
    assert (moe["experts"], moe["top_k"], moe["capacity"], moe["capacity_factor"]) == (4, 2, 32, 1.0)
    assert len(moe["counts"]) == 2 and all(len(c) == 4 and sum(c) == 2 * 64 for c in moe["counts"])
    drops = sum(max(0, c - 32) for row in moe["counts"] for c in row)
    assert abs(moe["drop_fraction"] - drops / 256.0) < 1e-12

