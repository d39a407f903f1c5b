"""Top-k mixture-of-experts FFN of the causal tiers (``n_experts`` / ``--moe-experts``): the reference semantics of
ops/ref.py (slot order, tie rule, capacity), the hand-written backward of models/mistral.py against autograd through
the oracle branch in float64, configuration, and the harness plumbing.  The GPU kernels: tests/test_moe_gpu.py."""
import json
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
from dltb.ops import ref
from dltb.parallel import engine_config, make_engine
from dltb.parallel.checkpoint import load_checkpoint, save_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- reference semantics
def _naive_assign(expert, E, C):
    """The slot rule spelled out as a loop over the (token, choice) pairs in row-major order."""
    N, K = len(expert), len(expert[0])
    fill = [0] * E
    slot = [[-1] * K for _ in range(N)]
    src, src_k = [-1] * (E * C), [-1] * (E * C)
    for n in range(N):
        for k in range(K):
            e = expert[n][k]
            p = fill[e]
            fill[e] += 1
            if p < C:
                slot[n][k] = e * C + p
                src[e * C + p], src_k[e * C + p] = n, k
    return slot, src, src_k, fill


def test_slot_order_overflow_and_empty_expert():
    # 12 tokens, E = 3, K = 2, C = 4: experts 0 and 1 are chosen 12 times each (8 dropped), expert 2 never
    expert = [[0, 1], [1, 0], [0, 1], [0, 1], [0, 1], [1, 0], [0, 1], [1, 0], [0, 1], [1, 0], [0, 1], [1, 0]]
    E, C = 3, 4
    slot, src, src_k, counts = ref.moe_assign(torch.tensor(expert, dtype=torch.int32), E, C)
    want = _naive_assign(expert, E, C)
    assert slot.tolist() == want[0] and src.tolist() == want[1] and src_k.tolist() == want[2]
    assert counts.tolist() == want[3] == [12, 12, 0]
    assert slot.dtype == src.dtype == src_k.dtype == counts.dtype == torch.int32
    # exactly the first C assignments of the overflowing experts are kept, in (n, k) order; expert 2 is empty
    assert src[:4].tolist() == [0, 1, 2, 3] and src_k[:4].tolist() == [0, 1, 0, 0]
    assert src[4:8].tolist() == [0, 1, 2, 3] and src_k[4:8].tolist() == [1, 0, 1, 1]
    assert src[8:].tolist() == [-1] * 4
    assert (slot[4:] == -1).all() and (slot[:4] >= 0).all()


def test_slot_order_mixed_routing_matches_the_loop():
    g = torch.Generator().manual_seed(1)
    for E, K, C in ((3, 2, 4), (8, 2, 16), (5, 4, 16), (8, 1, 16)):
        expert = torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(37)]).to(torch.int32)
        expert[:20, 0] = 0                                             # crowd expert 0 (rows stay distinct below)
        expert[:20, 1:] = torch.stack([1 + torch.randperm(E - 1, generator=g)[:K - 1] for _ in range(20)]).to(torch.int32)
        got = ref.moe_assign(expert, E, C)
        want = _naive_assign(expert.tolist(), E, C)
        assert [t.tolist() for t in got] == list(want), (E, K, C)
        assert want[3][0] > C                                          # the case does overflow


def test_capacity_formula():
    assert ref.moe_capacity(200, 8, 2, 1.25) == 64                     # ceil(62.5) = 63 -> 64
    assert ref.moe_capacity(4096, 8, 2, 1.0) == 1024
    assert ref.moe_capacity(24, 4, 2, 1.0) == 16                       # 12 -> 16
    assert ref.moe_capacity(24, 4, 2, 8.0) == 32                       # min(96, N = 24) -> 32
    assert ref.moe_capacity(128, 4, 2, 2.0) == 128                     # F = E / K: nothing can drop


def test_tie_rule_lowest_index_first():
    wr = torch.zeros(6, 64)
    h = torch.randn(5, 64)
    expert, gate, logits = ref.moe_route(h, wr, 4)
    assert expert.tolist() == [[0, 1, 2, 3]] * 5                       # identical logits: the lowest indices
    assert torch.equal(gate, torch.full((5, 4), 0.25)) and torch.equal(logits, torch.zeros(5, 6))
    # a strict maximum first, then the tie between the rest in index order
    wr[4, 0] = 1.0
    h[:, 0] = 2.0
    expert, gate, _ = ref.moe_route(h, wr, 2)
    assert expert.tolist() == [[4, 0]] * 5
    assert torch.allclose(gate[:, 0], torch.tensor(2.0).exp() / (1 + torch.tensor(2.0).exp()))
    # two pairs of equal logits: descending logit, ascending index inside a tie
    wr = torch.zeros(5, 64)
    wr[1, 0] = wr[3, 0] = 1.0
    wr[0, 0] = -1.0
    expert, _, _ = ref.moe_route(h, wr, 4)
    assert expert.tolist() == [[1, 3, 2, 4]] * 5


# ------------------------------------------------------------------------------------------- hand-written backward
def _grad_case():
    """N = 24, d = 64, f = 32, E = 4, K = 2 in float64, C = 16.  The router is biased so that expert 0 overflows:
    some tokens lose one assignment, one at least loses both, and one expert's slab is partly empty."""
    cfg = ModelConfig(arch="mistral", vocab_size=64, n_embd=64, n_head=1, n_kv_head=1, n_layer=1, ffn_hidden=32,
                      block_size=24, dropout=0.0, causal=True, tie_embeddings=False, n_experts=4, moe_top_k=2,
                      moe_capacity_factor=1.0)
    torch.manual_seed(3)
    model = mistral.MistralLM(cfg).double()
    oracle = OracleMistral(cfg).double()
    g = torch.Generator().manual_seed(4)
    u = torch.randn(64, generator=g, dtype=torch.float64)
    u /= u.norm()
    h = 0.5 * torch.randn(24, 64, generator=g, dtype=torch.float64) + u
    with torch.no_grad():
        wr = model.model.layers[0].mlp.router.weight
        wr.mul_(20.0)
        wr[0] += 3.0 * u            # nearly every token's first choice
        wr[1] += 2.2 * u            # the usual second choice, not always
        for ex in model.model.layers[0].mlp.experts:     # larger weights: gradients well above rounding
            ex.gate_up_proj.weight.mul_(10.0)
            ex.down_proj.weight.mul_(10.0)
    oracle.load_state_dict(model.state_dict())
    dm = torch.randn(24, 64, generator=g, dtype=torch.float64)
    return cfg, model, oracle, h, dm


def test_backward_formulas_against_autograd_float64():
    cfg, model, oracle, h, dm = _grad_case()
    unit = model.unit_blocks[0]
    ws = model.rt.acquire(unit)
    m, saved = mistral._moe_fwd(model, 0, h, ws[4:])
    slot, src = saved[2], saved[3]
    dropped = slot < 0
    assert dropped.all(1).any(), "no token lost both assignments"
    assert (dropped.any(1) & ~dropped.all(1)).any(), "no token lost exactly one"
    assert (~dropped.any(1)).any(), "no token kept both"
    assert (src.view(4, 16) < 0).any() and (src.view(4, 16)[0] >= 0).all()        # a partly empty slab; expert 0 full
    assert model.moe_counts("cpu")[0].tolist() == ref.moe_assign(saved[0], 4, 16)[3].tolist()
    assert int(model.moe_counts("cpu")[0].sum()) == 48
    # autograd through the oracle branch
    h_o = h.clone().requires_grad_(True)
    mlp = oracle.model.layers[0].mlp
    from dltb.models.oracle import _moe_ffn
    m_o = _moe_ffn(mlp, h_o, cfg)
    assert torch.allclose(m, m_o, rtol=1e-12, atol=1e-14)
    assert (m[dropped.all(1)] == 0).all()                                          # only the residual passes
    m_o.backward(dm)
    s = [model.rt.grad_slot(unit, j) for j in range(len(ws))]
    for t, _ in s[4:]:
        t.fill_(float("nan"))                                                       # accumulate = False overwrites
    dh = mistral._moe_bwd(model, unit, dm, h, ws, s, saved)
    want = {n: p.grad for n, p in oracle.named_parameters() if ".mlp." in n}
    got = {n: p.grad for n, p in model.named_parameters() if ".mlp." in n}
    assert sorted(want) == sorted(got) and len(got) == 9
    scale = max(float(v.abs().max()) for v in want.values())
    for n in want:
        assert float((want[n] - got[n]).abs().max()) <= 1e-12 * scale, n
    assert float(want["model.layers.0.mlp.router.weight"].abs().max()) > 1e-3 * scale   # the gates do carry gradient
    assert float((dh - h_o.grad).abs().max()) <= 1e-12 * float(h_o.grad.abs().max())
    # a second call accumulates
    m2, saved2 = mistral._moe_fwd(model, 0, h, ws[4:])
    s2 = [model.rt.grad_slot(unit, j) for j in range(len(ws))]
    assert all(acc for _, acc in s2)
    mistral._moe_bwd(model, unit, dm, h, ws, s2, saved2)
    for n in want:
        assert float((2 * want[n] - got[n]).abs().max()) <= 4e-12 * scale, n


def test_model_against_oracle_float64():
    cfg = get_model_config("mtiny", 32)
    cfg.n_experts, cfg.moe_capacity_factor = 4, 1.0
    cfg.validate()
    torch.manual_seed(0)
    m = build_model(cfg).double()
    o = OracleMistral(cfg).double()
    o.load_state_dict(m.state_dict())
    idx = torch.randint(0, cfg.vocab_size, (2, 32))
    l1, l2 = m(idx, idx)[1], o(idx, idx)[1]
    assert abs(l1.item() - l2.item()) <= 1e-12 * abs(l2.item())
    l1.backward()
    l2.backward()
    counts = m.moe_counts("cpu")
    assert int((counts - ref.moe_capacity(64, 4, 2, 1.0)).clamp(min=0).sum()) > 0      # the run does drop
    for (n, p), (n2, p2) in zip(m.named_parameters(), o.named_parameters()):
        assert n == n2
        tol = 1e-8 if "layernorm" in n or n == "model.norm.weight" else 1e-12      # norm slots pass through fp32
        assert float((p.grad - p2.grad).abs().max()) <= tol * max(1.0, float(p2.grad.abs().max())), n


# ------------------------------------------------------------------------------------------- configuration
def test_mtiny_moe_names_params_and_flops():
    cfg = get_model_config("mtiny", 64)
    cfg.n_experts = 4
    cfg.validate()
    model = build_model(cfg)
    names = [n for n, _ in model.named_parameters()]
    layer0 = [n for n in names if n.startswith("model.layers.0.")]
    assert layer0 == [f"model.layers.0.{n}" for n in
                      ["input_layernorm.weight", "self_attn.qkv_proj.weight", "self_attn.o_proj.weight",
                       "post_attention_layernorm.weight", "mlp.router.weight"]
                      + [f"mlp.experts.{e}.{w}.weight" for e in range(4) for w in ("gate_up_proj", "down_proj")]]
    assert [n.split("model.layers.0.")[1] for n in layer0] == [n for n, _ in model.model.layers[0].param_list()]
    assert cfg.num_params() == model.num_params() == sum(p.numel() for p in model.parameters())
    d, f, V, L, T = 128, 256, 256, 2, 64
    assert cfg.num_params() == V * d + L * (d + (d * d + 2 * 64 * d) + d * d + d + 4 * d + 4 * 3 * d * f) + d + V * d
    # per token: top-2 experts' FFN and the router product; attention causal
    n_mat = L * (2 * d * d + 2 * 64 * d + 2 * 3 * d * f + 4 * d) + V * d
    assert cfg.train_flops_per_token(T) == 6.0 * n_mat + 12 * L * T * d * 0.5
    std = float(model.model.layers[1].mlp.router.weight.std())
    assert 0.015 < std < 0.025                                         # router init: std 0.02


def test_defaults_are_unchanged():
    cfg = get_model_config("mtiny", 64)
    assert cfg.n_experts is None and cfg.moe_top_k == 2 and cfg.moe_capacity_factor == 1.25
    torch.manual_seed(0)
    model = build_model(cfg)
    assert [n for n, _ in model.model.layers[0].param_list()] == [
        "input_layernorm.weight", "self_attn.qkv_proj.weight", "self_attn.o_proj.weight",
        "post_attention_layernorm.weight", "mlp.gate_up_proj.weight", "mlp.down_proj.weight"]
    assert cfg.num_params() == model.num_params() == 361_088
    assert get_model_config("M7B", 4096).num_params() == 7_241_732_096
    old = {k: v for k, v in cfg.to_dict().items() if not k.startswith("moe_") and k != "n_experts"}
    assert ModelConfig(**old).n_experts is None                        # a dict saved before the keys existed
    assert ModelConfig(**dict(old, n_experts=8)).to_dict()["n_experts"] == 8


@pytest.mark.parametrize("bad", [dict(n_experts=1), dict(n_experts=65), dict(n_experts=2.0), dict(n_experts=True),
                                 dict(n_experts=8, moe_top_k=3), dict(n_experts=2, moe_top_k=4),
                                 dict(n_experts=8, moe_top_k=0), dict(n_experts=8, moe_capacity_factor=0.0),
                                 dict(n_experts=8, moe_capacity_factor=float("inf")),
                                 dict(n_experts=8, n_embd=96, n_head=1, n_kv_head=1)])
def test_out_of_range_values_are_refused(bad):
    base = get_model_config("mtiny", 64).to_dict()
    with pytest.raises(ValueError):
        ModelConfig(**dict(base, **bad))


def test_non_mistral_arch_is_refused():
    with pytest.raises(ValueError, match="mistral"):
        ModelConfig(n_experts=4)
    with pytest.raises(ValueError, match="mistral"):
        ModelConfig(moe_top_k=1)
    cfg = get_model_config("tiny", 32)
    cfg.n_experts = 4
    with pytest.raises(ValueError, match="mistral"):
        cfg.validate()


def test_recompute_with_moe_is_refused_by_the_model():
    cfg = get_model_config("mtiny", 32)
    cfg.n_experts = 4
    model = build_model(cfg)
    model.activation_recompute = "selective"
    idx = torch.randint(0, cfg.vocab_size, (1, 32))
    with pytest.raises(ValueError, match=r"--activation-recompute.*--moe-experts"):
        model(idx, idx)


# ------------------------------------------------------------------------------------------- harness
def _harness_args(tier, res, *more):
    return ["--strategy", "zero3", "--tier", tier, "--seq-len", "32", "--steps", "2", "--warmup-steps", "1",
            "--per-device-batch", "2", "--grad-accum", "1", "--results-dir", str(res), "--device", "cpu",
            "--log-every", "0", *more]


@pytest.mark.parametrize("tier", ["A", "tiny"])
@pytest.mark.parametrize("flag", [("--moe-experts", "4"), ("--moe-experts", "4", "--moe-top-k", "1")])
def test_harness_refuses_moe_on_the_tinygpt_tiers(tmp_path, capsys, tier, flag):
    from dltb.harness import main
    with pytest.raises(SystemExit) as e:
        main(_harness_args(tier, tmp_path / "res", *flag))
    assert e.value.code == 2
    assert "--moe-experts needs a causal tier" in capsys.readouterr().err
    assert not (tmp_path / "res").exists()


def test_harness_refuses_moe_flags_it_cannot_run(tmp_path, capsys):
    from dltb.harness import main
    for more, msg in ((("--activation-recompute", "selective", "--moe-experts", "4"), "--activation-recompute"),
                      (("--moe-top-k", "1"), "together with --moe-experts"),
                      (("--moe-experts", "4", "--moe-top-k", "3"), "moe_top_k"),
                      (("--moe-experts", "1"), "n_experts")):
        with pytest.raises(SystemExit) as e:
            main(_harness_args("mtiny", tmp_path / "res", *more))
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert msg in err and ("--moe-experts" in err or "moe" in err), (more, err)
    assert not (tmp_path / "res").exists()


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_world2_zero3_harness_writes_the_moe_block(tmp_path):
    """Two gloo ranks, ZeRO-3, two steps on the CPU: the extended sidecar carries the ``moe`` block (experts, top_k,
    capacity for the local rows, the last micro-step's counts per layer and expert, the drop fraction); the
    reference-format record does not change."""
    res = tmp_path / "res"
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", "--max-restarts=0",
           os.path.join(ROOT, "benchmarking", "train_harness.py"),
           *_harness_args("mtiny", res, "--moe-experts", "4", "--moe-capacity-factor", "1.0")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Mixture of experts: 4 experts, top-2, capacity 32 slots" in r.stdout
    ext = [f for f in os.listdir(res) if f.endswith(".extended.json")]
    plain = [f for f in os.listdir(res) if f.endswith(".json") and not f.endswith(".extended.json")]
    rec, side = json.loads((res / plain[0]).read_text()), json.loads((res / ext[0]).read_text())
    moe = side["moe"]
    assert (moe["experts"], moe["top_k"], moe["capacity"], moe["capacity_factor"]) == (4, 2, 32, 1.0)
    assert "local" in moe["scope"] and "rank" in moe["scope"]           # rank 0's rows, said in the block itself
    assert len(moe["counts"]) == 2 and all(len(c) == 4 and sum(c) == 2 * 64 for c in moe["counts"])
    drops = sum(max(0, c - 32) for row in moe["counts"] for c in row)
    assert abs(moe["drop_fraction"] - drops / 256.0) < 1e-12
    assert side["model"]["n_experts"] == 4 and side["params"] == 951_936
    assert not any("moe" in k for k in rec)
    cfg = get_model_config("mtiny", 32)
    cfg.n_experts = 4
    assert side["train_flops_per_token"] == cfg.train_flops_per_token(32)


def test_dense_sidecar_has_no_moe_block(tmp_path):
    from dltb.harness import main
    os.environ.pop("WORLD_SIZE", None)
    assert main(_harness_args("mtiny", tmp_path / "res")) == 0
    ext = [f for f in os.listdir(tmp_path / "res") if f.endswith(".extended.json")]
    side = json.loads((tmp_path / "res" / ext[0]).read_text())
    assert side["moe"] is None and side["model"]["n_experts"] is None


def test_save_resume_restores_experts_and_router(tmp_path):
    def engine():
        cfg = get_model_config("mtiny", 32)
        cfg.n_experts = 4
        cfg.validate()
        torch.manual_seed(0)
        return make_engine(build_model(cfg), engine_config("zero3", 1, "reference", bucket_mb=0.01), "cpu")

    g = torch.Generator().manual_seed(5)
    batches = [torch.randint(0, 256, (2, 32), generator=g) for _ in range(3)]

    def train(eng, bs):
        eng.train()
        for b in bs:
            eng.backward(eng(b, b)[1])
            eng.step()

    e1 = engine()
    init = {n: t.clone() for n, t in e1.full_state_dict().items()}
    train(e1, batches[:2])
    save_checkpoint(e1, str(tmp_path / "ck"))
    saved = {n: t.clone() for n, t in e1.full_state_dict().items()}
    e2 = engine()
    load_checkpoint(e2, str(tmp_path / "ck"))
    got = e2.full_state_dict()
    moe_names = [n for n in saved if ".mlp.router." in n or ".mlp.experts." in n]
    assert len(moe_names) == 2 * 9
    for n in saved:
        assert torch.equal(saved[n], got[n]), n
    for n in moe_names:
        assert not torch.equal(saved[n], init[n]), n                   # they did train
    train(e1, batches[2:])
    train(e2, batches[2:])
    for n, t in e1.full_state_dict().items():
        assert torch.equal(t, e2.full_state_dict()[n]), n
