"""Dropless mixture-of-experts routing (``moe_dropless`` / ``--moe-dropless``) on the CPU: the packed slot layout of
ops/ref.py, the grouped-GEMM definitions, the hand-written backward of the dropless layer against autograd through the
oracle in float64, its equality with the capacity layer at factor E / K, configuration, and the harness plumbing.
The GPU kernels: tests/test_moe_dropless_gpu.py."""
import json
import os

import pytest
import torch

import dltb
from dltb.harness import check_moe
from dltb.models import build_model, get_model_config
from dltb.models import mistral
from dltb.models.config import ModelConfig
from dltb.models.oracle import OracleMistral
from dltb.ops import functional as F_
from dltb.ops import ref


# ------------------------------------------------------------------------------------------- the packed layout
def _naive(expert, E):
    """The rule spelled out as a loop over the (token, choice) pairs in row-major order."""
    N, K = len(expert), len(expert[0])
    counts = [0] * E
    for row in expert:
        for e in row:
            counts[e] += 1
    offsets = [0]
    for c in counts:
        offsets.append(offsets[-1] + -(-c // 128) * 128)
    R = -(-(N * K) // 128) * 128 + 128 * E
    fill = [0] * E
    slot = [[-1] * K for _ in range(N)]
    src, src_k = [-1] * R, [-1] * R
    for n in range(N):
        for k in range(K):
            e = expert[n][k]
            s = offsets[e] + fill[e]
            fill[e] += 1
            slot[n][k] = s
            src[s], src_k[s] = n, k
    return slot, src, src_k, counts, offsets


def _routings():
    g = torch.Generator().manual_seed(1)
    out = {}
    for name, (N, E, K) in {"mixed": (37, 8, 2), "k4": (300, 5, 4), "k1": (129, 8, 1)}.items():
        out[name] = (torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(N)]).to(torch.int32), E)
    out["all_to_one"] = (torch.zeros(200, 1, dtype=torch.int32), 8)             # one segment of 256 rows, 7 empty
    out["all_to_last"] = (torch.full((128, 1), 63, dtype=torch.int32), 64)      # 63 empty segments first
    out["one_each"] = (torch.arange(64, dtype=torch.int32).view(64, 1), 64)     # 64 segments, 127 padding rows each
    out["one_each_k4"] = (torch.arange(64, dtype=torch.int32).view(16, 4), 64)
    e = torch.zeros(384, 1, dtype=torch.int32)                                  # counts of exactly 128, 127 and 129
    e[128:255] = 1
    e[255:] = 2
    out["edges_128_127_129"] = (e, 4)
    return out


@pytest.mark.parametrize("name", list(_routings()))
def test_assign_dropless_invariants(name):
    expert, E = _routings()[name]
    N, K = expert.shape
    slot, src, src_k, counts, offsets = ref.moe_assign_dropless(expert, E)
    R = ref.moe_dropless_rows(N, E, K)
    assert R == -(-(N * K) // 128) * 128 + 128 * E
    assert all(t.dtype == torch.int32 for t in (slot, src, src_k, counts, offsets))
    assert slot.shape == (N, K) and src.shape == src_k.shape == (R,)
    assert counts.shape == (E,) and offsets.shape == (E + 1,)
    want = _naive(expert.tolist(), E)
    assert [t.tolist() for t in (slot, src, src_k, counts, offsets)] == list(want)
    # segments are 128-aligned, ordered, hold their counts, and end inside [0, R]
    assert offsets[0] == 0 and (offsets % 128 == 0).all() and int(offsets[E]) <= R
    assert ((offsets[1:] - offsets[:-1]) == (counts + 127) // 128 * 128).all()
    # slot <-> src / src_k; nothing dropped; every other row is -1
    assert (slot >= 0).all()
    flat = slot.reshape(-1).long()
    assert flat.unique().numel() == N * K
    assert torch.equal(src[flat].view(N, K), torch.arange(N, dtype=torch.int32)[:, None].expand(N, K))
    assert torch.equal(src_k[flat].view(N, K), torch.arange(K, dtype=torch.int32)[None, :].expand(N, K))
    assert int((src >= 0).sum()) == int((src_k >= 0).sum()) == N * K
    rest = torch.ones(R, dtype=torch.bool)
    rest[flat] = False
    assert (src[rest] == -1).all() and (src_k[rest] == -1).all()
    for e in range(E):          # each segment: its assignments first, in (n, k) order, then padding
        seg = src[int(offsets[e]):int(offsets[e + 1])]
        c = int(counts[e])
        assert (seg[:c] >= 0).all() and (seg[c:] == -1).all()
        assert (seg[:c][1:] >= seg[:c][:-1]).all()
    assert (src[int(offsets[E]):] == -1).all()


def test_edge_counts_fill_one_one_and_two_tiles():
    expert, E = _routings()["edges_128_127_129"]
    _, _, _, counts, offsets = ref.moe_assign_dropless(expert, E)
    assert counts.tolist() == [128, 127, 129, 0] and offsets.tolist() == [0, 128, 256, 512, 512]


def test_same_order_as_the_capacity_layout():
    """With a capacity nobody exceeds, position p of expert e is the capacity path's slot e C + p."""
    expert, E = _routings()["mixed"]
    N, K = expert.shape
    slot, src, _, counts, offsets = ref.moe_assign_dropless(expert, E)
    C = ref.moe_capacity(N, E, K, E / K)
    cslot, csrc, _, ccounts = ref.moe_assign(expert, E, C)
    assert torch.equal(counts, ccounts) and (cslot >= 0).all()
    e = expert.long()
    assert torch.equal(slot.long() - offsets[e].long(), cslot.long() - e * C)


# ------------------------------------------------------------------------------------------- grouped GEMM definitions
def test_grouped_gemm_reference_definitions():
    g = torch.Generator().manual_seed(2)
    offsets = torch.tensor([0, 0, 128, 384, 384], dtype=torch.int32)           # empty, 128, 256, empty; tail of 128
    R, Kd, N = 512, 64, 128
    a = torch.randn(R, Kd, generator=g, dtype=torch.float64)
    bs = [torch.randn(N, Kd, generator=g, dtype=torch.float64) for _ in range(4)]
    c = ref.gemm_grouped_nt(a, offsets, bs)
    assert torch.equal(c[:128], a[:128] @ bs[1].t()) and torch.equal(c[128:384], a[128:384] @ bs[2].t())
    assert (c[384:] == 0).all()
    out = torch.full((R, N), 7.0, dtype=torch.float64)
    assert ref.gemm_grouped_nt(a, offsets, bs, out) is out and torch.equal(out, c)
    x = torch.randn(R, 32, generator=g, dtype=torch.float64)
    dws = [torch.full((Kd, 32), 5.0, dtype=torch.float64) for _ in range(4)]
    ref.gemm_grouped_tn(a, x, offsets, dws, [True, False, True, False])
    assert (dws[0] == 5.0).all()                                               # empty and accumulating: untouched
    assert torch.equal(dws[1], a[:128].t() @ x[:128])
    assert torch.equal(dws[2], a[128:384].t() @ x[128:384] + 5.0)
    assert (dws[3] == 0).all()                                                 # empty, not accumulating: zeros
    # the wrappers take the CPU definitions for CPU tensors
    assert torch.equal(F_.gemm_grouped_nt(a, offsets, bs), c)


# ------------------------------------------------------------------------------------------- the layer
def _layer_pair(E, K, aux=(0.0, 0.0), N=72, d=128, f=128):
    """One float64 layer, as a dropless model and as a capacity model at factor E / K with the same weights.  The
    router is biased, so that the experts' counts differ widely."""
    kw = dict(arch="mistral", vocab_size=64, n_embd=d, n_head=1, n_kv_head=1, n_layer=1, ffn_hidden=f, block_size=N,
              dropout=0.0, causal=True, tie_embeddings=False, n_experts=E, moe_top_k=K, moe_aux_loss_coef=aux[0],
              moe_z_loss_coef=aux[1])
    torch.manual_seed(3)
    drop = mistral.MistralLM(ModelConfig(moe_dropless=True, **kw)).double()
    g = torch.Generator().manual_seed(4)
    u = torch.randn(d, generator=g, dtype=torch.float64)
    u /= u.norm()
    h = 0.5 * torch.randn(N, d, generator=g, dtype=torch.float64) + u
    with torch.no_grad():
        mlp = drop.model.layers[0].mlp
        mlp.router.weight.mul_(20.0)
        mlp.router.weight[0] += 3.0 * u
        for ex in mlp.experts:
            ex.gate_up_proj.weight.mul_(10.0)
            ex.down_proj.weight.mul_(10.0)
    cap = mistral.MistralLM(ModelConfig(moe_capacity_factor=E / K, **kw)).double()
    cap.load_state_dict(drop.state_dict())
    dm = torch.randn(N, d, generator=g, dtype=torch.float64)
    return drop, cap, h, dm


def _run_layer(model, h, dm, daux=None):
    unit = model.unit_blocks[0]
    ws = model.rt.acquire(unit)
    out = mistral._moe_fwd(model, 0, h, ws[4:])
    s = [(torch.full_like(w, float("nan")), False) for w in ws]
    dh = mistral._moe_bwd(model, unit, dm, h, ws, s, out[1], daux)
    return out, dh, [t for t, _ in s[4:]]


@pytest.mark.parametrize("aux", [(0.0, 0.0), (0.02, 0.001)], ids=["plain", "aux"])
@pytest.mark.parametrize("E,K", [(4, 1), (4, 2), (8, 4)])
def test_dropless_layer_equals_capacity_layer_at_factor_e_over_k(E, K, aux):
    drop, cap, h, dm = _layer_pair(E, K, aux)
    daux = torch.tensor([0.7, -0.3], dtype=torch.float64) if any(aux) else None
    (m_d, *rest_d), dh_d, g_d = _run_layer(drop, h, dm, daux)
    (m_c, *rest_c), dh_c, g_c = _run_layer(cap, h, dm, daux)
    counts = drop.moe_counts("cpu")[0]
    assert torch.equal(counts, cap.moe_counts("cpu")[0]) and int(counts.sum()) == h.shape[0] * K
    assert int(counts.max()) > 2 * int(counts.min())                          # unequal segments
    saved = rest_d[0]
    assert saved[4].shape[0] == ref.moe_dropless_rows(h.shape[0], E, K)         # xe is [R, d]
    assert torch.allclose(m_d, m_c, rtol=1e-12, atol=1e-14)
    assert torch.allclose(dh_d, dh_c, rtol=1e-12, atol=1e-14)
    for a, b in zip(g_d, g_c):
        assert torch.isfinite(a).all() and torch.allclose(a, b, rtol=1e-12, atol=1e-14)
    if any(aux):
        assert torch.equal(rest_d[1], rest_c[1])                               # the layer's (balance, z)


def test_dropless_layer_accumulates_into_its_slots():
    drop, _, h, dm = _layer_pair(4, 2)
    unit = drop.unit_blocks[0]
    ws = drop.rt.acquire(unit)
    _, _, g1 = _run_layer(drop, h, dm)
    m, saved = mistral._moe_fwd(drop, 0, h, ws[4:])
    s = [(torch.ones_like(w), True) for w in ws]
    mistral._moe_bwd(drop, unit, dm, h, ws, s, saved)
    for (t, _), g in zip(s[4:], g1):
        assert torch.allclose(t, g + 1.0, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("aux", [(0.0, 0.0), (0.01, 0.001)], ids=["plain", "aux"])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_hand_written_backward_against_autograd_float64(K, aux):
    """The dropless model (hand-written layer backward, grouped products on the CPU definitions) against the oracle,
    which autograd differentiates: mtiny, E = 4, 64 rows."""
    cfg = ModelConfig(**dict(get_model_config("mtiny", 32).to_dict(), n_experts=4, moe_top_k=K, moe_dropless=True,
                             moe_aux_loss_coef=aux[0], moe_z_loss_coef=aux[1]))
    torch.manual_seed(0)
    m = build_model(cfg).double()
    o = OracleMistral(cfg).double()
    o.load_state_dict(m.state_dict())
    idx = torch.randint(0, cfg.vocab_size, (2, 32))
    packed = []                                         # the row counts the experts' products ran on
    real = F_.gemm_grouped_nt

    def spy(a, offsets, bs, out=None):
        packed.append(a.shape[0])
        return real(a, offsets, bs, out)

    F_.gemm_grouped_nt = spy
    try:
        l1, l2 = m(idx, idx)[1], o(idx, idx)[1]
        assert abs(l1.item() - l2.item()) <= 1e-12 * abs(l2.item())
        l1.backward()
        l2.backward()
    finally:
        F_.gemm_grouped_nt = real
    # the dropless path did run: four grouped NT products per layer, each on the R packed rows
    assert packed == [ref.moe_dropless_rows(64, 4, K)] * (4 * cfg.n_layer)
    assert (m.moe_counts("cpu").sum(1) == 64 * K).all()
    for (n, p), (n2, p2) in zip(m.named_parameters(), o.named_parameters()):
        assert n == n2
        tol = 1e-8 if "layernorm" in n or n == "model.norm.weight" else 1e-12      # norm slots pass through fp32
        assert float((p.grad - p2.grad).abs().max()) <= tol * max(1.0, float(p2.grad.abs().max())), n
    if K > 1 or any(aux):
        assert float(m.model.layers[0].mlp.router.weight.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------- configuration
def test_default_is_off_and_old_dicts_load():
    cfg = get_model_config("mtiny", 64)
    assert cfg.moe_dropless is False
    old = {k: v for k, v in cfg.to_dict().items() if k != "moe_dropless"}
    assert ModelConfig(**old).moe_dropless is False


@pytest.mark.parametrize("bad", [dict(moe_dropless=True),                                   # no experts
                                 dict(moe_dropless=1, n_experts=4),                          # not a bool
                                 dict(moe_dropless=True, n_experts=4, n_embd=192, n_head=3, n_kv_head=1),
                                 dict(moe_dropless=True, n_experts=4, ffn_hidden=320)])
def test_config_refusals(bad):
    base = get_model_config("mtiny", 64).to_dict()
    with pytest.raises(ValueError, match="moe_dropless"):
        ModelConfig(**dict(base, **bad))


def test_non_mistral_arch_is_refused():
    cfg = get_model_config("tiny", 32)
    cfg.moe_dropless = True
    with pytest.raises(ValueError, match="moe_dropless"):
        cfg.validate()


def test_recompute_is_refused_by_the_model():
    cfg = get_model_config("mtiny", 32)
    cfg.n_experts, cfg.moe_dropless = 4, True
    model = build_model(cfg)
    model.activation_recompute = "selective"
    idx = torch.randint(0, cfg.vocab_size, (1, 32))
    with pytest.raises(ValueError, match=r"--activation-recompute.*--moe-experts"):
        model(idx, idx)


def test_check_moe_refusals_and_setting():
    mt = lambda: get_model_config("mtiny", 32)
    with pytest.raises(ValueError, match="--moe-dropless is only used together with --moe-experts"):
        check_moe(None, None, None, "off", mt(), "mtiny", dropless=True)
    with pytest.raises(ValueError, match="--moe-dropless needs --moe-experts on a causal tier"):
        check_moe(4, None, None, "off", get_model_config("tiny", 32), "tiny", dropless=True)
    with pytest.raises(ValueError, match="--moe-capacity-factor 1.25 cannot be given"):
        check_moe(4, None, 1.25, "off", mt(), "mtiny", dropless=True)          # explicit, even at the default's value
    with pytest.raises(ValueError, match="--activation-recompute"):
        check_moe(4, None, None, "full", mt(), "mtiny", dropless=True)
    cfg = mt()
    check_moe(4, 1, None, "off", cfg, "mtiny", 0.01, None, dropless=True)
    assert cfg.moe_dropless is True and cfg.n_experts == 4 and cfg.moe_top_k == 1 and cfg.moe_aux_loss_coef == 0.01
    cfg = mt()
    check_moe(4, None, 2.0, "off", cfg, "mtiny")                               # the flag off: as before
    assert cfg.moe_dropless is False and cfg.moe_capacity_factor == 2.0


# ------------------------------------------------------------------------------------------- harness
def _harness_args(res, *more):
    return ["--strategy", "zero3", "--tier", "mtiny", "--seq-len", "32", "--steps", "2", "--warmup-steps", "1",
            "--per-device-batch", "2", "--grad-accum", "1", "--results-dir", str(res), "--device", "cpu",
            "--log-every", "0", *more]


def test_harness_refuses_what_it_cannot_run(tmp_path, capsys):
    from dltb.harness import main
    for more, msg in ((("--moe-dropless",), "only used together with --moe-experts"),
                      (("--moe-dropless", "--moe-experts", "4", "--moe-capacity-factor", "2.0"), "cannot be given"),
                      (("--moe-dropless", "--moe-experts", "4", "--activation-recompute", "full"),
                       "--activation-recompute")):
        with pytest.raises(SystemExit) as e:
            main(_harness_args(tmp_path / "res", *more))
        assert e.value.code == 2
        assert msg in capsys.readouterr().err, more
    assert not (tmp_path / "res").exists()


def test_harness_record_and_start_up_line(tmp_path, capsys):
    from dltb.harness import main
    os.environ.pop("WORLD_SIZE", None)
    res = tmp_path / "res"
    assert main(_harness_args(res, "--moe-experts", "4", "--moe-dropless")) == 0
    R = ref.moe_dropless_rows(64, 4, 2)
    assert R == 128 + 512
    out = capsys.readouterr().out
    assert f"Mixture of experts: 4 experts, top-2, dropless: {R} packed slot rows (R)" in out
    ext = [f for f in os.listdir(res) if f.endswith(".extended.json")]
    plain = [f for f in os.listdir(res) if f.endswith(".json") and not f.endswith(".extended.json")]
    rec, side = json.loads((res / plain[0]).read_text()), json.loads((res / ext[0]).read_text())
    moe = side["moe"]
    assert moe["dropless"] is True and moe["rows"] == R and moe["capacity"] is None and moe["drop_fraction"] == 0.0
    assert (moe["experts"], moe["top_k"]) == (4, 2)
    assert len(moe["counts"]) == 2 and all(len(c) == 4 and sum(c) == 128 for c in moe["counts"])
    assert side["model"]["moe_dropless"] is True
    assert not any("moe" in k for k in rec)


def test_capacity_record_is_unchanged(tmp_path):
    from dltb.harness import main
    os.environ.pop("WORLD_SIZE", None)
    res = tmp_path / "res"
    assert main(_harness_args(res, "--moe-experts", "4")) == 0
    ext = [f for f in os.listdir(res) if f.endswith(".extended.json")]
    moe = json.loads((res / ext[0]).read_text())["moe"]
    assert "dropless" not in moe and "rows" not in moe and moe["capacity"] == 48
