"""Document-masked causal attention for packed sequences on the CPU.  A token equal to the EOS id ends a
document and belongs to it; query i sees key j iff ``lo[i] <= j <= i`` (the same as ``j <= i < hi[j]``).
``ref.doc_bounds`` against a brute-force double loop, the reference ops against a dense fp64 masked softmax and
its autograd gradients, the Mistral-shape model against the stock-op oracle and against documents run on their
own, the synthetic data, the FLOP count and the harness flags."""
import json
import math
import os

import pytest
import torch

import dltb
from dltb.data.synthetic import SyntheticDataset
from dltb.models import ModelConfig, get_model_config
from dltb.models.mistral import MistralLM
from dltb.models.oracle import OracleMistral
from dltb.ops import functional as F_
from dltb.ops import ref
from dltb.ops.rng import StepSeed

B, T, HQ, HKV, D = 2, 32, 4, 2, 8
SCALE = 1.0 / math.sqrt(D)
SITE = 11
EOS = 7


def _seed():
    s = StepSeed(1234, 0)
    s.next()
    return s


def _inputs():
    g = torch.Generator().manual_seed(0)
    q = torch.randn(B * T, HQ * D, generator=g, dtype=torch.float64)
    k = torch.randn(B * T, HKV * D, generator=g, dtype=torch.float64)
    v = torch.randn(B * T, HKV * D, generator=g, dtype=torch.float64)
    do = torch.randn(B * T, HQ * D, generator=g, dtype=torch.float64)
    return q, k, v, do


def _brute(idx, eos, window):
    """lo / hi by the definition, one position at a time."""
    Bn, Tn = idx.shape
    out = torch.zeros(2, Bn, Tn, dtype=torch.int32)
    for b in range(Bn):
        for i in range(Tn):
            lo = 0
            for e in range(i):
                if idx[b, e] == eos:
                    lo = e + 1
            hi = Tn
            for e in range(Tn - 1, i - 1, -1):
                if idx[b, e] == eos:
                    hi = e + 1
            if window > 0:
                lo, hi = max(lo, i - window + 1), min(hi, i + window)
            out[0, b, i], out[1, b, i] = lo, hi
    return out


def _layouts(Tn):
    g = torch.Generator().manual_seed(Tn)
    rnd = torch.randint(0, EOS, (3, Tn), generator=g, dtype=torch.int64)
    rnd[torch.rand(3, Tn, generator=g) < 0.2] = EOS
    none = torch.randint(0, EOS, (1, Tn), generator=g, dtype=torch.int64)
    first, last, every = none.clone(), none.clone(), torch.full((1, Tn), EOS, dtype=torch.int64)
    first[0, 0] = EOS
    last[0, Tn - 1] = EOS
    return torch.cat([rnd, none, first, last, every])


@pytest.mark.parametrize("window", [0, 1, 7, 40, 1000])
@pytest.mark.parametrize("Tn", [1, 2, 40])
def test_doc_bounds_matches_brute_force(Tn, window):
    idx = _layouts(Tn)
    got = ref.doc_bounds(idx, EOS, window)
    assert got.dtype == torch.int32 and tuple(got.shape) == (2, idx.shape[0], Tn)
    assert torch.equal(got, _brute(idx, EOS, window))
    lo, hi = got[0].long(), got[1].long()
    pos = torch.arange(Tn).expand_as(lo)
    assert (lo[:, 1:] >= lo[:, :-1]).all() and (hi[:, 1:] >= hi[:, :-1]).all()        # monotone
    assert (lo <= pos).all() and (pos < hi).all() and (hi <= Tn).all() and (lo >= 0).all()
    vis_lo = (lo[:, :, None] <= pos[:, None, :]) & (pos[:, None, :] <= pos[:, :, None])      # [b, i, j]
    vis_hi = (pos[:, None, :] <= pos[:, :, None]) & (pos[:, :, None] < hi[:, None, :])
    assert torch.equal(vis_lo, vis_hi)                                                # the two forms agree
    assert torch.equal(F_.doc_bounds(idx, EOS, window), got)                          # the CPU path of the public op


def _rows_idx():
    idx = torch.randint(0, EOS, (B, T), generator=torch.Generator().manual_seed(3), dtype=torch.int64)
    idx[0, [4, 5, 20]] = EOS
    idx[1, [0, 15, 31]] = EOS
    return idx


def _dense(q, k, v, idx, window, p, sd):
    """softmax over the same-document causal pairs (and the band), written out densely in fp64."""
    heads = lambda t, H: t.reshape(B, T, H, D).transpose(1, 2)
    qh = heads(q, HQ)
    kh = heads(k, HKV).repeat_interleave(HQ // HKV, 1)
    vh = heads(v, HKV).repeat_interleave(HQ // HKV, 1)
    i = torch.arange(T)
    eos = (idx == EOS).long()
    doc = eos.cumsum(1) - eos
    vis = (i[None, :] <= i[:, None])[None] & (doc[:, :, None] == doc[:, None, :])
    if window:
        vis = vis & (i[None, :] > i[:, None] - window)[None]
    s = (qh @ kh.transpose(-1, -2)) * SCALE
    s = torch.where(vis[:, None], s, torch.full_like(s, float("-inf")))
    lse = torch.logsumexp(s, -1)
    pr = torch.softmax(s, -1)
    if p > 0:
        keep = ref._attn_keep(B, HQ, T, p, sd, SITE, q.device)
        pr = pr * keep.to(pr.dtype) / (1.0 - p)
    o = (pr @ vh).transpose(1, 2).reshape(B * T, HQ * D)
    return o, lse


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("window", [0, 6])
def test_ref_docmask_matches_dense_fp64(window, p):
    q, k, v, do = _inputs()
    sd = _seed()
    idx = _rows_idx()
    bounds = ref.doc_bounds(idx, EOS, window)
    o, lse = ref.attn_fwd(q, k, v, B, T, HQ, HKV, SCALE, True, p, sd, SITE, bounds=bounds)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    ro, rlse = _dense(qa, ka, va, idx, window, p, sd)
    assert torch.allclose(o, ro.detach(), atol=1e-12, rtol=1e-10)
    assert torch.allclose(lse.double(), rlse.detach(), atol=1e-5)         # ref returns lse in fp32
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ref.attn_bwd(q, k, v, o, do, rlse.detach(), dq, dk, dv, B, T, HQ, HKV, SCALE, True, p, sd, SITE, bounds=bounds)
    ro.backward(do)
    for name, a, r in (("dq", dq, qa.grad), ("dk", dk, ka.grad), ("dv", dv, va.grad)):
        assert torch.allclose(a, r, atol=1e-10, rtol=1e-8), (name, (a - r).abs().max().item())
    # the mask is really applied
    o_c, _ = ref.attn_fwd(q, k, v, B, T, HQ, HKV, SCALE, True, p, sd, SITE, window=window)
    assert not torch.allclose(o, o_c)
    # the public op takes the same keyword on the CPU path
    fo, flse, _ = F_.attn_fwd(q, k, v, B, T, HQ, HKV, SCALE, True, p, sd, SITE, bounds=bounds)
    assert torch.equal(fo, o) and torch.equal(flse, lse)
    fdq, fdk, fdv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    F_.attn_bwd(q, k, v, o, do, rlse.detach(), None, fdq, fdk, fdv, B, T, HQ, HKV, SCALE, True, p, sd, SITE,
                bounds=bounds)
    assert torch.equal(fdq, dq) and torch.equal(fdk, dk) and torch.equal(fdv, dv)


def test_docmask_refusals():
    q, k, v, do = _inputs()
    sd = _seed()
    g = [torch.empty_like(t) for t in (q, k, v)]
    bounds = ref.doc_bounds(_rows_idx(), EOS)
    lse = torch.zeros(B, HQ, T)
    with pytest.raises(ValueError, match="causal"):
        ref.attn_fwd(q, k, v, B, T, HQ, HKV, SCALE, False, 0.0, sd, SITE, bounds=bounds)
    with pytest.raises(ValueError, match="causal"):
        ref.attn_bwd(q, k, v, q, do, lse, *g, B, T, HQ, HKV, SCALE, False, 0.0, sd, SITE, bounds=bounds)
    with pytest.raises(ValueError, match="causal"):
        F_.attn_fwd(q, k, v, B, T, HQ, HKV, SCALE, False, 0.0, sd, SITE, bounds=bounds)
    with pytest.raises(ValueError, match="causal"):
        F_.attn_bwd(q, k, v, q, do, lse, None, *g, B, T, HQ, HKV, SCALE, False, 0.0, sd, SITE, bounds=bounds)
    with pytest.raises(ValueError, match="either bounds or window"):
        F_.attn_fwd(q, k, v, B, T, HQ, HKV, SCALE, True, 0.0, sd, SITE, window=4, bounds=bounds)
    with pytest.raises(ValueError, match="either bounds or window"):
        ref.attn_bwd(q, k, v, q, do, lse, *g, B, T, HQ, HKV, SCALE, True, 0.0, sd, SITE, window=4, bounds=bounds)
    with pytest.raises(ValueError, match="shape"):
        F_.attn_fwd(q, k, v, B, T, HQ, HKV, SCALE, True, 0.0, sd, SITE, bounds=bounds[:1])
    with pytest.raises(ValueError, match="int32"):
        F_.attn_fwd(q, k, v, B, T, HQ, HKV, SCALE, True, 0.0, sd, SITE, bounds=bounds.long())
    with pytest.raises(ValueError, match="int64"):
        F_.doc_bounds(_rows_idx().int(), EOS)
    with pytest.raises(ValueError, match=">= 0"):
        ref.doc_bounds(_rows_idx(), EOS, -1)


def test_config_validates_doc_eos_id():
    assert get_model_config("M7B", 4096).doc_eos_id is None              # no tier's default changes
    assert get_model_config("mtiny", 32).doc_eos_id is None
    with pytest.raises(ValueError, match="causal"):
        ModelConfig(causal=False, doc_eos_id=3)
    for bad in (-1, 32000, 1.5, True):
        with pytest.raises(ValueError, match="vocab_size"):
            ModelConfig(arch="mistral", causal=True, vocab_size=32000, doc_eos_id=bad)
    cfg = get_model_config("tiny", 32)
    cfg.doc_eos_id = 3
    with pytest.raises(ValueError, match="causal"):
        cfg.validate()
    old = get_model_config("mtiny", 32).to_dict()        # a config saved before the key existed still loads
    del old["doc_eos_id"]
    assert ModelConfig(**old).doc_eos_id is None
    assert ModelConfig(**dict(old, doc_eos_id=255, sliding_window=8)).to_dict()["doc_eos_id"] == 255


def _pair(eos, window=None, T_=32):
    cfg = get_model_config("mtiny", T_)
    cfg.doc_eos_id = eos
    cfg.sliding_window = window
    cfg.validate()
    torch.manual_seed(0)
    m = MistralLM(cfg).double()
    o = OracleMistral(cfg).double()
    o.load_state_dict(m.state_dict())
    return cfg, m, o


def _model_idx(cfg):
    idx = torch.randint(0, 255, (2, 32), generator=torch.Generator().manual_seed(1))
    idx[0, [3, 4, 17]] = 255
    idx[1, [0, 12, 31]] = 255
    return idx


@pytest.mark.parametrize("window", [None, 8])
def test_mistral_docmask_matches_oracle(window):
    """Tolerances of tests/test_attention_window_cpu.py::test_mistral_window_matches_oracle."""
    cfg, m, o = _pair(255, window)
    idx = _model_idx(cfg)
    tgt = idx.roll(-1, 1)
    tgt[1, -5:] = -1
    _, loss = m(idx, tgt)
    _, lo = o(idx, tgt)
    assert torch.allclose(loss, lo, atol=1e-10), (loss.item(), lo.item())
    loss.backward()
    lo.backward()
    got = dict(m.named_parameters())
    for name, p in o.named_parameters():
        assert got[name].grad is not None, name
        assert torch.allclose(got[name].grad, p.grad, atol=1e-9, rtol=1e-7), name
    # the mask is really applied: the same weights without it give another loss
    _, m_full, _ = _pair(None, window)
    _, l_full = m_full(idx, tgt)
    assert abs(l_full.item() - loss.item()) > 1e-6, (l_full.item(), loss.item())


def test_packing_equals_documents_run_alone():
    """RoPE positions are not reset per document: its scores depend on i - j only, so the logits at a document's
    positions in a packed row equal those of the document run on its own (fp64)."""
    cfg, m, _ = _pair(255)
    idx = torch.randint(0, 255, (1, 32), generator=torch.Generator().manual_seed(2))
    idx[0, 12] = 255                      # documents 0 .. 12 and 13 .. 31
    packed, _ = m(idx)
    cfg1, alone, _ = _pair(None)
    alone.load_state_dict(m.state_dict())
    a, _ = alone(idx[:, :13])
    b, _ = alone(idx[:, 13:])
    assert torch.allclose(packed[:, :13], a, atol=1e-10, rtol=1e-9)       # same positions: the same arithmetic
    # positions 13 .. 31 against 0 .. 18: R(i) q . R(j) k = q . R(j - i) k only up to the rounding of the cos / sin
    # tables, which the model keeps in fp32 (2^-24 relative per entry, a few of them per score)
    assert torch.allclose(packed[:, 13:], b, atol=1e-7, rtol=1e-6)
    full, _ = alone(idx)                  # and without the mask the second document does see the first
    assert not torch.allclose(full[:, 13:], b, atol=1e-6)


def test_synthetic_dataset_documents():
    V, Tn, N = 50, 64, 6
    base = SyntheticDataset(V, Tn, size=20, seed=5)
    want = torch.randint(0, V, (20, Tn), generator=torch.Generator().manual_seed(5), dtype=torch.int64)
    assert torch.equal(base.data, want)                                   # the default table is unchanged
    assert base.visible_pairs_per_row() == Tn * (Tn + 1) / 2
    ds = SyntheticDataset(V, Tn, size=20, seed=5, doc_len=N, eos_id=9)
    assert torch.equal(ds.data, SyntheticDataset(V, Tn, size=20, seed=5, doc_len=N, eos_id=9).data)
    assert not torch.equal(ds.data, SyntheticDataset(V, Tn, size=20, seed=6, doc_len=N, eos_id=9).data)
    eos = ds.data == 9
    assert eos[:, -1].all()                                               # a document is cut at the row end
    keep = ~eos & (want != 9)
    assert torch.equal(ds.data[keep], want[keep])                         # the tokens did not move
    assert (ds.data[~eos & (want == 9)] == 10).all()                      # stray EOS -> (eos + 1) % vocab
    pairs = 0
    for r in range(20):
        ends = eos[r].nonzero().flatten().tolist()
        lens = [e - s for s, e in zip([-1] + ends[:-1], ends)]
        assert sum(lens) == Tn and all(1 <= n <= 2 * N - 1 for n in lens)
        pairs += sum(n * (n + 1) // 2 for n in lens)
    assert ds.visible_pairs_per_row() == pairs / 20                       # a direct count
    # the same count from the mask itself, with a window folded in
    b = ref.doc_bounds(ds.data, 9, 4)
    direct = (torch.arange(Tn)[None] - b[0].long() + 1).sum().item() / 20
    assert ds.visible_pairs_per_row(4) == direct
    assert SyntheticDataset(V, Tn, size=4, doc_len=3).eos_id == V - 1
    with pytest.raises(ValueError, match="doc_len"):
        SyntheticDataset(V, Tn, size=4, doc_len=0)
    with pytest.raises(ValueError, match="eos_id"):
        SyntheticDataset(V, Tn, size=4, doc_len=3, eos_id=V)
    with pytest.raises(ValueError, match="doc_len"):
        SyntheticDataset(V, Tn, size=4, eos_id=3)


def test_train_flops_take_measured_pairs():
    T_ = 4096
    cfg = get_model_config("M7B", T_)
    full = cfg.train_flops_per_token(T_)
    assert cfg.train_flops_per_token(T_, None) == full                    # today's number exactly
    L, d = cfg.n_layer, cfg.n_embd
    pairs = 1000.0 * T_
    assert cfg.train_flops_per_token(T_, pairs) == pytest.approx(full - 12 * L * d * (T_ / 2) + 12 * L * d * 1000.0,
                                                                 rel=1e-12)


def _harness_args(tier, res, extra=("--doc-len", "8")):
    return ["--strategy", "ddp", "--tier", tier, "--seq-len", "32", "--steps", "2", "--warmup-steps", "1",
            "--per-device-batch", "1", "--grad-accum", "1", "--results-dir", str(res), "--device", "cpu", *extra]


def test_harness_records_the_documents(tmp_path):
    from dltb.harness import main
    os.environ.pop("WORLD_SIZE", None)
    assert main(_harness_args("mtiny", tmp_path / "res", ("--doc-len", "8", "--sliding-window", "16"))) == 0
    ext = [f for f in os.listdir(tmp_path / "res") if f.endswith(".extended.json")]
    side = json.loads((tmp_path / "res" / ext[0]).read_text())
    assert side["model"]["doc_eos_id"] == 255                             # default: vocab_size - 1
    assert side["data"]["doc_len"] == 8 and side["data"]["eos_id"] == 255
    ds = SyntheticDataset(256, 32, size=1000, seed=42, doc_len=8, eos_id=255)
    frac = ds.visible_pairs_per_row(16) / (32 * 33 / 2)
    assert side["data"]["visible_pair_fraction"] == pytest.approx(frac, rel=1e-12) and 0 < frac < 0.5
    cfg = get_model_config("mtiny", 32)
    assert side["train_flops_per_token"] == pytest.approx(
        cfg.train_flops_per_token(32, ds.visible_pairs_per_row(16)), rel=1e-12)
    assert side["train_flops_per_token"] < cfg.train_flops_per_token(32)
    plain = [f for f in os.listdir(tmp_path / "res") if f.endswith(".json") and not f.endswith(".extended.json")]
    rec = json.loads((tmp_path / "res" / plain[0]).read_text())
    assert "doc_len" not in rec and "doc_eos_id" not in rec and "data" not in rec


@pytest.mark.parametrize("tier,extra,message", [
    ("tiny", ("--doc-len", "8"), "--doc-len needs a causal tier; tier tiny attends non-causally"),
    ("mtiny", ("--doc-len", "0"), "--doc-len must be >= 1"),
    ("mtiny", ("--doc-len", "8", "--eos-id", "256"), "--eos-id must be in [0, 256) for tier mtiny"),
    ("mtiny", ("--doc-len", "8", "--eos-id", "-1"), "--eos-id must be in [0, 256) for tier mtiny"),
    ("mtiny", ("--eos-id", "3"), "--eos-id is only used together with --doc-len"),
])
def test_harness_refuses_bad_document_flags(tmp_path, capsys, tier, extra, message):
    """The harness's own validation, by its message (an unknown flag would also exit with 2)."""
    from dltb.harness import main
    with pytest.raises(SystemExit) as e:
        main(_harness_args(tier, tmp_path / "res", extra))
    assert e.value.code == 2                              # argparse's argument error
    assert message in capsys.readouterr().err
    assert not (tmp_path / "res").exists()
