"""The chunked LM head (``--head-chunk N``) on the MI355X: the two new kernels of csrc/xent.hip against the fused
kernel and the fp32 reference, the bf16 Mistral-shape model with the head in row chunks against the unchunked head,
the bytes the head no longer holds, HIP-graph replay, and two host-staged ranks."""
import copy

import pytest
import torch

import dltb
from dltb.models import build_model, get_model_config
from dltb.ops import functional as F_
from dltb.ops import ref
from dltb.ops._ext import ext
from dltb.parallel import GraphedStep, ParamRuntime, engine_config, make_engine
from multirank_util import compare, run
from test_head_chunk_cpu import _head_ctx
from test_kernels_gpu import close

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
EPS16 = 2.0 ** -9


# ------------------------------------------------------------------------------------------- kernels
# V = 8: one vector per row; 256: half a wave of a 512-thread row; 4096: exactly one vector per thread; 32000: the
# real vocabulary, 4000 vectors = 7.8 per thread (a partly filled last pass); 131072: the largest row the kernels
# take (32 vectors per thread).  70 rows: no multiple of anything
def _logits(N, V, dtype, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed + V)
    z = (torch.randn(N, V, device="cuda", generator=g) * 2.0).to(dtype)
    if N > 5:
        z[5] = 80.0
        z[5, 1::2] = -80.0                                  # one row of +-80
    t = torch.randint(0, V, (N,), device="cuda", generator=g)
    t[::7] = -1
    if N > 2:
        t[1], t[2] = 0, V - 1
    return z, t


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("V", [8, 256, 4096, 32000, 131072])
def test_xent_lse(V, dtype):
    z, t = _logits(70, V, dtype)
    keep = z.clone()
    loss, lse = F_.xent_lse(z, t, -1)
    assert loss.dtype == lse.dtype == torch.float32 and loss.shape == lse.shape == (70,)
    assert torch.equal(z, keep)                             # the logits are only read
    fused = ext().xent_fwd_bwd_(keep.clone(), t, -1)
    assert torch.equal(loss, fused)                         # the fused kernel's loss rows, bit for bit
    assert (loss[t == -1] == 0).all()
    close(lse, torch.logsumexp(keep.double(), -1), 1e-3, 1e-3, "lse")
    # into slices of longer rows, as the model calls it: nothing beside the slices is written
    lo = torch.full((100,), 7.0, device="cuda")
    ls = torch.full((100,), 7.0, device="cuda")
    F_.xent_lse(z, t, -1, loss_out=lo[16:86], lse_out=ls[16:86])
    assert torch.equal(lo[16:86], loss) and torch.equal(ls[16:86], lse)
    for buf in (lo, ls):
        assert (buf[:16] == 7.0).all() and (buf[86:] == 7.0).all()


# the grid runs over 16-byte vectors: (3, 131072) is 49152 vectors in 192 workgroups of which rows start inside a
# workgroup only at multiples of 64; (2048, 256) has 8 rows per workgroup; (70, 8) 70 vectors in one workgroup;
# (70, 32000) rows of 4000 vectors that start anywhere inside a workgroup
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("N,V", [(70, 8), (70, 256), (70, 4096), (70, 32000), (70, 131072), (3, 131072), (2048, 256)])
def test_xent_bwd_lse(N, V, dtype):
    z, t = _logits(N, V, dtype, seed=1)
    want = z.clone()
    ref.xent_fwd_bwd_(want, t, -1)
    _, lse = F_.xent_lse(z, t, -1)
    guard = torch.full((N + 2, V), 3.0, device="cuda", dtype=dtype)
    guard[1:N + 1] = z
    got = F_.xent_bwd_lse_(guard[1:N + 1], t, lse, -1)
    assert got.data_ptr() == guard[1].data_ptr()
    close(got, want, 1e-4, 2e-2, "dlogits")
    assert (got[t == -1] == 0).all()                        # ignored rows are exactly 0
    assert (guard[0] == 3.0).all() and (guard[N + 1] == 3.0).all()      # the rows around the chunk are untouched


def test_new_xent_ops_refuse_bad_operands():
    C = ext()
    z, t = _logits(8, 64, torch.bfloat16)
    _, lse = C.xent_lse(z, t, -1)
    with pytest.raises(RuntimeError):
        C.xent_lse(z[:, :60], t, -1)                        # not contiguous
    with pytest.raises(RuntimeError):
        C.xent_lse(z, t[:7], -1)
    with pytest.raises(RuntimeError):
        C.xent_lse(z, t, -1, torch.empty(7, device="cuda"))
    with pytest.raises(RuntimeError):
        C.xent_lse(torch.zeros(8, 12, device="cuda", dtype=torch.bfloat16), t, -1)      # V % 8
    with pytest.raises(RuntimeError):
        C.xent_bwd_lse_(z, t, lse[:7], -1)
    with pytest.raises(RuntimeError):
        C.xent_bwd_lse_(z, t, lse.double(), -1)
    with pytest.raises(RuntimeError):
        C.xent_bwd_lse_(z, t.int(), lse, -1)


# ------------------------------------------------------------------------------------------- model
def _cfg(vocab=None, layers=2, T=256):
    cfg = get_model_config("mtiny", T)
    cfg.n_layer = layers
    if vocab is not None:
        cfg.vocab_size = vocab
    return cfg


class _Runs:
    """One initialisation per shape; every run starts from a copy of it and runs once."""

    def __init__(self):
        self.cache = {}

    def get(self, vocab, B, chunk):
        key = (vocab, B, chunk)
        if key in self.cache:
            return self.cache[key]
        if ("base", vocab) not in self.cache:
            torch.manual_seed(0)
            self.cache[("base", vocab)] = build_model(_cfg(vocab)).to("cuda", torch.bfloat16)
        cfg = _cfg(vocab)
        m = copy.deepcopy(self.cache[("base", vocab)])
        m.rt = ParamRuntime()
        m.head_chunk = chunk
        g = torch.Generator().manual_seed(3)
        idx = torch.randint(0, cfg.vocab_size, (B, 256), generator=g).cuda()
        tgt = idx.roll(-1, 1).clone()
        tgt[:, ::9] = -1
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


def _head64(r, bounds):
    """float64 loss of the head on the run's own input, and the head's weight gradient summed over the rows
    before each boundary (the running sum the chunked backward holds after that chunk)."""
    m = r["model"]
    x = r["x"].double()
    wn = m.model.norm.weight.detach().double()
    wh = m.lm_head.weight.detach().double().requires_grad_()
    h = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + m.cfg.norm_eps) * wn
    rows = torch.nn.functional.cross_entropy(h @ wh.t(), r["tgt"], ignore_index=-1, reduction="none")
    count = (r["tgt"] != -1).sum().clamp(min=1)
    partial = [torch.autograd.grad(rows[:r1].sum() / count, wh, retain_graph=True)[0] for r1 in bounds]
    return (rows.sum() / count).detach(), partial


def _check_against_unchunked(runs, vocab, B, chunk):
    off, chk = runs.get(vocab, B, None), runs.get(vocab, B, chunk)
    R, V = B * 256, _cfg(vocab).vocab_size
    assert off["saved"].count(R * V) == 1 and R * V not in chk["saved"]
    assert torch.equal(off["x"], chk["x"]) and torch.equal(off["h"], chk["h"])
    w = chk["model"].lm_head.weight.detach()
    full = F_.linear_fwd(chk["h"], w)
    tg = chk["tgt"]
    parts = [F_.linear_fwd(chk["h"][r0:r0 + chunk], w) for r0 in range(0, R, chunk)]
    rows_equal = torch.equal(torch.cat(parts), full)
    bounds = list(range(chunk, R, chunk)) + [R]
    loss64, partial = _head64(chk, bounds)
    e_u, e_c = (abs(r["loss"].double() - loss64).item() for r in (off, chk))
    print(f"V {V} R {R} chunk {chunk}: chunk product rows bit-equal to the full product's: {rows_equal}; "
          f"loss error vs float64 unchunked {e_u:.3e} chunked {e_c:.3e}")
    if rows_equal:
        mine = torch.cat([F_.xent_lse(p, tg[i * chunk:(i + 1) * chunk], -1)[0] for i, p in enumerate(parts)])
        assert torch.equal(mine, F_.xent_fwd_bwd_(full.clone(), tg, -1))
        assert torch.equal(chk["loss"], off["loss"])
    else:
        assert e_c <= e_u + EPS16 * abs(loss64.item())
    slack = (EPS16 * sum(p.abs() for p in partial)).max().item()
    e_u, e_c = ((r["dW"].double() - partial[-1]).abs().max().item() for r in (off, chk))
    print(f"V {V} R {R} chunk {chunk}: head dW max error vs float64 unchunked {e_u:.3e} chunked {e_c:.3e} "
          f"slack {slack:.3e}")
    assert e_c <= e_u + slack
    for n, g in chk["grads"].items():
        assert g is not None and torch.isfinite(g.float()).all(), n


@pytest.mark.parametrize("chunk", [128, 384])
def test_model_chunked_head_bf16(runs, chunk):
    """mtiny in bf16, R = 512 rows, 4 chunks of 128 and a ragged 384 + 128.  Where the chunk product's rows carry
    the full product's bits the loss must be the unchunked loss bit for bit; otherwise it is held to the float64
    bound of tests/test_head_chunk_cpu.py with bf16's 2^-9.  The head's weight gradient is held to that bound
    either way: one more rounding per accumulated chunk.  Observed on the MI355X: the rows are bit-equal at both
    chunk sizes (and at V = 32000 in chunks of 64), so the bit-for-bit branch runs; the case taken is printed."""
    _check_against_unchunked(runs, None, 2, chunk)


def test_model_chunked_head_real_vocabulary(runs):
    """V = 32000 (4000 vectors per row: the kernels' partly filled last pass, rows that start inside a workgroup of
    the backward's grid), R = 256 in chunks of 64, end to end."""
    _check_against_unchunked(runs, 32000, 1, 64)


# ------------------------------------------------------------------------------------------- memory
def _memory(model, idx, tgt, chunk):
    """tests/test_recompute_gpu.py::_memory, with the targets held by the caller as the harness holds them: the
    chunked head keeps a view of them for its backward, the unchunked head has folded them into dlogits."""
    model.head_chunk = chunk
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    _, loss = model(idx, tgt)
    after_fwd = torch.cuda.memory_allocated() - base
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del loss
    return after_fwd, peak


def test_head_memory():
    torch.manual_seed(0)
    cfg = _cfg(4096, layers=1)
    model = build_model(cfg).to("cuda", torch.bfloat16)
    model.rt = ParamRuntime()
    R, N, V, d = 1024, 128, cfg.vocab_size, cfg.n_embd
    idx = torch.randint(0, V, (4, 256), device="cuda")
    tgt = idx.roll(-1, 1)
    _memory(model, idx, tgt, None)              # the first step allocates what stays: gradients, RoPE tables
    _memory(model, idx, tgt, N)
    fwd_off, peak_off = _memory(model, idx, tgt, None)
    fwd_chk, peak_chk = _memory(model, idx, tgt, N)
    print(f"after forward: off {fwd_off} chunked {fwd_chk}; peak: off {peak_off} chunked {peak_chk}")
    # the saving is the logits; the chunked head keeps the fp32 log-sum-exp rows instead
    assert fwd_off - fwd_chk >= R * V * 2 - 4 * R, (fwd_off, fwd_chk)
    # what the chunked backward newly holds at its peak, beside one chunk of logits
    new = {"lse [R] fp32": 4 * R,
           "dh of one chunk [N, d], copied into the assembled dh": N * d * 2}
    assert peak_off - peak_chk >= (R - N) * V * 2 - sum(new.values()), (peak_off, peak_chk, new)


# ------------------------------------------------------------------------------------------- graphs
def _engine_run(graphed, chunk):
    """tests/test_graphs_gpu.py::test_graph_replay_mistral's run: accumulation windows of 4 micro-steps, the
    first eager, the second captured, the last two replayed with new batches."""
    torch.manual_seed(0)
    cfg = _cfg()
    with torch.device("cuda"):
        model = build_model(cfg)
    model.head_chunk = chunk
    eng = make_engine(model, engine_config("zero3", 4, "reference"), "cuda:0")
    eng.train()
    g = torch.Generator(device="cuda").manual_seed(1)
    runner = GraphedStep(eng) if graphed else None
    losses = []
    for _ in range(16):
        idx = torch.randint(0, cfg.vocab_size, (1, 256), device="cuda", generator=g)
        if runner is None:
            loss = eng(idx, idx)[1]
            eng.backward(loss)
            eng.step()
        else:
            loss = runner(idx, idx)
        losses.append(loss.item())
    if runner is not None:
        assert len(runner.graphs) == eng.accum
    return losses, eng.full_state_dict()


def test_graph_replay_chunked_head():
    l0, s0 = _engine_run(False, 128)
    l1, s1 = _engine_run(True, 128)
    assert l0 == l1, (l0, l1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k


# ------------------------------------------------------------------------------------------- two ranks
def test_world2_host_staged_chunked_head(tmp_path):
    """Two ranks on one GPU (gloo, host-staged buffers), the Mistral-shape model under ZeRO-3: each rank's head
    sees 256 rows in two chunks.  Against the same case without the flag, at tests/test_multirank_gpu.py's
    tolerance."""
    args = ("--cases", "zero3_mistral", "--windows", "2")
    env = {"DLTB_COMM": "host"}
    off = run(tmp_path / "off.pt", 2, "cuda", extra=args, env_extra=env, timeout=300)
    chk = run(tmp_path / "chunk.pt", 2, "cuda", extra=args + ("--head-chunk", "128"), env_extra=env, timeout=300)
    assert set(off) == set(chk) == {"zero3_mistral"}
    bad = compare(off, chk, loss_tol=1e-3, upd_tol=0.02, cos_min=0.9998, param_tol=0.03)
    assert not bad, bad
