"""Bias gradients from the window-wide dW products (``bias_from_dw``, parallel/wgrad.py) on the CPU:

* the float64-derived reference of the GPU column-sum test (tests/test_gemm_tn_colsum_gpu.py) stays inside the
  bound that test applies, for its seeds -- as the float64 sum rounded once and as an fp32 sum in either order;
* ``WgradQueue`` writes the bias slots of batched and of single products;
* a 2-layer TinyGPT trains the same with the switch on and off (``model_grads`` is shared with
  tests/test_bias_from_dw_gpu.py).
"""
import pytest
import torch

import dltb  # noqa: F401
from dltb.models.config import ModelConfig
from dltb.models.tinygpt import TinyGPT
from dltb.parallel import engine_config, make_engine
from dltb.parallel.runtime import Unit
from dltb.parallel.wgrad import WgradQueue, strided_rows

from colsum_ref import BOUNDED, bounded_case, colsum64, colsum_bound
from gemm_ref import flagged
from rowwise_ref import half_ulp, round16

BF16, F16 = torch.bfloat16, torch.float16
ACCUM = 2
BIAS_SLOTS = (3, 5, 9, 11)                     # qkv, out-proj, fc1, fc2 bias of a block (param_list order)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("K,M,N,batch", BOUNDED, ids=lambda v: str(v))
def test_reference_of_the_bounded_gpu_test(dtype, K, M, N, batch):
    a, _, prev = bounded_case(dtype, K, M, N, batch)
    want, abs_sum = colsum64(a)
    for w, p in ((want, None), (want + prev.double(), prev)):
        bnd = colsum_bound(w, abs_sum, K, dtype, p)
        assert torch.isfinite(bnd).all() and float(bnd.min()) > 0
        once = round16(w, dtype)                                # the float64 sum, rounded once
        assert float(((once - w).abs() - half_ulp(w, dtype)).max()) <= 0 and flagged(once, w, bnd) == 0
        for order in (a.float(), a.float().flip(-2)):           # fp32 sums, forward and reversed k
            s = torch.zeros(batch, M)
            for k in range(K):
                s = s + order[:, k]
            if p is not None:
                s = s + p.float()
            assert flagged(s.to(dtype), w, bnd) == 0
        # ... and the bound is not vacuous: one dropped token row (|N(0,1)| against a bound of a quarter at the
        # most, at K = 1152 in bf16) is rejected in a good share of the columns
        dropped = round16(w - a[:, K // 2].double(), dtype)
        assert flagged(dropped, w, bnd) > 0.3


def test_strided_rows():
    flat = torch.arange(400.0)
    ts = [flat[100 * i + 7:100 * i + 39] for i in range(4)]
    v = strided_rows(ts)
    assert v.shape == (4, 32) and v.stride() == (100, 1) and all(torch.equal(v[i], t) for i, t in enumerate(ts))
    assert strided_rows([ts[0], ts[2], ts[3]]) is None and strided_rows([ts[1], ts[0]]) is None
    assert strided_rows([flat[0:32], flat[16:48]]) is None      # overlapping
    assert strided_rows([flat[0:32], torch.zeros(32)]) is None  # another storage
    assert strided_rows([flat[0:64:2], flat[100:164:2]]) is None


@pytest.mark.parametrize("layer_strided", [True, False])
@pytest.mark.parametrize("bias_acc", [False, True])
def test_queue_writes_bias_slots(layer_strided, bias_acc):
    torch.manual_seed(0)
    L, T, M, N, gap = 4, 16, 6, 5, 7
    units = [Unit(f"b{i}", [(f"w{i}", torch.nn.Parameter(torch.zeros(M, N)))], i) for i in range(L)]
    step = M * N + M + gap
    grad = torch.randn(L * step)
    before = grad.clone()
    dws = [grad[i * step:i * step + M * N].view(M, N) for i in range(L)]
    dbs = [grad[i * step + M * N:i * step + M * N + M] for i in range(L)]
    if layer_strided:
        dyb, xb = torch.randn(L, T, M), torch.randn(L, T, N)
        dys, xs = list(dyb), list(xb)
    else:
        dys, xs = [torch.randn(T, M) for _ in range(L)], [torch.randn(T, N) for _ in range(L)]
    q = WgradQueue()
    for i in reversed(range(L)):
        q.add(units[i], 0, dys[i], xs[i], dws[i], False, (dbs[i], bias_acc))
    q.flush()
    assert (q.batched_calls, q.single_calls) == ((1, 0) if layer_strided else (0, L))
    for i in range(L):
        assert torch.allclose(dws[i], dys[i].t() @ xs[i], atol=1e-5)
        old = before[i * step + M * N:i * step + M * N + M]
        assert torch.allclose(dbs[i], dys[i].sum(0) + (old if bias_acc else 0), atol=1e-5)
        assert torch.equal(grad[i * step + M * N + M:(i + 1) * step], before[i * step + M * N + M:(i + 1) * step])


def model_grads(device, on):
    """(losses, flat gradient, flat gradient after the first micro-step, bias mask, engine) of one accumulation
    window of a 2-layer TinyGPT at d = 256, T = 128, accum = 2 with dropout, fixed seeds; ``on``: the
    bias_from_dw switch."""
    torch.manual_seed(0)
    cfg = ModelConfig(vocab_size=512, n_embd=256, n_head=4, n_layer=2, block_size=128, dropout=0.1)
    model = TinyGPT(cfg)
    ecfg = engine_config("zero2", ACCUM, "reference")
    ecfg.extra["bias_from_dw"] = on
    eng = make_engine(model, ecfg, device)
    assert eng._window_wgrad and eng.bias_from_dw == on
    eng.train()
    g = torch.Generator().manual_seed(1)
    losses = []
    for m in range(ACCUM):
        idx = torch.randint(0, cfg.vocab_size, (2, 128), generator=g).to(device)
        loss = eng(idx, idx)[1]
        eng.backward(loss)
        losses.append(float(loss.detach()))
        if m + 1 < ACCUM:
            first = eng.flat_grad.detach().clone().cpu()
            eng.step()                         # (the window's last step would run the optimizer)
    assert eng.is_boundary
    grad = eng.flat_grad.detach().clone()
    mask = torch.zeros(grad.numel(), dtype=torch.bool)
    for u in model.unit_blocks:
        for j in BIAS_SLOTS:
            s = eng.layout.slot(u, j)
            assert len(s.shape) == 1
            mask[s.offset:s.offset + s.numel] = True
    assert int(mask.sum()) == cfg.n_layer * 9 * cfg.n_embd
    return losses, grad.cpu(), first, mask, eng


def window_colsums(eng, dtype):
    """float64 column sums (and sums of magnitudes) of the window's dY operands in the model's layer buffers,
    laid out like the flat gradient's bias slots, with the bound of tests/colsum_ref.py around them."""
    model, lb = eng.model, eng.model._lbufs
    want = torch.zeros(eng.flat_grad.numel(), dtype=torch.float64)
    bnd = torch.zeros_like(want)
    for i, u in enumerate(model.unit_blocks):
        r = model.cfg.n_layer - 1 - i if eng.wgrad_rows_reversed else i
        for j, buf in zip(BIAS_SLOTS, (lb.dqkv, lb.dx1, lb.df, lb.dm)):
            s = eng.layout.slot(u, j)
            w, a = colsum64(buf[r].cpu())
            want[s.offset:s.offset + s.numel] = w
            bnd[s.offset:s.offset + s.numel] = colsum_bound(w, a, buf.shape[1], dtype)
    return want, bnd


def compare_model(device):
    """Switch on against off.  Losses and every gradient but the four bias gradients of a block: identical (the
    forward and every other backward kernel see the same inputs).  The bias gradients sum the same 16-bit dY
    values in fp32 either way; off rounds the slot once per micro-step (accum = 2 roundings: r0 = round(s0), then
    round(r0 + s1)), on rounds the window's sum once.  Each rounding moves the value it rounds by at most half an
    ulp of THAT value, so the two differ by at most (accum + 1) / 2 = 1.5 ulps plus the fp32 summation-order
    noise (K 2^-24 relative to the summed magnitudes, K = 512 tokens: 2^-15, a small fraction of a bf16 ulp):
    2 bf16 ulps of the larger magnitude among the values that were rounded -- on, off and off's slot after the
    first micro-step, r0.  r0 belongs in it: where s1 cancels s0 the result is small and carries r0's rounding
    error.  Measured on the GPU with the magnitude taken from the two results alone: 71 of 4608 elements above
    2 ulps, the worst at 147.6 -- all of it off's first rounding, as the float64 check of the on arm shows
    (every element within half an ulp plus the fp32 bound of the float64 column sums of the window's dY)."""
    l_on, g_on, _, mask, eng = model_grads(device, True)
    # (the CPU engine keeps fp32 slots: the bf16 bound holds all the more)
    want, bnd = window_colsums(eng, g_on.dtype if g_on.dtype in (BF16, F16) else BF16)
    l_off, g_off, first_off, mask_off, _ = model_grads(device, False)
    assert torch.equal(mask, mask_off)
    assert l_on == l_off, (l_on, l_off)
    rest_on, rest_off = g_on[~mask], g_off[~mask]
    assert torch.isfinite(g_on).all() and float(rest_on.abs().max()) > 0
    assert torch.equal(rest_on, rest_off), f"{int((rest_on != rest_off).sum())} weight-gradient elements differ"
    b_on, b_off, b_first = g_on[mask].double(), g_off[mask].double(), first_off[mask].double()
    assert float(b_on.abs().max()) > 0
    assert flagged(b_on, want[mask], bnd[mask]) == 0, "on: outside the float64 bound of the window's column sums"
    narrow = (b_on - b_off).abs() / (2 * half_ulp(torch.maximum(b_on.abs(), b_off.abs()), BF16))
    print(f"bias gradients on vs off ({device}), in bf16 ulps of the larger of the two results: worst "
          f"{float(narrow.max()):.3f}, {int((narrow > 2).sum())} of {narrow.numel()} above 2, "
          f"{int((b_on != b_off).sum())} differ at all")
    big = torch.maximum(torch.maximum(b_on.abs(), b_off.abs()), b_first.abs())
    ratio = (b_on - b_off).abs() / (2 * half_ulp(big, BF16))
    print(f"... of the largest rounded magnitude (with off's first micro-step): worst {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 2.0
    return eng


def test_model_bias_from_dw_cpu():
    compare_model("cpu")
