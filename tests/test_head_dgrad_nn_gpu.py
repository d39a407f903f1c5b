"""The NN-layout MFMA GEMM (csrc/gemm_nn.hip) and the tied head's data gradient that runs on it.

``gemm_nn`` computes alpha * a b for a [M, K] (K-contiguous) and b [K, N] (N-contiguous) in bf16 and
fp16: against fp32 torch products on shapes that exercise a single k-step (shorter than the LDS
ring), uneven split-K, several blocks and strided operand views; bitwise on small integers (a
dropped or doubled k-slice, or A and B fragments pairing different k, cannot hide in a tolerance);
then ``head_dgrad`` must take the kernel wherever the engine has no cached W^T or the step is fp16,
eagerly, from a captured graph and inside an FSDP / fp16 DDP engine step."""
import warnings

import pytest
import torch

import dltb  # noqa: F401
from dltb.models import build_model, get_model_config
from dltb.ops import functional as F_
from dltb.ops._ext import ext
from dltb.parallel import engine_config, make_engine

pytestmark = pytest.mark.gpu
BF, FP = torch.bfloat16, torch.float16
CFGS = {0: (128, 128), 1: (256, 128), 2: (64, 64)}      # gemm_nn tile configs
G = 0.37


def rnd(*s, dtype=BF):
    return (torch.randn(*s, device="cuda") * 0.5).to(dtype)


def check(got, want, what):          # the project's tolerance for these products (test_blaslt_gpu.check)
    err = (got.float() - want).abs().max().item()
    tol = 2e-2 * want.abs().max().item() + 1e-2
    assert err <= tol, f"{what}: max err {err} > {tol}"


def views(M, N, K, dtype):
    """a: a column slice of a wider buffer (row stride K + 72), b: a row-strided view (row stride N + 64)."""
    a = rnd(M, K + 72, dtype=dtype)[:, 8:8 + K]
    b = rnd(K, N + 64, dtype=dtype)[:, 64:]
    assert a.stride(0) != K and b.stride(0) > N and a.shape == (M, K) and b.shape == (K, N)
    return a, b


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("M, N, K, splits", [(256, 128, 64, 1), (256, 256, 320, 2), (512, 256, 1024, 4),
                                              (192, 320, 256, 1)])
def test_gemm_nn_matches_fp32(dtype, M, N, K, splits):
    C = ext()
    torch.manual_seed(M + N + K)
    a, b = views(M, N, K, dtype)
    alpha = torch.tensor([G], device="cuda")
    want = a.float() @ b.float()
    ran = 0
    for cfg, (bm, bn) in CFGS.items():
        ok = M % bm == 0 and N % bn == 0
        assert C.gemm_nn_supported(M, N, K, cfg) == ok
        if not ok:
            continue
        what = f"{M}x{N}x{K} cfg {cfg} splits {splits}"
        check(C.gemm_nn(a, b, splits=splits, cfg=cfg), want, what)
        got = C.gemm_nn(a, b, splits=splits, cfg=cfg, alpha=alpha)
        assert got.dtype == dtype and got.shape == (M, N)
        check(got, want * G, what + " alpha")
        buf = torch.zeros(M, N + 8, device="cuda", dtype=dtype)
        out = buf[:, :N]
        assert C.gemm_nn(a, b, out=out, splits=splits, cfg=cfg, alpha=alpha).data_ptr() == out.data_ptr()
        assert torch.equal(out, got), what + " out="
        assert not buf[:, N:].any(), what + " wrote past the row"
        ran += 1
    assert ran >= 1
    if (M, N) == (192, 320):
        assert ran == 1          # only the 64 x 64 config divides it


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("splits", [1, 3])
def test_gemm_nn_exact_on_small_integers(dtype, splits):
    """Entries in {-1, 0, 1}, K = 192, alpha = 0.5: every result is a multiple of 0.5 of magnitude
    <= 96, exact in fp32 partials and in both 16-bit formats, so the kernel must equal the fp32
    product bit for bit, with one k-step per split and with all three in one."""
    C = ext()
    gen = torch.Generator(device="cuda").manual_seed(5)
    M, N, K = 256, 128, 192
    a = torch.randint(-1, 2, (M, K), device="cuda", generator=gen).to(dtype)
    b = torch.randint(-1, 2, (K, N), device="cuda", generator=gen).to(dtype)
    want = ((a.float() @ b.float()) * 0.5).to(dtype)
    alpha = torch.tensor([0.5], device="cuda")
    for cfg in CFGS:
        got = C.gemm_nn(a, b, splits=splits, cfg=cfg, alpha=alpha)
        assert torch.equal(got, want), f"cfg {cfg}: {(got.float() - want.float()).abs().max().item()}"


def test_gemm_nn_refuses_mixed_formats_and_bad_shapes():
    C = ext()
    a, b = rnd(256, 128), rnd(128, 128)
    with pytest.raises(RuntimeError, match="all be bf16 or all fp16"):
        C.gemm_nn(a, b.to(FP))
    with pytest.raises(RuntimeError, match="all be bf16 or all fp16"):
        C.gemm_nn(a, b, out=torch.empty(256, 128, device="cuda", dtype=FP))
    assert not C.gemm_nn_supported(200, 128, 128, 0) and not C.gemm_nn_supported(256, 128, 96, 0)
    assert not C.gemm_nn_supported(128, 128, 128, 1) and not C.gemm_nn_supported(256, 128, 128, 3)
    with pytest.raises(RuntimeError, match="not supported"):
        C.gemm_nn(rnd(200, 128), b)
    with pytest.raises(RuntimeError, match="not supported"):
        C.gemm_nn(rnd(256, 96), rnd(96, 128))
    with pytest.raises(RuntimeError, match="K mismatch"):
        C.gemm_nn(a, rnd(64, 128))
    with pytest.raises(RuntimeError, match="inner dim contiguous"):
        C.gemm_nn(a, rnd(128, 128).t())
    with pytest.raises(RuntimeError, match="row strides"):
        C.gemm_nn(rnd(256, 132)[:, :128], b)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        C.gemm_nn(rnd(256, 144)[:, 4:132], b)


# ----------------------------------------------------------------------------- head_dgrad dispatch
@pytest.fixture(scope="module")
def head():
    """TinyGPT-A's head at 2048 tokens, both formats from the same values; fp32 references computed once."""
    torch.manual_seed(0)
    dl, w = rnd(2048, 32000), rnd(32000, 1024)
    ops = {BF: (dl, w), FP: (dl.to(FP), w.to(FP))}
    want = {dt: (a.float() @ b.float()) * G for dt, (a, b) in ops.items()}
    return ops, want, torch.tensor([G], device="cuda")


class counted:
    """F_.torch_fallbacks emptied for the block and restored after it; warnings are recorded."""

    def __enter__(self):
        self.saved = dict(F_.torch_fallbacks)
        F_.torch_fallbacks.clear()
        self.w = warnings.catch_warnings(record=True)
        self.caught = self.w.__enter__()
        warnings.simplefilter("always")
        return self

    def __exit__(self, *exc):
        self.w.__exit__(*exc)
        F_.torch_fallbacks.clear()
        F_.torch_fallbacks.update(self.saved)

    def fell_back(self):
        return F_.torch_fallbacks.get("head_dgrad"), [str(w.message) for w in self.caught if "head_dgrad" in str(w.message)]


@pytest.mark.parametrize("dtype, with_wt", [(BF, False), (FP, False), (FP, True)],
                         ids=["bf16", "fp16", "fp16_wt"])
def test_head_dgrad_takes_the_nn_kernel(head, dtype, with_wt):
    ops, want, g = head
    dl, w = ops[dtype]
    wt = w.t().contiguous() if with_wt else None
    with counted() as c:
        got = F_.head_dgrad(dl, w, wt, g)
        assert c.fell_back() == (None, [])
    assert got.dtype == dtype
    check(got, want[dtype], "head_dgrad 2048 x 32000 x 1024")


def test_head_dgrad_512_tokens_and_switch(head):
    """The 512-token head (another tile / split choice) takes the kernel too; own_head_nn = False
    restores the counted torch product."""
    ops, want, g = head
    dl, w = ops[BF][0][:512], ops[BF][1]
    with counted() as c:
        got = F_.head_dgrad(dl, w, None, g)
        assert c.fell_back() == (None, [])
        check(got, want[BF][:512], "head_dgrad 512 x 32000 x 1024")
        F_.own_head_nn = False
        try:
            ref = F_.head_dgrad(dl, w, None, g)
        finally:
            F_.own_head_nn = True
        n, msgs = c.fell_back()
        assert n == 1 and len(msgs) == 1
        check(ref, want[BF][:512], "torch product")
        # a layout the kernel does not take goes back to the fallback instead of raising
        F_.head_dgrad(dl, ops[BF][1].t().contiguous().t(), None, g)
        assert c.fell_back()[0] == 2


def test_head_dgrad_replays_from_a_graph(head):
    ops, _, g = head
    dl, w = ops[BF]
    eager = F_.head_dgrad(dl, w, None, g)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F_.head_dgrad(dl, w, None, g)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        y = F_.head_dgrad(dl, w, None, g)
    y.zero_()
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)


# ----------------------------------------------------------------------------- engine level
def _engine(which, cfg):
    model = build_model(cfg)
    if which == "fsdp":
        return make_engine(model, engine_config("fsdp", 2, "reference"), "cuda:0")
    # the fp16 DDP engine of `harness.py --strategy ddp --dtype auto`
    from dltb.comm.topology import recommend_bucket_mb
    from dltb.harness import _engine_for, build_parser
    args = build_parser().parse_args(["--strategy", "ddp", "--tier", "A", "--seq-len", "512", "--steps", "3",
                                      "--per-device-batch", "1", "--grad-accum", "2", "--results-dir", "unused"])
    assert args.dtype == "auto"
    args.dtype, args.grad_comm_dtype, args.bucket_mb = "fp16", "fp32", recommend_bucket_mb(1)
    eng = _engine_for(args, model, torch.device("cuda:0"))[0]
    assert eng.compute_dtype == FP
    return eng


@pytest.mark.parametrize("which", ["fsdp", "ddp_fp16"])
@pytest.mark.parametrize("strict", [False, True], ids=["counted", "strict"])
def test_engine_steps_without_head_fallback(which, strict):
    torch.manual_seed(0)
    cfg = get_model_config("A", 512, dropout=0.1)
    cfg.n_layer = 2
    eng = _engine(which, cfg)
    eng.train()
    idx = torch.randint(0, cfg.vocab_size, (1, 512), device="cuda")
    losses = []
    F_.strict_kernels = strict
    try:
        with counted() as c:
            for _ in range(6):                 # 3 optimizer steps of 2 micro-steps
                loss = eng(idx, idx)[1]
                eng.backward(loss)
                eng.step()
                losses.append(loss.item())
            assert c.fell_back() == (None, [])
    finally:
        F_.strict_kernels = False
    assert all(l == l for l in losses)
    assert losses[-1] < losses[0], losses      # memorising one batch must reduce the loss
