"""Block-scaled FP8 AdamW moments on the GPU: ``adamw_fp8_kernel`` and the quantiser / decoder bindings against the
contract of ``ops/ref.py`` (tests/test_adamw_fp8_cpu.py checks that contract itself).

Segments of 4, 252, 260, 4096 and 4356 elements at owner starts 12, 16, 268, 528 and 4624 (4-aligned, none
256-aligned): a single lane, a partial block, one block plus one lane, one full row, a row plus a partial block.
"""
import json
import math

import pytest
import torch

import dltb  # noqa: F401
from dltb.models import build_model, get_model_config
from dltb.ops import ref
from dltb.ops._ext import ext
from dltb.optim.adamw import FlatAdamW
from dltb.parallel import engine_config, make_engine
from multirank_util import compare, report, run
from test_adamw_fp8_cpu import inputs, neighbours

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 42
LENS = (4, 252, 260, 4096, 4356)
STARTS = (12, 16, 268, 528, 4624)
N = 4624 + 4356 + 20
LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 0.01


@pytest.mark.parametrize("name", list(inputs()))
@pytest.mark.parametrize("kind", [ref.FP8_KIND_M, ref.FP8_KIND_S])
def test_quantiser_bit_exact(name, kind):
    x = inputs()[name]
    if kind == ref.FP8_KIND_S:
        x = x.abs()
    for counter, off, nearest in ((3, 8, False), (2 ** 31 - 1, 2 ** 33 + 12, False), (0, 0, True)):
        want_c, want_s = ref.fp8_quantize(x, kind, SEED, counter, off, "nearest" if nearest else "stochastic")
        got_c, got_s = ext().fp8_quantize(x.to(DEV), kind, SEED, counter, off, nearest)
        assert torch.equal(got_s.cpu(), want_s), (name, kind, counter)
        diff = got_c.cpu() != want_c
        assert not diff.any(), (name, kind, counter, int(diff.sum()), x[diff][:4], got_c.cpu()[diff][:4], want_c[diff][:4])
        assert torch.equal(ext().fp8_dequantize(got_c, got_s).cpu(), ref.fp8_dequantize(want_c, want_s))


def _segments(dst):
    return [(s, n, dst[s:s + n]) for s, n in zip(STARTS, LENS)]


def _fresh(dst_dtype=torch.bfloat16, seed=SEED, sub_group=0, state="fp8", gen_seed=1):
    """An optimizer whose state is the nearest-rounded image of random moments (so it starts from decodable values).
    The moments are an Adam state's: per element one gradient scale over 4 decades, |m| <= about 2 sqrt(v).  The
    master bound of the whole-step test (1e-6 + 1e-5 |p|, tests/test_kernels_gpu.py) is relative to p, not to the
    update: it presumes updates of the size that test has (lr times a few).  Independent m and v would give
    |m| / sqrt(v) of 1e3 and more, updates far larger than p, and the fp32 rounding of such an update alone
    (2^-24 |update| per operation, in adamw_kernel just the same) is past that bound."""
    g = torch.Generator().manual_seed(gen_seed)
    p0 = torch.randn(N, generator=g)
    scale = 10.0 ** (torch.rand(N, generator=g) * 4.0 - 3.0)
    m0 = torch.randn(N, generator=g) * scale
    v0 = ((0.5 + torch.randn(N, generator=g).abs()) * scale) ** 2
    dst = torch.zeros(N, dtype=dst_dtype, device=DEV)
    opt = FlatAdamW(p0.to(DEV), _segments(dst), lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, sub_group=sub_group,
                    state=state, seed=seed)
    opt.load_state_dict({"step": 0, "master": p0, "exp_avg": m0, "exp_avg_sq": v0})
    return opt, dst


def _mask():
    m = torch.zeros(N, dtype=torch.bool)
    for s, n in zip(STARTS, LENS):
        m[s:s + n] = True
    return m


def _scale_of(opt, which):
    """Per-element scale over the owner space (1 outside the segments)."""
    out = torch.ones(N, dtype=torch.float64)
    for i, (s, n) in enumerate(zip(STARTS, LENS)):
        sc = opt._seg_scales(i)[which].cpu().double()
        out[s:s + n] = sc.repeat_interleave(256)[:n]
    return out


def _within_one_quantum(dec, want, scale, floor, what):
    """|dec - want| <= the E4M3 quantum of ``want`` at its block's scale (the floor code allowed for s)."""
    t = (want.abs() / scale).clamp(max=448.0).float()
    lo, hi = neighbours(t)
    quantum = (hi - lo).double().clamp(min=2.0 ** -9) * scale
    ok = (dec.double() - want).abs() <= quantum
    if floor:
        ok |= (dec.double() == scale * 2.0 ** -9) & (want.abs() <= scale * 2.0 ** -9)
    assert bool(ok.all()), (what, int((~ok).sum()), dec[~ok][:4], want[~ok][:4], scale[~ok][:4])


@pytest.mark.parametrize("dst_dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("grad16", [True, False], ids=["g16", "g32"])
@pytest.mark.parametrize("with_gscale", [False, True], ids=["nogs", "gs"])
def test_whole_step_against_float64(dst_dtype, grad16, with_gscale):
    """3 steps; each from the decoded state before it: master and the 16-bit copy against float64 at the bounds of
    tests/test_kernels_gpu.py's AdamW-against-torch test (1e-6 + 1e-5 rel, 1e-2 + 1e-2 rel), every decoded moment
    within one quantum of its float64 value."""
    opt, dst = _fresh(dst_dtype)
    inside = _mask()
    gs = torch.tensor([0.37], device=DEV) if with_gscale else None
    gen = torch.Generator().manual_seed(17)
    for step in range(1, 4):
        sd = opt.state_dict()
        p, m, v = (sd[k].cpu().double() for k in ("master", "exp_avg", "exp_avg_sq"))
        g = torch.randn(N, generator=gen).to(dst_dtype if grad16 else torch.float32)
        opt.step(g.to(DEV), LR, gs)
        gg = g.double() * (float(gs.item()) if with_gscale else 1.0)
        p64 = p * (1.0 - LR * WD)
        m64 = m + (1.0 - B1) * (gg - m)
        v64 = B2 * v + (1.0 - B2) * gg * gg
        p64 = p64 - (LR / (1.0 - B1 ** step)) * m64 / (v64.sqrt() / math.sqrt(1.0 - B2 ** step) + EPS)
        got = opt.state_dict()
        gp = got["master"].cpu()
        assert torch.equal(gp[~inside], p.float()[~inside])                  # nothing outside the segments moved
        err = (gp.double() - p64).abs()[inside]
        tol = (1e-6 + 1e-5 * p64.abs())[inside]
        assert bool((err <= tol).all()), ("master", step, float((err / tol).max()))
        d16 = dst.cpu().double()
        want16 = p64.to(dst_dtype).double()
        assert bool(((d16 - want16).abs() <= 1e-2 + 1e-2 * want16.abs())[inside].all()), ("16-bit copy", step)
        assert not dst.cpu()[~inside].any()
        ms, ss = _scale_of(opt, 0), _scale_of(opt, 1)
        _within_one_quantum(got["exp_avg"].cpu()[inside], m64[inside], ms[inside], False, ("m", step))
        _within_one_quantum(got["exp_avg_sq"].cpu().sqrt()[inside], v64.sqrt()[inside], ss[inside], True, ("s", step))
        assert not opt.exp_avg.cpu()[~inside].any() and not opt.exp_avg_sq.cpu()[~inside].any()


def _state(opt, dst):
    return [t.clone() for t in (opt.master, opt.exp_avg, opt.exp_avg_sq, opt.exp_avg_scale, opt.exp_avg_sq_scale, dst)]


def _grads(k, dtype=torch.bfloat16):
    gen = torch.Generator().manual_seed(23)
    return [torch.randn(N, generator=gen).to(dtype).to(DEV) for _ in range(k)]


def test_launch_forms_bitwise():
    """Per-segment launches, sub-group launches (one table row each) and a capped grid give the single launch's
    codes, scales, master and copies bit for bit: every form addresses the scales of the global row."""
    grads = _grads(2)
    outs = {}
    for form in ("single", "segments", "sub_groups", "grid_cap"):
        opt, dst = _fresh(sub_group=4096 if form == "sub_groups" else 0)
        rows = opt._tables[0].numel()
        assert rows == 1 + 1 + 1 + 1 + 2
        for g in grads:
            opt.prepare(LR)
            if form == "segments":
                for i in reversed(range(len(LENS))):
                    opt.launch_segment(i, g)
            elif form == "grid_cap":
                opt._launch_rows(0, rows, g, None, grid_cap=4)
            else:
                assert opt.launches_per_step == (rows if form == "sub_groups" else 1)
                opt.launch(g)
        outs[form] = _state(opt, dst)
    for form, got in outs.items():
        for a, b in zip(outs["single"], got):
            assert torch.equal(a, b), form
    assert outs["single"][1].any() and not torch.equal(outs["single"][3], torch.ones_like(outs["single"][3]))


def test_skipped_step_touches_nothing():
    opt, dst = _fresh(torch.float16)
    opt.step(_grads(1, torch.float16)[0], LR)
    before = _state(opt, dst)
    opt.prepare(LR)
    opt.hp[3:4].fill_(1.0)                      # the dynamic loss scaler's skip
    opt.launch(_grads(2, torch.float16)[1])
    for a, b in zip(before, _state(opt, dst)):
        assert torch.equal(a, b)


def test_graph_replay_counter_travels_through_hp():
    """A captured launch replayed 3 times (the step values uploaded before each replay) equals 3 eager steps bit for
    bit; two replays from one state with different counters give different codes."""
    g = _grads(1)[0]
    eager, dst_e = _fresh()
    for _ in range(3):
        eager.step(g, LR)
    opt, dst = _fresh()
    opt.prepare(LR)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.launch(g)
    graph.replay()
    for _ in range(2):
        opt.prepare(LR)
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(_state(eager, dst_e), _state(opt, dst)):
        assert torch.equal(a, b)
    codes = []
    for counter in (4, 5):
        opt.master.copy_(eager.master), opt.exp_avg.copy_(eager.exp_avg), opt.exp_avg_sq.copy_(eager.exp_avg_sq)
        opt.exp_avg_scale.copy_(eager.exp_avg_scale), opt.exp_avg_sq_scale.copy_(eager.exp_avg_sq_scale)
        opt.step_count = counter - 1
        opt.prepare(LR)
        graph.replay()
        torch.cuda.synchronize()
        codes.append(opt.exp_avg.clone())
    assert not torch.equal(codes[0], codes[1])


def test_default_state_launches_the_existing_kernel(monkeypatch):
    """``state="fp32"`` goes through ``ext().adamw`` alone, and its 3-step run is bit for bit the one made before any
    fp8 optimizer existed in the process."""
    calls = {"adamw": 0, "adamw_fp8": 0}
    C = ext()
    real, real8 = C.adamw, C.adamw_fp8

    def count(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped
    monkeypatch.setattr(C, "adamw", count("adamw", real))
    monkeypatch.setattr(C, "adamw_fp8", count("adamw_fp8", real8))
    grads = _grads(3)

    def run32():
        opt, dst = _fresh(state="fp32")
        assert opt.exp_avg.dtype == torch.float32 and opt.hp.numel() == 4 and opt.exp_avg_scale is None
        for g in grads:
            opt.step(g, LR)
        return [t.clone() for t in (opt.master, opt.exp_avg, opt.exp_avg_sq, dst)]
    first = run32()
    assert calls == {"adamw": 3, "adamw_fp8": 0}
    o8, _ = _fresh()
    o8.step(grads[0], LR)
    assert calls == {"adamw": 3, "adamw_fp8": 1}
    for a, b in zip(first, run32()):
        assert torch.equal(a, b)
    assert calls == {"adamw": 6, "adamw_fp8": 1}


# ------------------------------------------------------------------------------ engines
# the bounds of tests/test_multirank_gpu.py (bf16 HIP run against its reference run, fp32 state)
BOUNDS = dict(loss_tol=1e-3, upd_tol=0.02, cos_min=0.9998, param_tol=0.03)
STEPS8 = ("--windows", "8", "--accum", "1", "--optimizer-state", "fp8", "--init-device", "cpu")


def _check(cpu, gpu, what):
    print(f"[adamw_fp8] {what} GPU vs CPU:", json.dumps(report(cpu, gpu)))
    for case, r in gpu.items():
        assert len(r["losses"]) == 8 and r["losses"][-1] < r["losses"][0], (case, r["losses"])
    bad = compare(cpu, gpu, **BOUNDS)
    assert not bad, (what, bad)


def test_engines_world1_match_cpu(tmp_path):
    """mtiny under zero2 and ddp, 8 optimizer steps with the fp8 state: the HIP run against the CPU engine (the same
    blocks and random words; the moments differ by the bf16 gradients)."""
    ex = ("--cases", "cp_zero2,cp_ddp") + STEPS8
    _check(run(tmp_path / "c.pt", 1, "cpu", extra=ex), run(tmp_path / "g.pt", 1, "cuda", extra=ex, timeout=600), "ws1")


def test_engine_world2_zero3_host_staged_matches_cpu(tmp_path):
    ex = ("--cases", "zero3_mistral") + STEPS8
    cpu = run(tmp_path / "c.pt", 2, "cpu", extra=ex)
    gpu = run(tmp_path / "g.pt", 2, "cuda", extra=ex, env_extra={"DLTB_COMM": "host"}, timeout=600)
    _check(cpu, gpu, "ws2 zero3")


def test_engine_resume_continues_bit_for_bit():
    """zero2 on mtiny: save after step 4, load into a fresh engine, steps 5-8 equal the uninterrupted run's."""
    cfg = get_model_config("mtiny", 256)
    table = torch.randint(0, cfg.vocab_size, (8, 1, 256), generator=torch.Generator().manual_seed(4)).to(DEV)

    def engine():
        torch.manual_seed(0)
        with torch.device(DEV):
            model = build_model(cfg)
        eng = make_engine(model, engine_config("zero2", 1, "reference", optimizer_state="fp8"), "cuda:0")
        eng.train()
        assert eng.opt.fp8 and eng.memory_report()["optimizer_state"] == "fp8"
        return eng

    def steps(eng, lo, hi):
        out = []
        for k in range(lo, hi):
            loss = eng(table[k], table[k])[1]
            eng.backward(loss)
            eng.step()
            out.append(loss.item())
        return out
    a = engine()
    la = steps(a, 0, 8)
    fa = {k: v.clone() for k, v in a.full_state_dict().items()}
    oa = a.opt.state_dict()
    b = engine()
    steps(b, 0, 4)
    sd = b.state_dict()
    sd["optimizer"] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd["optimizer"].items()}
    c = engine()
    c.load_state_dict(sd)
    lc = steps(c, 4, 8)
    assert lc == la[4:], (lc, la[4:])
    fc = c.full_state_dict()
    for k in fa:
        assert torch.equal(fa[k], fc[k]), k
    oc = c.opt.state_dict()
    for k in ("master", "exp_avg", "exp_avg_sq"):
        assert torch.equal(oa[k], oc[k]), k
