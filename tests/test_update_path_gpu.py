"""The optimizer update path, kernel by kernel, against the float64 references of tests/update_ref.py:

    f32_from_bf16_ -> sumsq_ -> clip_coef | amp_step -> adamw        (csrc/elementwise.hip, csrc/adamw.hip)

Tolerances come from the number formats and the references alone (each is derived where it is used);
none is taken from what the kernels return.  Every test prints the figures it asserts on."""
import functools
import math

import pytest
import torch

import dltb  # noqa: F401
from dltb.ops import ref
from dltb.ops._ext import ext
from dltb.optim.adamw import FlatAdamW
from dltb.optim.amp import DynamicLossScaler

from update_ref import (AMP_EXTRA, AMP_INIT_SCALE, AMP_INTERVAL, AMP_NORM_SQ, adamw64, amp64,
                        bias_correction_bound, clip64)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16

# a sqrt, a multiply, an add and a divide in fp32, with room: 8 half-ulps
SCALAR_RTOL = 8 * 2.0 ** -24


def f32(x):
    return float(torch.tensor(x, dtype=F32))


def bits(t):
    """The tensor's storage as integers (bitwise comparisons: -0.0 != 0.0, nan == nan)."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def rel(got, want):
    return abs(got - want) / abs(want)


# ------------------------------------------------------------------------------ f32_from_bf16_
# 8 elements per lane, 256 lanes, at most 2048 blocks: at the second size the full grid wraps its
# grid-stride loop, and the last pass covers 3 vectors only.
@pytest.mark.parametrize("n", [8, 8 * (256 * 2048 + 3)])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("dtype", [BF16, F16])
def test_f32_from_16bit_is_exact(dtype, accumulate, n):
    gen = torch.Generator(DEV).manual_seed(n % 997 + int(accumulate))
    src = torch.randn(n, device=DEV, generator=gen).to(dtype)
    dst0 = torch.randn(n, device=DEV, generator=gen)
    dst = dst0.clone()
    ext().f32_from_bf16_(dst, src, accumulate)
    want = dst0 + src.float() if accumulate else src.float()      # one fp32 add per element, or none
    assert same_bits(dst, want)


# ------------------------------------------------------------------------------ sumsq_
# The longest chain of fp32 additions a term passes through (csrc/adamw.hip, sumsq_kernel and
# sumsq_final_kernel), at the size where it is longest (one unrolled pass, then the tail loop):
#    3   g0*g0 + g1*g1 + g2*g2 + g3*g3, left to right
#    2   a[0] += ... in the unrolled pass, and once more in the tail loop
#    2   (a[0] + a[1]) + (a[2] + a[3])
#    6   wave_sum: six shuffle-and-add rounds over 64 lanes
#    4   block_sum: 0 + red[0] + red[1] + red[2] + red[3]
#    4   sumsq_final_kernel: 1024 partials over 256 lanes, acc += part[i] four times
#   10   its block_sum (6 + 4)
#    1   out[0] += acc
# = 32 additions, and one rounding for the square itself.  All terms are non-negative, so the relative
# error of the sum is at most 33 roundings of 2^-24 each to first order; 2^-23 each leaves the margin.
SUMSQ_CHAIN = 32
SUMSQ_RTOL = (SUMSQ_CHAIN + 1) * 2.0 ** -23
SUMSQ_UNROLLED_AND_TAIL = 4 * (4 * 256 * 1024 + 5 * 256 + 1)     # one unrolled pass, the tail loop on 1281 lanes
SUMSQ_TAIL_ONLY = 4 * (256 * 1024 - 1)                           # the full grid, the tail loop only
SUMSQ_OUT0 = 3.25


def _sumsq_input(dtype, n):
    gen = torch.Generator(DEV).manual_seed(n % 1009)
    return torch.randn(n, device=DEV, generator=gen).to(dtype)


@pytest.mark.parametrize("n", [4, 1020, 1024, SUMSQ_UNROLLED_AND_TAIL, SUMSQ_TAIL_ONLY])
@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_sumsq_against_float64(dtype, n):
    x = _sumsq_input(dtype, n)
    out = torch.full((1,), SUMSQ_OUT0, device=DEV)               # the kernel adds into out
    ext().sumsq_(x, out)
    want = SUMSQ_OUT0 + float((x.double() ** 2).sum())
    err = rel(out.item(), want)
    print(f"sumsq {dtype} n={n}: relative error {err:.3e} (bound {SUMSQ_RTOL:.3e})")
    assert err <= SUMSQ_RTOL
    again = torch.full((1,), SUMSQ_OUT0, device=DEV)
    ext().sumsq_(x, again)
    assert same_bits(out, again)                                 # fixed summation order


@pytest.mark.parametrize("where", ["inf_first", "inf_last", "nan_middle"])
@pytest.mark.parametrize("n", [1020, SUMSQ_UNROLLED_AND_TAIL])
@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_sumsq_carries_non_finite_input(dtype, n, where):
    """The inf check of dynamic loss scaling: one inf or nan anywhere makes the sum non-finite."""
    x = _sumsq_input(dtype, n)
    if where == "inf_first":
        x[0] = float("inf")
    elif where == "inf_last":
        x[-1] = float("-inf")
    else:
        x[n // 2 + 1] = float("nan")
    out = torch.zeros(1, device=DEV)
    ext().sumsq_(x, out)
    assert not math.isfinite(out.item())


# ------------------------------------------------------------------------------ clip_coef
@pytest.mark.parametrize("norm_sq, max_norm, extra, with_norm", [
    (7.3, 1.0, 1.0, True),           # clip active
    (0.31, 1.0, 1.0, True),          # clip inactive: the norm is below max_norm
    (7.3, 0.0, 1.0, True),           # no clipping
    (467.2, 1.0, 0.125, True),       # extra_scale: norm 2.7, active
    (20.0, 1.0, 0.125, True),        # extra_scale: norm 0.56, inactive
    (7.3, 0.0, 0.125, True),
    (467.2, 1.0, 0.125, False),      # norm_out None
])
def test_clip_coef_against_float64(norm_sq, max_norm, extra, with_norm):
    nsq = torch.tensor([norm_sq], dtype=F32, device=DEV)
    coef = torch.full((1,), -1.0, device=DEV)
    nrm = torch.full((1,), -1.0, device=DEV) if with_norm else None
    ext().clip_coef(nsq, max_norm, coef, nrm, extra)
    want_c, want_n = clip64(nsq.item(), max_norm, extra)
    print(f"clip_coef: coef error {rel(coef.item(), want_c):.3e}"
          + (f", norm error {rel(nrm.item(), want_n):.3e}" if with_norm else ""))
    assert rel(coef.item(), want_c) <= SCALAR_RTOL
    if with_norm:
        assert rel(nrm.item(), want_n) <= SCALAR_RTOL


# ------------------------------------------------------------------------------ amp_step
LR, B1, B2, EPS, WD, GS = 3e-3, 0.8, 0.95, 1e-6, 0.1, 0.37


@pytest.mark.parametrize("max_norm", [1.0, 0.0])
def test_amp_step_against_float64(max_norm):
    """One state and one hp = [lr, 0, 0, 0] through: finite, finite (clip active), inf, finite, nan, three
    finite calls (the scale grows on the last).  Compared with amp64 after every call."""
    C = ext()
    b1, b2 = f32(B1), f32(B2)                                    # the values the kernel receives
    state = torch.tensor([AMP_INIT_SCALE, 0.0, 0.0, 0.0], device=DEV)
    hp = torch.tensor([LR, 0.0, 0.0, 0.0], device=DEV)
    want_state = state.tolist()
    taken = 0
    for call, v in enumerate(AMP_NORM_SQ, 1):
        nsq = torch.tensor([v], dtype=F32, device=DEV)
        coef = torch.full((1,), -1.0, device=DEV)
        nrm = torch.full((1,), -1.0, device=DEV)
        hp_before = hp.clone()
        C.amp_step(nsq, state, coef, nrm, hp, max_norm, AMP_EXTRA, B1, B2, 2.0, 0.5, AMP_INTERVAL)
        want_state, want_c, want_n, want_hp = amp64(want_state, nsq.item(), hp_before.tolist(), max_norm,
                                                    AMP_EXTRA, b1, b2, 2.0, 0.5, AMP_INTERVAL)
        assert state.tolist() == want_state, f"call {call}: state"          # powers of two, small integers
        assert same_bits(hp[0], hp_before[0]), f"call {call}: hp[0] (lr) is the host's"
        assert hp[3].item() == want_hp[3], f"call {call}: skip flag"
        if not math.isfinite(v):
            assert want_hp[3] == 1.0
            assert same_bits(hp[1:3], hp_before[1:3]), f"call {call}: bias corrections of a skipped call"
            assert coef.item() == 0.0
            assert not math.isfinite(nrm.item()) and math.isnan(nrm.item()) == math.isnan(v)
            continue
        taken += 1
        t = want_state[2]
        # the device step count: one lower than the call count after the inf, two lower after the nan
        assert t == taken == call - (call > 3) - (call > 5)
        e1, e2 = rel(hp[1].item(), want_hp[1]), rel(hp[2].item(), want_hp[2])
        print(f"amp_step call {call} (t={int(t)}): coef error {rel(coef.item(), want_c):.3e}, norm error "
              f"{rel(nrm.item(), want_n):.3e}, hp[1] error {e1:.3e} (bound {bias_correction_bound(b1, t):.3e}), "
              f"hp[2] error {e2:.3e} (bound {bias_correction_bound(b2, t):.3e})")
        assert rel(coef.item(), want_c) <= SCALAR_RTOL
        assert rel(nrm.item(), want_n) <= SCALAR_RTOL
        assert e1 <= bias_correction_bound(b1, t) and e2 <= bias_correction_bound(b2, t)
    assert want_state == [512.0, 0.0, 6.0, 2.0]


# ------------------------------------------------------------------------------ adamw
# One owner space of five segments: a single vector, one vector short of adamw_chunk() (4096), one exact
# chunk, a chunk plus a vector, two chunks plus two vectors.  Each destination is a view into one 16-bit
# buffer with GAP sentinel elements before, between and after the views; the views at element offsets
# 12, 28 and 4132 sit at 8-byte but not 16-byte aligned addresses.
SEG_LENS = (4, 4092, 4096, 4100, 8200)
N = sum(SEG_LENS)
GAP = 12
SENTINEL = 0x7E57
GRADS = {"f32": F32, "bf16": BF16, "f16": F16}
COMBOS = [("f32", BF16), ("bf16", BF16), ("f32", F16), ("f16", F16)]       # gradient dtype x destination dtype


class Layout:
    def __init__(self, ddtype, lens=SEG_LENS, gap=GAP):
        self.buf = torch.empty(sum(lens) + gap * (len(lens) + 1), dtype=ddtype, device=DEV)
        bits(self.buf).fill_(SENTINEL)
        self.is_gap = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEV)
        self.segments = []
        ostart, off = 0, gap
        for n in lens:
            self.segments.append((ostart, n, self.buf[off:off + n]))
            self.is_gap[off:off + n] = False
            ostart, off = ostart + n, off + n + gap
        if lens is SEG_LENS:
            assert ext().adamw_chunk() == 4096
            assert any(d.data_ptr() % 16 == 8 for _, _, d in self.segments)

    def check(self, master, what):
        """Gaps untouched; every destination the round-to-nearest-even 16-bit copy of the kernel's own master."""
        assert bool((bits(self.buf)[self.is_gap] == SENTINEL).all()), f"{what}: a gap between destinations was written"
        for i, (ostart, n, dst) in enumerate(self.segments):
            assert same_bits(dst, master[ostart:ostart + n].to(dst.dtype)), f"{what}: 16-bit copy of segment {i}"


class Oracle:
    """The float64 trajectory, and beside it the same formula in plain fp32 torch (ref.adamw_flat on CPU
    tensors).  The fp32 evaluation's maximum error against float64 sets the kernel's tolerance: 4 times
    it, per quantity (the margin covers the kernel's different operation order: step_size * m / denom
    against addcdiv, m + w (g - m) against lerp)."""

    def __init__(self, master, m, v):
        self.s64 = [x.double().clone() for x in (master, m, v)]
        self.s32 = [x.float().clone() for x in (master, m, v)]
        self.mag = None

    def step(self, g, t, gscale):
        """``g`` as stored (fp32 or 16-bit), ``gscale`` the fp32 value the kernel reads."""
        _, m, v = self.s64
        zero = torch.zeros_like(m)
        # the size of the update with the cancellation in m taken out: the scale of a zero-master comparison
        self.mag = -adamw64(zero, m.abs(), v, g.double().abs(), LR, B1, B2, EPS, 0.0, t, gscale)[0]
        self.s64 = list(adamw64(*self.s64, g, LR, B1, B2, EPS, WD, t, gscale))
        ref.adamw_flat(*self.s32, g, LR, B1, B2, EPS, WD, t, torch.tensor(gscale, dtype=F32))

    def zero_master(self):
        self.s64[0].zero_()
        self.s32[0].zero_()

    def abs_errors(self, state):
        return [float((x.double().cpu() - w).abs().max()) for x, w in zip(state, self.s64)]

    def rel_update_error(self, master):
        return float(((master.double().cpu() - self.s64[0]).abs() / self.mag).max())

    def check(self, state, what, zero_master=False):
        got, base = self.abs_errors(state), self.abs_errors(self.s32)
        for name, e, b in zip(("master", "exp_avg", "exp_avg_sq"), got, base):
            print(f"{what}: {name} max error {e:.3e}; fp32 torch {b:.3e}, tolerance {4 * b:.3e}")
        if zero_master:
            e, b = self.rel_update_error(state[0]), self.rel_update_error(self.s32[0])
            print(f"{what}: update max relative error {e:.3e}; fp32 torch {b:.3e}, tolerance {4 * b:.3e}")
            assert e <= 4 * b, f"{what}: update (zero master)"
            got, base = got[1:], base[1:]
        for e, b in zip(got, base):
            assert e <= 4 * b, what


@functools.lru_cache(maxsize=None)
def _case(kind, gname):
    """Inputs (CPU, read-only) of one case.  'traj': three steps from zero moments; 'late': one step at
    step 1000 from random exp_avg and random non-negative exp_avg_sq; 'probe': 'late' with master = 0."""
    gen = torch.Generator().manual_seed(20)
    master = torch.randn(N, generator=gen)
    if kind == "traj":
        m, v, steps = torch.zeros(N), torch.zeros(N), (1, 2, 3)
    else:
        m, v, steps = 0.3 * torch.randn(N, generator=gen), 0.2 * torch.rand(N, generator=gen), (1000,)
    if kind == "probe":
        master = torch.zeros(N)
    grads = tuple(torch.randn(N, generator=gen).to(GRADS[gname]) for _ in steps)
    return master, m, v, steps, grads


def _opt(case, ddtype, sub_group=0):
    master, m, v, _, _ = case
    lay = Layout(ddtype)
    opt = FlatAdamW(master.to(DEV), lay.segments, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD,
                    sub_group=sub_group)
    opt.exp_avg.copy_(m)
    opt.exp_avg_sq.copy_(v)
    return opt, lay


def _state(opt):
    return opt.master, opt.exp_avg, opt.exp_avg_sq


def _manual_hp(t, skip=0.0):
    """[lr, lr/bc1, 1/sqrt(bc2), skip] computed in float64 and stored as fp32, as FlatAdamW.upload does."""
    return torch.tensor([LR, LR / (1.0 - B1 ** t), 1.0 / math.sqrt(1.0 - B2 ** t), skip], dtype=F32, device=DEV)


def _launch(opt, mode, g, gscale, t, skip=False):
    """One update at step ``t``.  'host': hyper-parameters as host arguments (hp=None); 'hp': a hand-made
    device hp through ext().adamw; the rest through FlatAdamW (prepare uploads hp)."""
    if mode in ("host", "hp"):
        hp = None if mode == "host" else _manual_hp(t, float(skip))
        ext().adamw(*_state(opt), g, *opt._tables, gscale, LR, B1, B2, EPS, WD, t, hp, opt.dst_f16)
        return
    opt.step_count = t - 1
    opt.prepare(LR)
    if skip:
        opt.hp[3] = 1.0
    if mode in ("launch", "sub_group"):
        assert opt.launches_per_step == (8 if opt.sub_group else 1)
        opt.launch(g, gscale)
    elif mode == "segments":
        for i in range(len(opt.segments)):
            opt.launch_segment(i, g, gscale)
    elif mode == "grid_cap":                       # all 8 rows of the block table on 3 workgroups
        opt._launch_rows(0, opt._tables[0].numel(), g, gscale, 3)
    else:
        raise ValueError(mode)


def _run(kind, gname, ddtype, mode):
    case = _case(kind, gname)
    opt, lay = _opt(case, ddtype, ext().adamw_chunk() if mode == "sub_group" else 0)
    gscale = torch.tensor([GS], dtype=F32, device=DEV)
    for t, g in zip(case[3], case[4]):
        _launch(opt, mode, g.to(DEV), gscale, t)
        lay.check(opt.master, f"{kind} {gname} {mode} step {t}")
    return opt, lay


@functools.lru_cache(maxsize=None)
def _oracle(kind, gname):
    master, m, v, steps, grads = _case(kind, gname)
    o = Oracle(master, m, v)
    for t, g in zip(steps, grads):
        o.step(g, t, f32(GS))
    return o


@pytest.mark.parametrize("mode", ["host", "launch"])
@pytest.mark.parametrize("kind", ["traj", "late", "probe"])
@pytest.mark.parametrize("gname, ddtype", COMBOS)
def test_adamw_against_float64(gname, ddtype, kind, mode):
    opt, _ = _run(kind, gname, ddtype, mode)
    _oracle(kind, gname).check(_state(opt), f"adamw {kind} {gname}->{ddtype} {mode}", zero_master=kind == "probe")


@pytest.mark.parametrize("kind", ["traj", "late"])
@pytest.mark.parametrize("gname, ddtype", COMBOS)
def test_adamw_device_hp_is_bitwise_the_host_arguments(gname, ddtype, kind):
    want, wlay = _run(kind, gname, ddtype, "host")
    for mode in ("hp", "launch"):
        got, lay = _run(kind, gname, ddtype, mode)
        for a, b in zip(_state(got) + (lay.buf,), _state(want) + (wlay.buf,)):
            assert same_bits(a, b), mode


@pytest.mark.parametrize("mode", ["sub_group", "segments", "grid_cap"])
@pytest.mark.parametrize("gname, ddtype", COMBOS)
def test_adamw_decomposed_launches_are_bitwise_the_single_launch(gname, ddtype, mode):
    want, wlay = _run("traj", gname, ddtype, "launch")
    got, lay = _run("traj", gname, ddtype, mode)
    for a, b in zip(_state(got) + (lay.buf,), _state(want) + (wlay.buf,)):
        assert same_bits(a, b)


@pytest.mark.parametrize("mode", ["hp", "launch", "segments", "sub_group", "grid_cap"])
@pytest.mark.parametrize("gname, ddtype", [("bf16", BF16), ("f32", F16)])
def test_adamw_skip_flag_leaves_every_byte(gname, ddtype, mode):
    case = _case("late", gname)
    opt, lay = _opt(case, ddtype, ext().adamw_chunk() if mode == "sub_group" else 0)
    gscale = torch.tensor([GS], dtype=F32, device=DEV)
    _launch(opt, "launch", case[4][0].to(DEV), gscale, 999)       # destinations hold real copies
    before = [x.clone() for x in _state(opt) + (lay.buf,)]
    _launch(opt, mode, case[4][0].to(DEV), gscale, 1000, skip=True)
    for a, b in zip(_state(opt) + (lay.buf,), before):
        assert same_bits(a, b)


def test_adamw_rejects_hp_without_skip_flag():
    """The kernel reads hp[3]: a three-element hp is an error, and nothing is launched."""
    case = _case("late", "bf16")
    opt, lay = _opt(case, BF16)
    before = [x.clone() for x in _state(opt) + (lay.buf,)]
    with pytest.raises(RuntimeError, match="adam hp"):
        ext().adamw(*_state(opt), case[4][0].to(DEV), *opt._tables, None, LR, B1, B2, EPS, WD, 1000,
                    _manual_hp(1000)[:3], False)
    for a, b in zip(_state(opt) + (lay.buf,), before):
        assert same_bits(a, b)


# ------------------------------------------------------------------------------ the chain
def test_update_chain_as_the_engine_runs_it():
    """prepare -> sumsq_ -> DynamicLossScaler.step -> launch(g, coef), as Engine._apply_update and
    _clip_coef do with fp16 gradients: a clean step, one with an inf gradient, a clean one.  Every float64
    stage is fed the fp32 value its kernel stage received, and every such value is checked against the
    float64 stage before it: sumsq_ by SUMSQ_RTOL, coef by SCALAR_RTOL, hp by the bias-correction bound."""
    C = ext()
    lens, S0, max_norm, extra = (4100, 8196), 2.0 ** 12, 1.0, 0.5
    n = sum(lens)
    assert n == 12296
    gen = torch.Generator().manual_seed(6)
    master0 = torch.randn(n, generator=gen)
    lay = Layout(F16, lens, 0)
    opt = FlatAdamW(master0.to(DEV), lay.segments, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
    scaler = DynamicLossScaler(DEV, init_scale=S0, growth_interval=2000)
    norm_sq, coef, gnorm = (torch.zeros(1, device=DEV) for _ in range(3))
    oracle = Oracle(master0, torch.zeros(n), torch.zeros(n))
    b1, b2 = f32(B1), f32(B2)
    want_state = [S0, 0.0, 0.0, 0.0]
    for k in range(3):
        S = want_state[0]
        g = (0.05 * torch.randn(n, generator=gen) * S).to(F16)     # the backward seed is S: gradients arrive scaled
        if k == 1:
            g[777] = float("inf")
        if k == 2:                                                   # zero-master form: the result is the update
            opt.master.zero_()
            oracle.zero_master()
        before = [x.clone() for x in _state(opt) + (lay.buf,)]
        gd = g.to(DEV)
        opt.prepare(LR)
        norm_sq.zero_()
        C.sumsq_(gd, norm_sq)
        scaler.step(norm_sq, coef, gnorm, opt.hp, max_norm, extra, opt.betas)
        opt.launch(gd, coef)

        want_nsq = float((g.double() ** 2).sum())
        want_state, want_c, want_n, want_hp = amp64(want_state, norm_sq.item(), [f32(LR), 0.0, 0.0, 0.0], max_norm,
                                                    extra, b1, b2, 2.0, 0.5, 2000)
        assert scaler.state.tolist() == want_state and opt.hp[3].item() == want_hp[3]
        if k == 1:
            assert not math.isfinite(norm_sq.item()) and coef.item() == 0.0
            assert want_state == [S0 / 2, 0.0, 1.0, 1.0]             # S halved, one step taken, one skipped
            for a, b in zip(_state(opt) + (lay.buf,), before):
                assert same_bits(a, b)                               # nothing moved
            continue
        t = want_state[2]
        assert t == (1 if k == 0 else 2) and opt.step_count == k + 1  # the device count, not the host's
        assert rel(norm_sq.item(), want_nsq) <= SUMSQ_RTOL
        assert want_n > max_norm                                     # the clip is active
        assert rel(coef.item(), want_c) <= SCALAR_RTOL and rel(gnorm.item(), want_n) <= SCALAR_RTOL
        assert same_bits(opt.hp[0], torch.tensor(LR, device=DEV))
        assert rel(opt.hp[1].item(), want_hp[1]) <= bias_correction_bound(b1, t)
        assert rel(opt.hp[2].item(), want_hp[2]) <= bias_correction_bound(b2, t)
        oracle.step(g, int(t), coef.item())                          # unscaled by the current (halved) S
        oracle.check(_state(opt), f"chain step {k + 1} (t={int(t)})", zero_master=k == 2)
        lay.check(opt.master, f"chain step {k + 1}")
