"""The float64 references of tests/update_ref.py (the oracle of tests/test_update_path_gpu.py)
against torch.optim.AdamW and the CPU branch of DynamicLossScaler.step, and the float32
bias-correction bound used on the GPU."""
import math

import numpy as np
import torch

import dltb  # noqa: F401
from dltb.optim.amp import DynamicLossScaler

from update_ref import (AMP_EXTRA, AMP_INIT_SCALE, AMP_INTERVAL, AMP_NORM_SQ, adamw64, amp64,
                        bias_correction_bound, clip64)


def test_adamw64_matches_torch_adamw():
    lr, (b1, b2), eps, wd = 3e-3, (0.8, 0.95), 1e-6, 0.1
    gen = torch.Generator().manual_seed(0)
    p0 = torch.randn(1000, dtype=torch.float64, generator=gen)
    tp = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for t in range(1, 6):
        g = torch.randn(1000, dtype=torch.float64, generator=gen)
        tp.grad = g.clone()
        opt.step()
        p, m, v = adamw64(p, m, v, g, lr, b1, b2, eps, wd, t)
    st = opt.state[tp]
    torch.testing.assert_close(p, tp.detach(), rtol=1e-12, atol=0)
    torch.testing.assert_close(m, st["exp_avg"], rtol=1e-12, atol=0)
    torch.testing.assert_close(v, st["exp_avg_sq"], rtol=1e-12, atol=0)


def test_adamw64_gscale_scales_the_gradient():
    gen = torch.Generator().manual_seed(1)
    p, m, g = (torch.randn(64, dtype=torch.float64, generator=gen) for _ in range(3))
    v = torch.rand(64, dtype=torch.float64, generator=gen)
    a = adamw64(p, m, v, g, 3e-3, 0.8, 0.95, 1e-6, 0.1, 7, 0.37)
    b = adamw64(p, m, v, g * 0.37, 3e-3, 0.8, 0.95, 1e-6, 0.1, 7)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_clip64_cases():
    assert clip64(4.0, 1.0, 1.0) == (1.0 / (2.0 + 1e-6), 2.0)          # active
    assert clip64(0.25, 1.0, 1.0) == (1.0, 0.5)                        # inactive
    assert clip64(4.0, 0.0, 0.125) == (0.125, 0.25)                    # no clipping at all
    c, n = clip64(4096.0, 1.0, 0.125)                                  # the norm is that of extra * g
    assert n == 8.0 and c == 0.125 / (8.0 + 1e-6)


def test_amp64_matches_the_cpu_scaler_branch():
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))        # noqa: E731
    b1, b2 = f32(0.8), f32(0.95)
    for max_norm in (1.0, 0.0):
        mine = DynamicLossScaler("cpu", init_scale=AMP_INIT_SCALE, growth_interval=AMP_INTERVAL)
        state, hp = mine.state.tolist(), [f32(3e-3), 0.0, 0.0, 0.0]
        coef, nrm = torch.zeros(1), torch.zeros(1)
        taken = 0
        for nsq in AMP_NORM_SQ:
            nsq = f32(nsq)
            old_hp = list(hp)
            mine.step(torch.tensor([nsq]), coef, nrm, None, max_norm, AMP_EXTRA, (b1, b2))
            state, c64, n64, hp = amp64(state, nsq, hp, max_norm, AMP_EXTRA, b1, b2, 2.0, 0.5, AMP_INTERVAL)
            assert state == mine.state.tolist()
            if math.isfinite(nsq):
                taken += 1
                assert not mine.last_skipped and hp[3] == 0.0
                assert abs(float(coef) - c64) <= 2.0 ** -23 * c64
                assert abs(float(nrm) - n64) <= 2.0 ** -23 * n64
                # what the CPU branch leaves to FlatAdamW.upload: the bias corrections of the device step count
                assert hp[0] == old_hp[0]
                assert hp[1] == hp[0] / (1.0 - b1 ** taken) and hp[2] == 1.0 / math.sqrt(1.0 - b2 ** taken)
            else:
                assert mine.last_skipped and hp[3] == 1.0 and hp[:3] == old_hp[:3]
                assert float(coef) == c64 == 0.0
                assert not math.isfinite(float(nrm)) and not math.isfinite(n64)
        assert state == [512.0, 0.0, 6.0, 2.0]


def test_float32_bias_corrections_stay_inside_the_bound():
    """hp[1] = lr / (1 - b1^t) and hp[2] = 1 / sqrt(1 - b2^t) evaluated in float32 (numpy's powf) against
    float64 on the same float32 betas: the worst case over these t is printed as a fraction of the bound."""
    lr = np.float32(3e-3)
    one = np.float32(1.0)
    worst = 0.0
    for betas in ((0.9, 0.999), (0.9, 0.95)):
        b1, b2 = (np.float32(b) for b in betas)
        for t in list(range(1, 3001)) + [10 ** 4, 10 ** 5]:
            tf = np.float32(t)
            h1 = lr / (one - np.power(b1, tf))
            h2 = one / np.sqrt(one - np.power(b2, tf))
            assert h1.dtype == h2.dtype == np.float32
            w1 = float(lr) / (1.0 - float(b1) ** t)
            w2 = 1.0 / math.sqrt(1.0 - float(b2) ** t)
            e1 = abs(float(h1) - w1) / w1 / bias_correction_bound(float(b1), t)
            e2 = abs(float(h2) - w2) / w2 / bias_correction_bound(float(b2), t)
            assert e1 <= 1.0 and e2 <= 1.0, (betas, t, e1, e2)
            worst = max(worst, e1, e2)
    print(f"worst float32 bias-correction error: {worst:.3f} of the bound")
