"""The model-level check of tests/test_bias_from_dw_cpu.py on the GPU (bf16 kernels): a 2-layer TinyGPT at d = 256,
T = 128, accum = 2 with dropout gives identical losses and weight gradients with the bias_from_dw switch on and off,
and bias gradients within 2 bf16 ulps (the bound is derived in ``compare_model``)."""
import pytest

from test_bias_from_dw_cpu import compare_model

pytestmark = pytest.mark.gpu


def test_model_bias_from_dw_gpu():
    eng = compare_model("cuda:0")
    assert eng._wq.batched_calls >= 4 and eng._wq.single_calls == 0
