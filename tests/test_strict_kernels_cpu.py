"""Strict mode for torch GEMM fallbacks: ``functional.strict_kernels`` turns the counted fallback into
an error, ``harness.py --strict-kernels`` sets it for one run and records it in the sidecar."""
import json
import os
import warnings

import pytest

import dltb  # noqa: F401
from dltb.ops import functional as F_


@pytest.fixture
def clean_counter():
    saved = dict(F_.torch_fallbacks)
    F_.torch_fallbacks.clear()
    yield
    F_.strict_kernels = False
    F_.torch_fallbacks.clear()
    F_.torch_fallbacks.update(saved)


def test_fallback_counts_by_default_and_raises_when_strict(clean_counter):
    assert F_.strict_kernels is False and F_.own_head_nn is True
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        F_._note_torch_fallback("head_dgrad", (8, 16), (16, 4))
        F_._note_torch_fallback("head_dgrad", (8, 16), (16, 4))
    assert F_.torch_fallbacks == {"head_dgrad": 2}
    assert len(caught) == 1 and "head_dgrad" in str(caught[0].message)      # warned once per op
    F_.strict_kernels = True
    with pytest.raises(RuntimeError, match=r"head_dgrad.*\(8, 16\).*\(16, 4\)"):
        F_._note_torch_fallback("head_dgrad", (8, 16), (16, 4))
    assert F_.torch_fallbacks == {"head_dgrad": 2}                          # an error is not a count


def test_parser_accepts_strict_kernels():
    from dltb.harness import build_parser
    base = ["--strategy", "ddp", "--tier", "tiny", "--seq-len", "32", "--steps", "2", "--per-device-batch", "1",
            "--grad-accum", "1", "--results-dir", "r"]
    assert build_parser().parse_args(base).strict_kernels is False
    assert build_parser().parse_args(base + ["--strict-kernels"]).strict_kernels is True


@pytest.mark.parametrize("flag", [True, False], ids=["strict", "default"])
def test_harness_sidecar_records_strict_kernels(tmp_path, clean_counter, flag):
    from dltb.harness import main
    os.environ.pop("WORLD_SIZE", None)
    main(["--strategy", "ddp", "--tier", "tiny", "--seq-len", "32", "--steps", "3", "--warmup-steps", "1",
          "--per-device-batch", "1", "--grad-accum", "2", "--results-dir", str(tmp_path / "res"), "--device", "cpu"]
         + (["--strict-kernels"] if flag else []))
    ext = [f for f in os.listdir(tmp_path / "res") if f.endswith(".extended.json")]
    side = json.loads((tmp_path / "res" / ext[0]).read_text())
    assert side["strict_kernels"] is flag
    assert side["torch_gemm_fallbacks"] is None          # CPU products are not fallbacks
    assert F_.strict_kernels is False                    # the flag holds for its run only
