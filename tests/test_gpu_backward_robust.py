"""Rounding robustness of the BACKWARD of the wide 2-D layers on hostile statistics.  -m gpu.

tests/test_gpu_wino_robust.py feeds the forward what a trained net feeds it; every backward test feeds dz ~ N(0,1).  In training dz is
1e-6 .. 1e-9, sparse, and differs by orders of magnitude between the images of a batch.  Here the filter gradient and the input gradient
of 3x3 512 -> 512 and 4x4 512 -> 256 (B = 2, 24 x 24 map: ragged F(6x6) tiles) are measured against float64 on
scripts/robust_util.hostile_gradients crossed with the hostile activations of hostile_inputs:

  filter gradient: every route ops._launch_wgrad can be pinned to -- direct, wino2, wino43 / wino44, wino3l_split
  input gradient:  direct, F(2x2,3x3) / F(2x2,2x2)x4, F(4x4,3x3), F(6x6,3x3), F(4x4,4x4), the last three on the exact-fp32, bf16x3 and
                   fp16x2 multiply stage

Bar: the project's gradient bar, max|got - f64| <= 2e-4 * max|f64|, purely relative.  (The exact arithmetic alone is far inside it: the
F(4x4,3x3) filter-gradient identity emulated in fp32 NumPy on these statistics stays at 4e-6 of max|dw|, a plain fp32 reduction at 8e-7.)
With one image 2^20 above the other, the exact and bf16x3 stages work tile-locally, so EACH image's dx must meet the bar against its own
maximum; fp16x2 scales by one power of two per tensor (documented), so there only the whole tensor is held to the bar and the per-image
figure is printed.  Every figure is printed before anything is asserted; profiles/backward_robustness.md holds the table
(scripts/backward_robustness.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts import robust_util as RU  # noqa: E402

pytestmark = pytest.mark.gpu


def _x_names(layer):
    return list(RU.backward_inputs(layer)[0])


@pytest.mark.parametrize("xk", range(len(RU.X_CASES)))
@pytest.mark.parametrize("layer", list(RU.BACKWARD_LAYERS))
def test_filter_gradient_on_hostile_statistics(layer, xk):
    x_name = _x_names(layer)[xk]
    errs = RU.measure_filter_gradient(layer, x_name)
    for (route, dz_name), e in errs.items():
        print("dw %s | x: %s | dz: %s | %s: %.2e" % (layer, x_name, dz_name, route, e))
    bad = {k: e for k, e in errs.items() if not e <= RU.GRAD_BAR}
    assert not bad, bad


@pytest.mark.parametrize("layer", list(RU.BACKWARD_LAYERS))
def test_input_gradient_on_hostile_statistics(layer):
    errs = RU.measure_input_gradient(layer)
    bad = {}
    for (scheme, dz_name), (whole, per_image) in errs.items():
        print("dx %s | dz: %s | %s: %.2e  per image: %s" % (layer, dz_name, scheme, whole, " ".join("%.2e" % e for e in per_image)))
        if not whole <= RU.GRAD_BAR:
            bad[(scheme, dz_name)] = whole
        if dz_name.startswith("one image") and not scheme.endswith("h") and not max(per_image) <= RU.GRAD_BAR:
            bad[(scheme, dz_name, "per image")] = per_image
    assert not bad, bad
