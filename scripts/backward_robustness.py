#!/usr/bin/env python
"""Markdown tables of the rounding errors of every filter-gradient route and every input-gradient launch of the wide 2-D layers against
float64, on the hostile statistics of tests/test_gpu_backward_robust.py (same seeds, same cases).
    python scripts/backward_robustness.py > profiles/backward_robustness.md     (needs the GPU)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts import robust_util as RU  # noqa: E402


def main():
    B, H, W = RU.BACKWARD_MAP
    print("# Backward of the wide 2-D layers on hostile statistics\n")
    print("Errors are max|got - float64| / max|float64| over the whole tensor; B = %d, map %d x %d; bar %.0e, purely relative." % (B, H, W, RU.GRAD_BAR))
    print("`s` = the bf16x3 multiply stage, `h` = fp16x2 (one power-of-two scale per tensor), no suffix = exact fp32.\n")
    worst = {}
    for layer, (k, _cin, _cout) in RU.BACKWARD_LAYERS.items():
        routes = RU.WGRAD_ROUTES[k]
        print("## %s: filter gradient\n" % layer)
        print("| x | dz | " + " | ".join(routes) + " |")
        print("|---|---|" + "---|" * len(routes))
        for x_name in RU.backward_inputs(layer)[0]:
            errs = RU.measure_filter_gradient(layer, x_name)
            for dz_name in RU.backward_inputs(layer)[2]:
                print("| %s | %s | " % (x_name, dz_name) + " | ".join("%.2e" % errs[(r, dz_name)] for r in routes) + " |", flush=True)
                for r in routes:
                    worst[("dw", layer, r)] = max(worst.get(("dw", layer, r), 0.0), errs[(r, dz_name)])
        schemes = RU.DGRAD_SCHEMES[k]
        errs = RU.measure_input_gradient(layer)
        print("\n## %s: input gradient\n" % layer)
        print("| dz | " + " | ".join(schemes) + " |")
        print("|---|" + "---|" * len(schemes))
        for dz_name in RU.backward_inputs(layer)[2]:
            print("| %s | " % dz_name + " | ".join("%.2e" % errs[(s, dz_name)][0] for s in schemes) + " |")
            for s in schemes:
                worst[("dx", layer, s)] = max(worst.get(("dx", layer, s), 0.0), errs[(s, dz_name)][0])
        print("\nPer image, against that image's own max|float64| (image 0 carries the gain where there is one):\n")
        print("| dz | " + " | ".join(schemes) + " |")
        print("|---|" + "---|" * len(schemes))
        for dz_name in RU.backward_inputs(layer)[2]:
            print("| %s | " % dz_name + " | ".join(" / ".join("%.2e" % e for e in errs[(s, dz_name)][1]) for s in schemes) + " |")
        print()
    print("## Worst per route\n")
    print("| gradient | layer | route | worst | above half the bar |")
    print("|---|---|---|---|---|")
    for (what, layer, r), e in worst.items():
        print("| %s | %s | %s | %.2e | %s |" % (what, layer, r, e, "YES" if e > RU.GRAD_BAR / 2 else ""))


if __name__ == "__main__":
    main()
