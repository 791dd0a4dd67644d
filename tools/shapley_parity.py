#!/usr/bin/env python3
"""Exactness of the sampled Shapley values on the GPU against the fp32 NumPy oracle, per fixture of tests/test_gpu_shapley.py, both measured
against the fp64 oracle on the GPU's own after_Lc rows and walks; and of the exact enumerations on the tiny structures against the subset
formula:
    python tools/shapley_parity.py [out.txt]
Prints (and writes) the GPU's rel_err, the oracle's and their ratio per fixture; tests/test_gpu_shapley.py's SHAPLEY_F is twice the worst
ratio, rounded up."""
import math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
import test_gpu_shapley as t
lines = ["fixture                  rel_err(phi_gpu, phi64)  rel_err(phi32, phi64)  ratio   (%d walks per structure, GPU's own after_Lc rows and walks)" % t.P_TEST]
worst = 0.0
for label, fn, cases in (("", t.shapley_errors, list(t.CASES)), (" all n! walks", t.exact_errors, ["sizes", "sizes_no_ga_norm"])):
    for case in cases:
        e_gpu, e_32 = fn(case)
        ratio = e_gpu / max(e_32, 1e-30)
        worst = max(worst, ratio)
        lines.append("%-24s %-24.3e %-22.3e %.2f" % (case + label, e_gpu, e_32, ratio))
lines.append("worst ratio %.2f -> SHAPLEY_F = %d" % (worst, max(1, math.ceil(2 * worst))))
print("\n".join(lines))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
