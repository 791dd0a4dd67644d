#!/usr/bin/env python3
"""Exactness of the leave-one-out contributions (y - ablated) on the GPU against the fp32 NumPy oracle, per fixture of
tests/test_gpu_ablate.py, both measured against the fp64 oracle on the GPU's own after_Lc rows:
    python tools/ablate_parity.py [out.txt]
Prints (and writes) the GPU's rel_err, the oracle's and their ratio per fixture; tests/test_gpu_ablate.py's CONTRIB_F is twice the
worst ratio, rounded up."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
import test_gpu_ablate as t
lines = ["fixture            rel_err(c_gpu, c64)  rel_err(c32, c64)  ratio   (leave-one-out contributions, GPU's own after_Lc rows)"]
worst = 0.0
for case in t.CASES:
    e_gpu, e_32 = t.contribution_errors(case)
    ratio = e_gpu / max(e_32, 1e-30)
    worst = max(worst, ratio)
    lines.append("%-18s %-20.3e %-18.3e %.2f" % (case, e_gpu, e_32, ratio))
lines.append("worst ratio %.2f" % worst)
print("\n".join(lines))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
