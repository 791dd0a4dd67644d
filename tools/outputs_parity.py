#!/usr/bin/env python3
"""The selected inference outputs (attention maps, after_Lc, bf_property) at size against the NumPy fp64 oracle, per oracle case of
tests/test_gpu_output_sizes.py (64-row edge tiles, 64-row atom tiles, the general embedding, exact fp32, plain fp32):
    python tools/outputs_parity.py [out.txt [pytest options]]
Runs that module's tests in this process (needs the GPU) and prints (and writes) what they measured: per case and output
rel_err(gpu, fp64) and its bound max(RTOL, 2 rel_err(fp32 oracle, fp64))."""
import os, sys
import pytest
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_gpu_output_sizes.py")] + sys.argv[2:])
t = sys.modules["test_gpu_output_sizes"]
lines = ["%-40s %-18s %-12s %s" % ("case", "output", "rel_err", "bound")] + t.PARITY_LINES
lines.append("pytest exit status %d; worst rel_err / bound %.2f" % (rc, max([float(l.split()[-2]) / float(l.split()[-1]) for l in t.PARITY_LINES] or [float("nan")])))
print("\n".join(lines))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
sys.exit(int(rc))
