#!/usr/bin/env python3
"""Monte Carlo dropout at size against the torch fp64 restatement, per oracle case of tests/test_gpu_mc_sizes.py (64-row edge tiles,
chunk tiles, 64-row atom tiles, the no-edge batch):
    python tools/mc_parity.py [out.txt [pytest options]]
Runs that module's tests in this process (needs the GPU) and prints (and writes) what they measured: per case and sample
rel_err(y_gpu, y64) and its bound max(RTOL, 2 rel_err(y32, y64)); per case the GA mean / std errors and their bound 10 RTOL."""
import os, sys
import pytest
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_gpu_mc_sizes.py")] + sys.argv[2:])
t = sys.modules["test_gpu_mc_sizes"]
lines = ["%-44s %-7s %-12s %s" % ("case", "sample", "rel_err", "bound")] + t.PARITY_LINES
lines.append("pytest exit status %d; worst rel_err / bound %.2f" % (rc, max([float(l.split()[-2]) / float(l.split()[-1]) for l in t.PARITY_LINES] or [float("nan")])))
print("\n".join(lines))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
sys.exit(int(rc))
