#!/usr/bin/env python3
"""Crystals whose neighbour lists repeat an atom and point at the atom itself (tests/crystal_batches.py) on every GPU path, per
comparison of tests/test_gpu_crystal.py:
    python tools/crystal_parity.py [out.txt [pytest options]]
Runs that module's tests in this process (needs the GPU) and prints (and writes) what they measured: per case and tensor or output the
error against the fp64 reference, the fp32 reference's own error against it (nan where the rule has none) and the bound."""
import os, sys
import pytest
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_gpu_crystal.py")] + sys.argv[2:])
t = sys.modules["test_gpu_crystal"]
ratios = [float(l.split()[-3]) / float(l.split()[-1]) for l in t.PARITY_LINES]
lines = [t.HEADER] + t.PARITY_LINES
lines.append("pytest exit status %d; %d comparisons, worst error / bound %.2f" % (rc, len(ratios), max(ratios or [float("nan")])))
print("\n".join(lines))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
sys.exit(int(rc))
