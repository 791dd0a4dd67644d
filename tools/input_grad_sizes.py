#!/usr/bin/env python3
"""Input gradients on every variant of the backward the call can take, per comparison of tests/test_gpu_input_grad_sizes.py:
    python tools/input_grad_sizes.py [out.txt [pytest options]]
Runs that module's tests in this process (needs the GPU) and prints (and writes) what they measured: per case and leaf the worst error
against fp64 autograd under the batch's normalisation, the torch-fp32 graph's own error, the bound, and the worst structure's error over
its own bound under its own normalisation (nan where the comparison has none)."""
import os, sys
import pytest
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_gpu_input_grad_sizes.py")] + sys.argv[2:])
t = sys.modules["test_gpu_input_grad_sizes"]
lines = [t.HEADER] + t.PARITY_LINES
lines.append("pytest exit status %d; %d comparisons, worst error / bound %.2f, worst structure's error / its bound %.2f" % (
    rc, len(t.RATIOS), max([a for a, _ in t.RATIOS] or [float("nan")]), max([b for _, b in t.RATIOS if b == b] or [float("nan")])))
print("\n".join(lines))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
sys.exit(int(rc))
