#!/usr/bin/env python3
"""Batches whose tensors pass 2^31 bytes, up to the upload limit: what tests/test_gpu_large_rows.py measured per case.
    python tools/large_rows_record.py [out.txt [pytest arguments]]
Runs that module's tests in this process (needs the GPU; the first failure ends the run) -- or, with pytest arguments, whatever they
name, the module among it -- and prints (and writes) one line per case: atoms, edges, the largest tensor's shape and bytes, the wall
time of the case, the device memory its resident batch took (hipMemGetInfo before the upload minus after the last launch), and why it
skipped if it did (out of device memory is the only reason a case may skip for)."""
import os, sys
import pytest
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[2:] or ["-x", os.path.join(ROOT, "tests", "test_gpu_large_rows.py")]
rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider"] + args)
t = sys.modules["test_gpu_large_rows"]
skipped = sum("skipped:" in l for l in t.RECORD_LINES)
lines = list(t.RECORD_LINES) + ["pytest exit status %d; %d cases, %d skipped" % (rc, len(t.RECORD_LINES), skipped)]
print("\n".join(lines))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
sys.exit(int(rc))
