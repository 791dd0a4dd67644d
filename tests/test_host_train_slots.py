"""The training backward's slot bookkeeping (csrc/scann_train_slots.h) on the host, no GPU.

`make -C scann--material_amd/csrc asan-train` compiles csrc/scann_train_check.cpp -- a stand-alone program, host code only -- under
AddressSanitizer + UBSan and runs it: the capped bump (consecutive regions and one reduce entry each, an exact fill, one float more sets
`overrun` and hands out nothing, the context stays overrun; wgrad_add through the same bump), every partition over row counts on both
sides of its switches (workgroups x rows per workgroup cover the rows; the count is the one the launcher's former expression gives), and
det_slot_floats / wpart_slot_floats against the sums they replaced."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slot_bookkeeping_under_asan_and_ubsan():
    csrc = os.path.join(ROOT, "scann--material_amd", "csrc")
    r = subprocess.run(["make", "--no-print-directory", "-C", csrc, "asan-train"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "scann_train_check: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
