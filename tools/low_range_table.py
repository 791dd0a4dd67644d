"""profiles/low_range_parity.txt from two runs of tests/test_gpu_low_range.py with -s (one on the parent commit's library, one on this
tree's): one table per case and k -- the fp32 oracle's error, the GPU's error before and after, the bound, and which kernels ran.
    SCANN_HIP_LIB=<the parent commit's libscann_hip.so> python -m pytest tests/test_gpu_low_range.py -s > parent.log
    python -m pytest tests/test_gpu_low_range.py -s > new.log
    python tools/low_range_table.py parent.log new.log > profiles/low_range_parity.txt
(a library without scann_weights_exact is never exact: Engine.weights_exact() is then False and the test goes on to print its figures)"""
import sys


def read(path):
    out, order = {}, []
    for line in open(path):
        if not line.lstrip(".FEsx").startswith("LOWRANGE |"):
            continue
        _, label, name, e32, gpu, bound, how = [f.strip() for f in line.split("|")]
        if label not in out:
            out[label] = {}
            order.append(label)
        out[label].setdefault(name, (float(e32.split()[1]), float(gpu.split()[1]), float(bound.split()[1]), how))
    return out, order


def main():
    old, _ = read(sys.argv[1])
    new, order = read(sys.argv[2])
    print(__doc__.split("\n")[0].replace("profiles/low_range_parity.txt from", "From") + " ...")
    print("Errors are rel_err (tests/test_gpu_parity.py) against the fp64 oracle; bound = max(1e-4, 2 x fp32 oracle).  'before' is the parent\n"
          "commit's library, named through SCANN_HIP_LIB (always the split-fp16 kernels), 'after' this commit's; 'exact' = the handle was sent to the exact-fp32 kernels\n"
          "when its weights were loaded (no forward is run twice: scann_exact_reruns stays 0).  '-' = not reported: per-layer tensors come\n"
          "from a debug forward, which an exact handle refuses.  '<<' marks a figure outside its bound.\n")
    print("Summary: the worst tensor of each case (error / bound).  A case inside its bound on the parent commit is kept as a regression test.")
    print("  %-42s %-30s %-30s %s" % ("case", "before", "after", "after ran"))
    for label in order:
        def worst(d):
            if not d:
                return "-"
            n = max(d, key=lambda t: d[t][1] / d[t][2])
            return "%-18s %.2e%s" % (n, d[n][1], "<<" if not d[n][1] <= d[n][2] else "  ")
        print("  %-42s %-30s %-30s %s" % (label, worst(old.get(label)), worst(new[label]), next(iter(new[label].values()))[3]))
    print()
    for label in order:
        print("== %s ==" % label)
        print("  %-18s %10s %10s %10s %10s  %s" % ("tensor", "fp32", "before", "after", "bound", "after ran"))
        names = list(new[label]) + [n for n in old.get(label, {}) if n not in new[label]]
        for n in names:
            a, b = new[label].get(n), old.get(label, {}).get(n)
            e32, bound = (a or b)[0], (a or b)[2]
            cell = lambda r: "-" if r is None else "%.2e%s" % (r[1], "<<" if not r[1] <= r[2] or "NOT FINITE" in r[3] else "")
            print("  %-18s %10.2e %10s %10s %10.2e  %s" % (n, e32, cell(b), cell(a), bound, a[3] if a else new[label][names[0]][3]))
        print()


if __name__ == "__main__":
    main()
