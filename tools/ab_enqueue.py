#!/usr/bin/env python3
"""A/B of two builds of the library where only the host's enqueue time can differ (a change to the launch schedule's host code):
    python tools/ab_enqueue.py <reps> <parent lib> <new lib> [bench] [tools]
Alternates the two builds (SCANN_HIP_LIB) inside one call, `reps` times each and in turns first, over the launch-bound measurements -- `bench`: bench.py
--no-extras (as tools/ab_libs.sh) and its legs one_batch_per_launch and training_step; `tools`: tools/models_rate.py and tools/mc_rate.py --
and prints every repetition, the medians, the parent's min-to-max spread, and whether the new build's median is worse than the parent's
by more than that spread.  Stops at the first command that fails."""
import json, os, re, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
reps, libs, groups = int(sys.argv[1]), [os.path.abspath(p) for p in sys.argv[2:4]], sys.argv[4:] or ["bench", "tools"]
PY, BENCH = sys.executable, os.path.join(ROOT, "bench.py")


def bench_value(out):
    return {"molecules/s": json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])["value"]}


def models_rate(out):  # wall time per call of K forwards on one handle (a) and of the model set (c), per shape
    return {"%s %s us" % (shape, way): float(us) for shape, a, c in re.findall(r"^(\d+ x \d+) structures.*?one handle (\d+) us.*?model set (\d+) us", out, re.M)
            for way, us in (("(a) 5 forwards", a), ("(c) model set", c))}


def mc_rate(out):
    return {"%s %s ms" % (shape, what): float(ms) for shape, mc, fw in re.findall(r"^(\d+ x \d+) structures.*?: ([\d.]+) ms per MC sample, ([\d.]+) ms per plain", out, re.M)
            for what, ms in (("MC sample", mc), ("plain forward", fw))}


RUNS = {"bench": [("bench.py --no-extras --steps 800", [PY, BENCH, "--no-extras", "--steps", "800"], bench_value, True),
                  ("bench.py --leg one_batch_per_launch", [PY, BENCH, "--leg", "one_batch_per_launch"], bench_value, True),
                  ("bench.py --leg training_step", [PY, BENCH, "--leg", "training_step"], bench_value, True)],
        "tools": [("tools/models_rate.py", [PY, os.path.join(ROOT, "tools", "models_rate.py")], models_rate, False),
                  ("tools/mc_rate.py", [PY, os.path.join(ROOT, "tools", "mc_rate.py")], mc_rate, False)]}
for title, cmd, parse, higher_is_better in [r for g in groups for r in RUNS[g]]:
    got = [{}, {}]
    for rep in range(reps):
        for i in ((0, 1), (1, 0))[rep % 2]:  # (parent first, then new first: neither build always runs on the warmer device)
            lib = libs[i]
            r = subprocess.run(cmd, env=dict(os.environ, SCANN_HIP_LIB=lib), capture_output=True, text=True, timeout=300, cwd=ROOT)
            vals = parse(r.stdout) if r.returncode == 0 else {}
            if not vals:
                sys.exit("%s failed with %s (rc %d): %s" % (title, os.path.basename(lib), r.returncode, r.stderr[-1500:]))
            for k, v in vals.items():
                got[i].setdefault(k, []).append(v)
            print("%-38s rep %d  %-26s %s" % (title, rep + 1, os.path.basename(lib), "  ".join("%s %.6g" % kv for kv in vals.items())), flush=True)
    for k in got[0]:
        p, n = got[0][k], got[1][k]
        mp, mn, spread = statistics.median(p), statistics.median(n), max(p) - min(p)
        worse = (mp - mn) if higher_is_better else (mn - mp)
        print("== %s, %s: parent median %.6g (min %.6g, max %.6g, spread %.3g), new median %.6g (min %.6g, max %.6g): new is %s by %.3g = %.2f %% -> %s"
              % (title, k, mp, min(p), max(p), spread, mn, min(n), max(n), "worse" if worse > 0 else "better", abs(worse), 100 * abs(worse) / mp,
                 "REGRESSION (beyond the parent's spread)" if worse > spread else "within the parent's spread" if worse > 0 else "ok"), flush=True)
