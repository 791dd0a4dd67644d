#!/bin/bash
# Atom-tile heights against each other on ONE box (launch_atom's thresholds, scann_kernels.hip): ms of atom launches per forward
# (scann_forward_profile) and molecules/s for every SCANN_ATOM_ROWS of <rows list> at every --group of <group list>, eight launch groups
# each.  A run that fails ends the sweep.  Lines are appended to <out file> (profiles/atom_rows_sweep.txt is four passes).
#   tools/atom_rows_sweep.sh <out file> "<rows list>" "<group list>"      e.g.  tools/atom_rows_sweep.sh sweep.txt "32 64 96" "8 10 12 14 16"
root=$PWD
out=$1
mkdir -p "$(dirname "$out")"
for g in $3; do
  for rows in $2; do
    line=$(SCANN_ATOM_ROWS=$rows timeout -k 10 120 python3 $root/bench.py --no-extras --steps $((8 * g)) --warmup $g --group $g --prewarm 0.3) || { echo "group $g rows $rows: exit $?" | tee -a $out; exit 1; }
    echo "$line" | python3 -c "import sys,json; d=json.loads(sys.stdin.readline()); p=d['roofline']['per_forward_ms']; print('group %2d rows %3d  %9.0f molecules/s  atom %.4f ms  edge %.4f ms  total %.4f ms' % ($g, $rows, d['value'], p['ms_atom'], p['ms_edge'], p['ms_total']))" | tee -a $out || exit 1
  done
done
