#!/bin/bash
# Same-box A/B of `smooth(sol)`: another commit of this repository against this tree, alternating processes, so that what the
# bridges of the default dense="marginal" cost shows against the run-to-run spread of the other commit itself.  A library of
# another commit cannot be swapped in through PNMOL_HIP_LIB as tools/ab_bench.sh does for the step (the binding declares every
# symbol of its own header), so the other side is a whole tree:
#     git archive PARENT | tar -x -C /some/dir && (cd /some/dir && python __graft_entry__.py)
# usage (on the GPU box, from the repository root): bash tools/ab_smooth.sh /some/dir [N] [STEPS] [ROUNDS]
# One JSON line per run ("tree": parent / new), as in profiles/dense/bench_dense.jsonl.
other=$1; N=${2:-256}; steps=${3:-100}; rounds=${4:-3}
here=$(cd "$(dirname "$0")/.." && pwd)
for i in $(seq $rounds); do
  timeout -k 10 300 python "$here/tools/bench_smooth_ab.py" "$other" $N $steps parent || exit 1
  timeout -k 10 300 python "$here/tools/bench_smooth_ab.py" "$here" $N $steps new || exit 1
done
