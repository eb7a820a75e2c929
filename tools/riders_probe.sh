#!/bin/bash
# developer probe (GPU box): the duration of each role of k_conn2_riders (page filing, goal copies, goal path), per window of steps, mean and
# maximum over the rows of Q queries in one sequence, with riders_fast = 0 and = 1 of the same library
#   bash tools/riders_probe.sh [Q] [extra compiler flags]
Q=${1:-128}
PORRT_CXXFLAGS="-DPORRT_TIMING=5 $2" python -c "from po_rrt_amd import build as b; b.build(force=True)" > /dev/null 2>&1 || exit 1
timeout -k 10 300 python tools/riders_probe.py $Q 0 1
python -c "from po_rrt_amd import build as b; b.build(force=True)" > /dev/null 2>&1
