"""Developer probe (a library built with -DPORRT_TIMING=5, see tools/riders_probe.sh): how long each workgroup of k_conn2_riders takes.

  python tools/riders_probe.py [Q] [riders_fast values, default "0 1"]

Q configs[1] queries (seeds differ) in ONE launch sequence (batch_streams = 1: the riders run with nothing beside them), K = 1024.  Per row the
kernel leaves the sum of each role's durations over the steps of three windows (Counters::tim): the first eight steps, the later steps
before a copy of the goal point is on the goal path, the steps after.  Printed: the mean and the maximum over the rows of a role's mean
duration per step, per window.  The kernel's length at a step is the maximum over the roles.
"""
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np
import cases, po_rrt_amd

Q = int(sys.argv[1]) if len(sys.argv) > 1 else 128
forms = [int(a) for a in sys.argv[2:]] or [0, 1]
ROLES = ["0 page filing", "1 goal copies", "2 goal path"]
WINDOWS = ["steps 1-8", "later, before the first goal copy", "after the first goal copy"]
case = cases.cfg2(111500)
for fast in forms:
    engs = [cases.configure(po_rrt_amd.Engine(0), case) for _ in range(Q)]
    for j, e in enumerate(engs):
        e.set_sampler((-1.0, -1.0), (1.0, 1.0), j)
        e.set_option("batch_streams", 1)
        e.set_option("riders_fast", fast)
    po_rrt_amd.Engine.grow_batch(engs, [case.start] * Q, case.max_step, case.search_radius, case.n_iter_min, 1024)
    tim = np.array([[e.get_option("tim%d" % i) for i in range(12)] for e in engs], dtype=np.float64)
    if not tim[:, 9:12].any():
        sys.exit("no timers: build the library with -DPORRT_TIMING=5 (tools/riders_probe.sh)")
    print("riders_fast = %d, %d rows, one sequence; us per step, mean over rows / max over rows" % (fast, Q))
    for w, wn in enumerate(WINDOWS):
        steps = tim[:, 9 + w]
        rows = steps > 0
        print("  %s: %.1f steps per row on average, %d rows with such steps" % (wn, steps.mean(), rows.sum()))
        if not rows.any():
            continue
        per = [1e-2 * tim[rows, 3 * r + w] / steps[rows] for r in range(3)]
        for r, rn in enumerate(ROLES):
            print("    role %-14s mean %6.1f  max %6.1f" % (rn, per[r].mean(), per[r].max()))
        longest = np.max(np.stack(per), axis=0)
        print("    longest role      mean %6.1f  max %6.1f   (a bound from below on the kernel: per-step maxima are not kept)" % (longest.mean(), longest.max()))
