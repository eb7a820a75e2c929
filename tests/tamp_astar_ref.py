"""Python restatement of MapShelfDomainTampRRT::plan(.., TampSearch::AStar) (plan_astar, src/map_shelves_tamp_rrt.rs:432-563): the
yardstick of the device planner (porrt_tamp_rrt_plan_astar, Engine.plan_tamp_rrt_astar).

TEST INFRASTRUCTURE ONLY, built on the CPU oracle through the helpers of tests/tamp_rrt_ref.py.  Never imported by the product.

The reference's loop: pop the node of lowest priority; one child per remaining zone IN ORDER (no shuffle is drawn), two RRT* queries
per child, priority = expected cost + reaching probability * heuristic; the first popped node without remaining zones is the solution.

Ours, not the reference's (its Priority::cmp never says Equal, common.rs:235-239):
  - bit-equal priorities pop in ascending search node id; ids are given in the sequential order -- a node's children get the next
    ids, in zone order, at the moment the node is popped; +0.0 and -0.0 are equal;
  - a prior with an entry that is not > 0 is refused.

Stream modes as in tamp_rrt_ref.py.  With streams = 1 a node's cost and priority are functions of its zone prefix alone, which allows
speculation: when the top of the queue has no computed children, it and the next best non-leaf entries without children (up to
`wave`) are expanded together; their children enter the queue only when their parent is popped in the replay.  A failed query
fails the plan only when its parent is popped.
"""
import heapq
import math

import numpy as np

import tamp_rrt_ref as R
from tamp_rrt_ref import NoPath          # noqa: F401  (re-exported for the tests)


def norm2(a, b):
    """common.rs:203-213"""
    d2 = 0.0
    for xa, xb in zip(a, b):
        dx = xb - xa
        d2 += dx * dx
    return math.sqrt(d2)


class Planner(R.Planner):
    """plan_astar on one oracle context.  `query(start, which, zone, p, prefix)` -> (path, cost) or None replaces the oracle's RRT*
    (a test stubs failures with it); the default is the Planner's own _query."""

    def plan(self, start, belief, max_step=0.1, search_radius=2.0, n_iter_min=2500, n_iter_max=10000, K=128, streams=1, wave=1,
             query=None):
        o = self.o
        nz = o.n_zones()
        if len(belief) != nz or not R.check_belief_state(belief):
            raise ValueError("invalid prior")
        if not all(float(b) > 0.0 for b in belief):
            raise ValueError("a prior entry that is not > 0")
        p = dict(max_step=max_step, search_radius=search_radius, n_iter_min=n_iter_min, n_iter_max=n_iter_max, K=K)
        if query is None:
            def query(st, which, zone, p, prefix):
                return self._query(st, which, zone, p)
        if streams == 0:
            wave = 1
            o.set_sampler(self.low, self.up, self.seed)
        zone_pos = [(float(z[0]), float(z[1])) for z in o.zone_positions()]
        start = (float(start[0]), float(start[1]))
        root = dict(id=0, target=None, parent=None, remaining=list(range(nz)), obs_state=start, path_obs=[], path_pick=[], rp=1.0,
                    belief=[float(x) for x in belief], ec=0.0, priority=0.0, prefix=(), kids=None, popped=False)
        nodes = [root]
        queue = [(0.0, 0)]
        stats = dict(queries=0, waves=0, speculated=0)

        def expand(u):
            vb = list(u["belief"])
            if u["target"] is not None:
                vb[u["target"]] = 0.0
            vb = R.normalize(vb)
            rp = u["rp"] * R.transition_probability(u["belief"], vb)
            kids = []
            for t in u["remaining"]:
                v = dict(target=t, parent=u["id"], remaining=[z for z in u["remaining"] if z != t], rp=rp, belief=vb,
                         prefix=u["prefix"] + (t,), kids=None, popped=False, fail=None)
                kids.append(v)
                if streams == 1:
                    o.set_sampler(self.low, self.up, R.edge_seed(self.seed, v["prefix"]))
                r = query(u["obs_state"], "observation", t, p, v["prefix"])
                stats["queries"] += 1
                if r is None:
                    v["fail"] = "observation"
                    if streams == 0:
                        break                    # the sequential loop ends here: this node is being popped
                    continue
                v["path_obs"], v["obs_cost"] = r
                v["obs_state"] = (float(r[0][-1][0]), float(r[0][-1][1]))
                r = query(v["obs_state"], "pickup", t, p, v["prefix"])
                stats["queries"] += 1
                if r is None:
                    v["fail"] = "pickup"
                    if streams == 0:
                        break
                    continue
                v["path_pick"], v["pick_cost"] = r
                v["ec"] = u["ec"] + rp * (v["obs_cost"] + vb[t] * v["pick_cost"])
                h = 0.0
                for z in v["remaining"]:
                    h = h + vb[z] * norm2(v["obs_state"], zone_pos[z])
                v["priority"] = v["ec"] + rp * h
            u["kids"] = kids

        solution = None
        try:
            while solution is None and queue:
                # replay: pops while the top is a leaf or has its children
                while queue:
                    u = nodes[queue[0][1]]
                    if u["remaining"] and u["kids"] is None:
                        break
                    heapq.heappop(queue)
                    u["popped"] = True
                    for v in u["kids"] or []:
                        if v["fail"] is not None:
                            raise NoPath(len(nodes), v["target"], v["fail"])
                        v["id"] = len(nodes)
                        nodes.append(v)
                        heapq.heappush(queue, (v["priority"], v["id"]))
                    if not u["remaining"]:
                        solution = u
                        break
                if solution is not None or not queue:
                    break
                batch = []
                for _, uid in sorted(queue):
                    u = nodes[uid]
                    if u["remaining"] and u["kids"] is None:
                        batch.append(u)
                        if len(batch) == wave:
                            break
                stats["waves"] += 1
                for u in batch:
                    expand(u)
        finally:
            if streams == 0:
                o.set_sampler(self.low, self.up, self.seed)
        if solution is None:
            raise RuntimeError("No solution found!")
        stats["speculated"] = sum(1 for n in nodes if n["kids"] is not None and not n["popped"])
        stats["failed_speculated"] = sum(1 for n in nodes if n["kids"] is not None and not n["popped"]
                                         for v in n["kids"] if v["fail"] is not None)
        chain = []
        n = solution
        while n is not None:
            chain.append(n)
            n = nodes[n["parent"]] if n["parent"] is not None else None
        chain.reverse()
        pol = R.build_policy(o, chain)
        pol.update(search_cost=solution["ec"], zone_order=list(solution["prefix"]), search_nodes=len(nodes),
                   node_parents=np.array([-1 if n["parent"] is None else n["parent"] for n in nodes], dtype=np.int64),
                   node_targets=np.array([-1 if n["target"] is None else n["target"] for n in nodes], dtype=np.int32),
                   node_ec=np.array([n["ec"] for n in nodes], dtype=np.float64),
                   node_priority=np.array([n["priority"] for n in nodes], dtype=np.float64), **stats)
        return pol
