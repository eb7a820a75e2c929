"""Python restatement of MapShelfDomainTampRRT::plan(.., TampSearch::BranchAndBoundMultipleViewPoints)
(src/map_shelves_tamp_rrt.rs:293-430) with the viewpoints of a query walked in ascending node id: the yardstick of
porrt_tamp_rrt_plan_viewpoints / Engine.plan_tamp_rrt_viewpoints.

TEST INFRASTRUCTURE ONLY, built on the CPU oracle and the helpers of tamp_rrt_ref; never imported by the product package.

streams = 0  one continuous stream: per (node, zone) the observation query, then the pickup queries of its viewpoints in order
streams = 1  the observation query of (u, t) on a stream seeded ho = splitmix64(u.h ^ (t + 1)) (root h = the sampler seed), the pickup
             query of the viewpoint of rank j on h = splitmix64(ho ^ ((j + 1) << 32)), which is the child's h
wave: up to `wave` nodes are popped at once, all their queries run, then the children are pushed and the leaves recorded in the
sequential order.  wave = 1 is the reference's loop.
max_viewpoints: 0 = all (the reference); n > 0 = per observation query the n solutions of lowest cost (ties: lower id), walked in
ascending id.
"""
import math

import numpy as np

import solutions_ref
import tamp_rrt_ref as R
from oracle import orc

M64 = R.M64


class NoLeaf(RuntimeError):
    """expect("No solution found!") (:423): the search ended without a leaf"""


def keep(sols, max_viewpoints):
    if max_viewpoints and len(sols) > max_viewpoints:
        order = sorted(range(len(sols)), key=lambda k: (sols[k][2], sols[k][0]))[:max_viewpoints]
        return [sols[k] for k in sorted(order)]
    return list(sols)


class Planner:
    def __init__(self, o, seed, low=(-1.0, -1.0), up=(1.0, 1.0), goal_radius=0.05):
        self.o, self.seed, self.low, self.up, self.goal_radius = o, seed, low, up, goal_radius
        self.drng = orc.Pcg64.seed_from_u64(seed)

    def _grow(self, start, goal, zone, p):
        o = self.o
        if goal == "observation":
            o.set_observation_goal(zone)
        else:
            zp = o.zone_positions()[zone]
            o.set_square_goal(np.array([zp]), np.array([1], dtype=np.uint64), self.goal_radius)
        o.grow(start, p["max_step"], p["search_radius"], p["n_iter_min"], p["n_iter_max"], batch_K=p["K"], algo=orc.ALGO_BATCHED_KD)

    def plan(self, start, belief, max_step=0.1, search_radius=2.0, n_iter_min=2500, n_iter_max=10000, K=128, streams=1, wave=1,
             max_viewpoints=0):
        o = self.o
        nz = o.n_zones()
        if len(belief) != nz or not R.check_belief_state(belief):
            raise ValueError("invalid prior")
        p = dict(max_step=max_step, search_radius=search_radius, n_iter_min=n_iter_min, n_iter_max=n_iter_max, K=K)
        if streams == 0:
            wave = 1
            o.set_sampler(self.low, self.up, self.seed)
        start = (float(start[0]), float(start[1]))
        root = dict(id=0, target=None, parent=None, remaining=R.shuffled(range(nz), self.drng), obs_state=start, path_obs=[],
                    path_pick=[], rp=1.0, belief=[float(x) for x in belief], ec=0.0, prefix=(), ranks=(), h=self.seed & M64)
        nodes = [root]
        stack = [0]
        best = math.inf
        best_leaf = None
        leaf_costs = []
        stats = dict(queries=0, waves=0, pruned=0, observation_queries=0, pickup_queries=0, viewpoints_found=0, viewpoints_kept=0)
        viewpoint_counts = []                                  # per observation query, in the sequential order
        while stack:
            popped = [stack.pop() for _ in range(min(wave, len(stack)))]
            stats["waves"] += 1
            made = []
            for uid in popped:
                u = nodes[uid]
                kids = []
                for t in u["remaining"]:
                    rem = [z for z in R.shuffled(u["remaining"], self.drng) if z != t]      # one shuffle per zone, not per viewpoint
                    vb = list(u["belief"])
                    if u["target"] is not None:
                        vb[u["target"]] = 0.0
                    vb = R.normalize(vb)
                    rp = u["rp"] * R.transition_probability(u["belief"], vb)
                    ho = R.splitmix64(u["h"] ^ (int(t) + 1))
                    if streams == 1:
                        o.set_sampler(self.low, self.up, ho)
                    self._grow(u["obs_state"], "observation", t, p)
                    stats["queries"] += 1
                    stats["observation_queries"] += 1
                    sols = solutions_ref.of_oracle(o)
                    kept = keep(sols, max_viewpoints)
                    viewpoint_counts.append(len(sols))
                    stats["viewpoints_found"] += len(sols)
                    stats["viewpoints_kept"] += len(kept)
                    for j, (_, path, cost) in enumerate(kept):
                        h = R.splitmix64(ho ^ (((j + 1) << 32) & M64))
                        end = (float(path[-1][0]), float(path[-1][1]))
                        if streams == 1:
                            o.set_sampler(self.low, self.up, h)
                        self._grow(end, "pickup", t, p)
                        stats["queries"] += 1
                        stats["pickup_queries"] += 1
                        r = o.best_solution()
                        if r is None:
                            raise R.NoPath(len(nodes), t, "pickup")
                        v = dict(id=len(nodes), target=t, parent=uid, remaining=rem, rp=rp, belief=vb, prefix=u["prefix"] + (t,),
                                 ranks=u["ranks"] + (j,), h=h, path_obs=path, obs_cost=cost, obs_state=end, path_pick=r[0], pick_cost=r[1])
                        nodes.append(v)
                        kids.append(v)
                made.append((u, kids))
            for u, kids in made:
                for v in kids:
                    v["ec"] = u["ec"] + v["rp"] * (v["obs_cost"] + v["belief"][v["target"]] * v["pick_cost"])
                    if v["ec"] < best:
                        stack.append(v["id"])
                    else:
                        stats["pruned"] += 1
                if not u["remaining"]:
                    leaf_costs.append(u["ec"])
                    if u["ec"] < best:
                        best = u["ec"]
                    if best_leaf is None or u["ec"] <= best_leaf["ec"]:
                        best_leaf = u
        if streams == 0:
            o.set_sampler(self.low, self.up, self.seed)
        if best_leaf is None:
            raise NoLeaf("No solution found!")
        chain = []
        n = best_leaf
        while n is not None:
            chain.append(n)
            n = nodes[n["parent"]] if n["parent"] is not None else None
        chain.reverse()
        pol = R.build_policy(o, chain)
        pol.update(search_cost=best_leaf["ec"], zone_order=list(best_leaf["prefix"]), viewpoint_ranks=list(best_leaf["ranks"]),
                   search_nodes=len(nodes), viewpoint_counts=viewpoint_counts, largest_set=max(viewpoint_counts, default=0),
                   leaf_costs=sorted(leaf_costs), **stats)
        return pol
