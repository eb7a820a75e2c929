"""Python restatement of RRT::get_solutions (src/rrt.rs:195-246): the yardstick of porrt_solutions / Engine.solutions().

TEST INFRASTRUCTURE ONLY, on the CPU oracle's tree (Oracle.tree(), Oracle.final_ids()).  Never imported by the product package.

The reference collects the "firstly final" node ids in a HashSet and returns them in its order, which is unspecified; here the set
is sorted: ascending node id, the order the device call promises.
"""
import math

import numpy as np


def firstly_final_ids(parent, final_ids):
    """get_firstly_final_node_ids (rrt.rs:229-246), literally: from every final node move up while the parent is final; a missing
    parent reads as id 0 (unwrap_or(0)).  Returns the set sorted."""
    final_set = set()
    for i in final_ids:
        final_set.add(int(i))
    first = set()
    for i in final_ids:
        first_id = int(i)
        while (int(parent[first_id]) if parent[first_id] >= 0 else 0) in final_set:
            first_id = int(parent[first_id])               # .unwrap(): a final node's parent that is final exists
        first.add(first_id)
    return sorted(first)


def path_to(xy, parent, node):
    """RRTTree::get_path_to (rrt.rs:48-61): root first"""
    ids = []
    p = int(node)
    while p >= 0:
        ids.append(p)
        p = int(parent[p])
    ids.reverse()
    return np.array([[xy[i][0], xy[i][1]] for i in ids], dtype=np.float64).reshape(-1, 2)


def path_cost(path):
    """get_path_cost (rrt.rs:223-227): norm2 of consecutive states summed from 0.0 in path order"""
    s = 0.0
    for a, b in zip(path[:-1], path[1:]):
        d2 = 0.0
        dx = float(b[0]) - float(a[0])
        d2 += dx * dx
        dx = float(b[1]) - float(a[1])
        d2 += dx * dx
        s += math.sqrt(d2)
    return s


def solutions(xy, parent, final_ids):
    """get_solutions (rrt.rs:195-221) -> [(id, path n x 2, cost)] in ascending node id"""
    out = []
    for i in firstly_final_ids(parent, final_ids):
        p = path_to(xy, parent, i)
        out.append((i, p, path_cost(p)))
    return out


def of_oracle(o):
    """the solutions of the oracle's last grow"""
    xy, parent, _ = o.tree()
    return solutions(xy, parent, o.final_ids())
