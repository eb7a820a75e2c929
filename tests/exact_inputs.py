"""Sample streams that make exact ties between DIFFERENT places, and helpers that count, on a finished oracle object, the ties a stream
made.  Plain numpy with fixed seeds.

Every coordinate of a stream is a dyadic rational (k / 2^m with small k), so coordinate differences, their squares and the sums of
two squares are exact in f64: two nodes at the same Euclidean distance from a sample are at bit-equal `norm2`, whichever way the
difference is taken, and `norm2 <= radius` meets equality whenever the radius is a whole number of pitches.  A continuous sampler
never does either; exact duplicates do, but at one place only (same region page, same steer result)."""
import numpy as np


# ---------------------------------------------------------------------------------------------------------------------- streams
def lattice_points(pitch):
    """the points (i * pitch, j * pitch), |i|, |j| < 1 / pitch, in row-major order: pitch 1/16 has 961, pitch 1/32 has 3969"""
    m = int(round(1.0 / pitch))
    assert m * pitch == 1.0 and m & (m - 1) == 0, "the pitch must be a power of two"
    k = np.arange(-(m - 1), m, dtype=np.float64) * pitch
    gx, gy = np.meshgrid(k, k, indexing="ij")
    return np.stack([gx.reshape(-1), gy.reshape(-1)], axis=1)


def lattice(pitch, seed, n):
    """n samples: the lattice points shuffled, cycled in that order when n exceeds their number"""
    pts = lattice_points(pitch)
    pts = pts[np.random.default_rng(seed).permutation(len(pts))]
    return np.ascontiguousarray(pts[np.arange(n) % len(pts)])


def lattice_once(pitch, seed, n):
    """the same without repetition (a repeated point makes a zero-length roadmap edge, on which the reference's extract_path can
    circle); raises when n is too large"""
    pts = lattice_points(pitch)
    if n > len(pts):
        raise ValueError("lattice_once: pitch %g has %d points, %d asked" % (pitch, len(pts), n))
    return np.ascontiguousarray(pts[np.random.default_rng(seed).permutation(len(pts))[:n]])


def staircase(n):
    """(-0.9 + i / 1024, -0.9 + i / 1024) with every third point repeated: x and y never decrease, and KdTree::add sends an equal
    coordinate to the right, so the kd-tree of this stream is one chain, as deep as the stream is long"""
    i = np.arange(n)
    i = i - (i + 1) // 4                       # 0 1 2 2 3 4 5 5 6 ...
    v = -0.9 + i / 1024.0
    return np.ascontiguousarray(np.stack([v, v], axis=1))


def cluster(n, centre, half_width, seed):
    """n distinct points centre + (i, j) / 8192, |i|, |j| <= half_width * 8192 (the centre snapped to a multiple of 1 / 8192)"""
    r = int(np.floor(half_width * 8192.0))
    side = 2 * r + 1
    if n > side * side:
        raise ValueError("cluster: %d points asked, the square holds %d" % (n, side * side))
    pick = np.random.default_rng(seed).choice(side * side, size=n, replace=False)
    c = np.round(np.asarray(centre, dtype=np.float64) * 8192.0)
    ij = np.stack([pick // side - r, pick % side - r], axis=1).astype(np.float64)
    return np.ascontiguousarray((c + ij) / 8192.0)


def decimal_grid(seed, n):
    """the points (i / 100, j / 100), |i|, |j| <= 95, shuffled and cycled: pixel corners of a 200 x 200 raster over [-1, 1)^2, none
    of them exact in binary"""
    k = np.arange(-95, 96, dtype=np.float64) / 100.0
    gx, gy = np.meshgrid(k, k, indexing="ij")
    pts = np.stack([gx.reshape(-1), gy.reshape(-1)], axis=1)
    pts = pts[np.random.default_rng(seed).permutation(len(pts))]
    return np.ascontiguousarray(pts[np.arange(n) % len(pts)])


# ---------------------------------------------------------------------------------------------------------------------- counting
def norm2(xy, q):
    """common.rs:203-213 for every row of xy against q"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    dx, dy = q[0] - xy[:, 0], q[1] - xy[:, 1]
    return np.sqrt(0.0 + dx * dx + dy * dy)


def norm1_exceeds(a, b, max_step):
    """steer's test (common.rs: the L1 norm against max_step): True when a sample at b is steered from a"""
    return abs(b[0] - a[0]) + abs(b[1] - a[1]) > max_step


def count_pairs_at_distance(xy, d):
    """unordered pairs of nodes whose norm2 is exactly d (d = 0: pairs of nodes at one place)"""
    xy = np.asarray(xy, dtype=np.float64)
    total = 0
    for j in range(1, len(xy)):
        total += int(np.count_nonzero(norm2(xy[:j], xy[j]) == d))
    return total


def count_shared_dist_root(xy, dist):
    """nodes whose dist_root is, bit for bit, also the dist_root of a node at another place"""
    xy, dist = np.asarray(xy, dtype=np.float64), np.asarray(dist, dtype=np.float64)
    order = np.argsort(dist.view(np.uint64), kind="stable")
    bits = dist.view(np.uint64)[order]
    starts = np.flatnonzero(np.concatenate(([True], bits[1:] != bits[:-1], [True])))
    shared = 0
    for a, b in zip(starts[:-1], starts[1:]):
        if b - a > 1:
            p = xy[order[a:b]]
            other = (p[:, None, :] != p[None, :, :]).any(axis=2).any(axis=1)
            shared += int(np.count_nonzero(other))
    return shared


def count_nearest_ties(xy, samples, different_places=True):
    """samples whose least norm2 to the rows of xy is attained by more than one node (at more than one place)"""
    xy = np.asarray(xy, dtype=np.float64)
    n = 0
    for q in np.asarray(samples, dtype=np.float64).reshape(-1, 2):
        d = norm2(xy, q)
        at = xy[d == d.min()]
        n += int(len(at) > 1 and (not different_places or (at != at[0]).any()))
    return n


def count_equidistant_places(xy, samples):
    """over all samples, the neighbours in distance order that are at bit-equal norm2 from the sample and at different places.  0 means
    that no comparison of distances from these samples to any subset of these nodes is decided by anything but a strict inequality,
    except between nodes at one place"""
    xy = np.asarray(xy, dtype=np.float64)
    runs = 0
    for q in np.asarray(samples, dtype=np.float64).reshape(-1, 2):
        d = norm2(xy, q)
        order = np.argsort(d, kind="stable")
        ds, ps = d[order], xy[order]
        runs += int(np.count_nonzero((ds[1:] == ds[:-1]) & (ps[1:] != ps[:-1]).any(axis=1)))
    return runs


def walk_tie_counts(cost_rows, wave=64):
    """cost_rows: for every step of a walk, the costs of the list the step takes its first minimum of, in list order.  Returns
    (steps with more than one least entry, those whose least entries sit in different lanes of a wave that strides the list
    (pos % wave), those with a least entry at a list position >= wave)"""
    tied = lanes = late = 0
    for row in cost_rows:
        row = np.asarray(row, dtype=np.float64)
        if row.size == 0 or not np.isfinite(row.min()):
            continue
        pos = np.flatnonzero(row == row.min())
        if len(pos) > 1:
            tied += 1
            lanes += int(len(set((pos % wave).tolist())) > 1)
            late += int(pos[-1] >= wave)
    return tied, lanes, late


def kd_depth(xy):
    """depth of the reference's kd-tree (nearest_neighbor.rs:29-46: insertion in id order, axes alternate, equal goes right): a plain
    insert that keeps its own position instead of recursing, so a chain of any length is fine.  The CPU file checks it against the
    oracle's kd-tree on a lattice stream."""
    pts = np.asarray(xy, dtype=np.float64).tolist()
    left, right, deepest = {}, {}, 1
    for i in range(1, len(pts)):
        cur, axis, depth = 0, 0, 1
        while True:
            side = left if pts[i][axis] < pts[cur][axis] else right
            depth += 1
            if cur not in side:
                side[cur] = i
                break
            cur, axis = side[cur], 1 - axis
        deepest = max(deepest, depth)
    return deepest


# ---------------------------------------------------------------------------------------------------------------------- the cases
def moved_lattice(pitch, seed, n):
    """lattice() with every point (x, y) moved by (x^2 / 3 + x^3 / 5, y^2 / 7 + y^3 / 11) / 64.  A translation would not do: q + v and
    q - v stay at one distance from q under any affine map; nor would an even or an odd map alone, which keeps f(q) - f(-q) the
    same in x and y, or |f(a)| = |f(-a)|.  Under this one the steps q -> q + a and q - a -> q differ unless q = -5 / 9 (x) or
    -11 / 21 (y), no lattice point, and the cubic terms differ between the axes -- so no sample has two places at one distance other
    than by an accident of rounding, which count_equidistant_places rules out on the finished tree."""
    xy = lattice(pitch, seed, n)
    x, y = xy[:, 0], xy[:, 1]
    return np.ascontiguousarray(xy + np.stack([x * x / 3.0 + x * x * x / 5.0, y * y / 7.0 + y * y * y / 11.0], axis=1) / 64.0)


def rrt_iteration_samples(case, xy, n_iter):
    """the sample of every iteration 1 .. n_iter of an RRT* growth fed the injected stream xy: every 100th iteration takes the goal
    point and draws nothing (rrt.rs:176-181)"""
    out, k = np.zeros((n_iter, 2)), 0
    for i in range(1, n_iter + 1):
        if i % 100 == 0:
            out[i - 1] = case.goals[0]
        else:
            out[i - 1] = xy[k]
            k += 1
    return out


RRT_ITERS = 2000
RRT_SEEDS = tuple(range(8))
SINGLE_SEED = 3          # the stream of the single-query runs: its K = 1 growth steers from a tied nearest node (the CPU file shows it)
ROW_MIN = [600 + (1200 * j) // 7 for j in range(8)]                    # form (c): loop conditions of their own, 600 .. 1800
ROW_MAX = [a + 100 + 37 * (j % 5) for j, a in enumerate(ROW_MIN)]      # ... and n_iter_max above, within the 2000 samples


def rrt_lattice_case():
    """cfg2 with max_step = 0.125 = two pitches of lattice(1/16): below about 1900 nodes heuristic_radius is max_step itself"""
    import cases
    c = cases.cfg2(RRT_ITERS)
    c.update(name="cfg2_lattice16", max_step=0.125)
    return c


def rrt_decimal_case():
    """cfg2 as it is (max_step 0.1) for decimal_grid(): every sample on a pixel corner of the 200 x 200 raster"""
    import cases
    c = cases.cfg2(RRT_ITERS)
    c.update(name="cfg2_decimal")
    return c


# ---------------------------------------------------------------------------------------------------------------------- kd forms
# The inputs of tests/test_gpu_kd_forms.py (the kd tie-order side chain in every form) and of their CPU side,
# tests/test_kd_forms_inputs_cpu.py.  A key is (stream, seed, K, n_iter_min, n_iter_max):
#   "lattice":    rrt_lattice_case() fed lattice(1/16, seed, n_iter_max), cycled past its 961 points: ties between different places;
#   "chain":      cases.empty_space from (-0.9, -0.9) fed staircase(n): a kd-tree that is (nearly) one chain, in which nearly every
#                 new node of a group bids for the same child slot; ties between copies at one place;
#   "duplicates": cfg2 fed _dup_samples of test_gpu_parity_r3.py (exact copies of other samples): equal-cost parents off the goal path.
KDF_SEEDS = tuple(range(8))
KDF_CLAIM = {128: (1, 2000), 256: (4, 2500), 512: (4, 4500), 1024: (4, 9000)}      # K: (kd_group, n_iter): two full groups and a short one at least
KDF_LOCATE64 = (64, (3, 0), 2000)          # K, the seeds of its two rows, n_iter: 8 steps * 64 * 2 rows < 4096 nodes a group
KDF_VARIANT_K, KDF_VARIANT_ITERS, KDF_VARIANT_SEEDS = 256, 2500, tuple(range(9))
KDF_CHAIN_K, KDF_CHAIN_ITERS = 256, 3000
KDF_SINGLE = (("lattice", SINGLE_SEED, 64, 2000), ("lattice", SINGLE_SEED, 1024, 9000), ("chain", 0, KDF_CHAIN_K, KDF_CHAIN_ITERS))
KDF_ROWS_K = 128
KDF_SEQ_ITERS, KDF_SEQ_K, KDF_SEQ_CHECKED = 3000, 256, (0, 4)          # (N_ITER and K of test_gpu_launch_sequences.py, the contexts it compares)
KDF_DUP_SAMPLES, KDF_DUP_K = 4000, 512
KDF_DUP_ITERS = KDF_DUP_SAMPLES - KDF_DUP_SAMPLES // 100 - 5           # (every 100th iteration takes the goal point and draws nothing)


def kd_forms_inputs(stream, seed, n_iter_min, n_iter_max):
    """(case, injected samples) of a key"""
    import cases
    if stream == "lattice":
        c, xy = rrt_lattice_case(), lattice(1 / 16, seed, n_iter_max)
    elif stream == "chain":
        c, xy = cases.empty_space(), staircase(n_iter_max)
        c.update(name="empty_staircase", start=(-0.9, -0.9))
    elif stream == "duplicates":
        from test_gpu_parity_r3 import _dup_samples
        c, xy = cases.cfg2(), _dup_samples(KDF_DUP_SAMPLES, 20 + seed)
    else:
        raise ValueError(stream)
    c.update(n_iter_min=n_iter_min, n_iter_max=n_iter_max)
    return c, xy


def kd_forms_keys():
    """every key the GPU file grows an oracle for, once each, in a fixed order"""
    keys = []
    for K, (_, n) in sorted(KDF_CLAIM.items()):
        keys += [("lattice", s, K, n, n) for s in KDF_SEEDS]
    K, seeds, n = KDF_LOCATE64
    keys += [("lattice", s, K, n, n) for s in seeds]
    keys += [("lattice", s, KDF_VARIANT_K, KDF_VARIANT_ITERS, KDF_VARIANT_ITERS) for s in KDF_VARIANT_SEEDS]
    keys += [(st, s, K, n, n) for st, s, K, n in KDF_SINGLE]
    keys += [("lattice", s, KDF_ROWS_K, ROW_MIN[s], ROW_MAX[s]) for s in KDF_SEEDS]
    keys += [("lattice", s, KDF_SEQ_K, a, KDF_SEQ_ITERS) for s in KDF_SEQ_CHECKED for a in (KDF_SEQ_ITERS, 1000)]
    keys += [("duplicates", s, KDF_DUP_K, KDF_DUP_ITERS, KDF_DUP_ITERS) for s in KDF_SEEDS]
    return list(dict.fromkeys(keys))


PTO_ITERS = 2500


def pto_lattice_case():
    """cfg3_near with max_step = 0.0625 = two pitches of lattice_once(1/32)"""
    import cases
    c = cases.cfg3_near(PTO_ITERS)
    c.update(name="cfg3_near_lattice32", max_step=0.0625)
    return c


def pto_stream(seed=0):
    return lattice_once(1.0 / 32, seed, PTO_ITERS)


# ---------------------------------------------------------------------------------------------------------------------- walks
def count_steering_ties(xy, samples, nearest, K, max_step):
    """(iterations whose sample has a node at another place at bit-equal norm2 to the nearest node the oracle chose, those of them
    that steer from both).  Only the part of the step's snapshot that is known to exist is looked at -- ids up to the largest nearest
    id chosen in this step or an earlier one -- so every tie counted is one the step's search met."""
    xy, nearest = np.asarray(xy, dtype=np.float64), np.asarray(nearest).astype(np.int64)
    ties = steered = known = 0
    for i, (q, j) in enumerate(zip(np.asarray(samples, dtype=np.float64), nearest)):
        if i % K == 0:
            known = max(known, int(nearest[i:i + K].max()) + 1)
        d = norm2(xy[:known], q)
        other = np.flatnonzero((d == d[j]) & (xy[:known] != xy[j]).any(axis=1))
        if other.size:
            ties += 1
            steered += int(norm1_exceeds(xy[j], q, max_step) and norm1_exceeds(xy[other[0]], q, max_step))
    return ties, steered


class Roadmap:
    """PRM::plan_path (prm.rs:111-123) over a roadmap's arrays in plain Python: the kd-tree's nearest nodes (first visited wins),
    dijkstra from the goal node, then from the start node always the first parent of least cost-to-goal + edge in push order."""

    def __init__(self, xy, efrom, eto):
        import qmdp_ref as Q
        self.Q = Q
        self.pts = [tuple(p) for p in np.asarray(xy, dtype=np.float64).tolist()]
        self.adj = Q.children_from_edges(len(self.pts), efrom, eto)
        self.kd = Q.KdTree(self.pts)
        self.weighted = Q.weighted_parents(self.pts, self.adj)

    def walk(self, start, goal):
        """(states of the path, per step the costs of the node's list in list order, for walk_tie_counts)"""
        Q, pts, adj = self.Q, self.pts, self.adj
        node, target = self.kd.nearest(tuple(float(v) for v in start)), self.kd.nearest(tuple(float(v) for v in goal))
        dist = Q.dijkstra_world(None, None, self.weighted, None, [target])
        if dist[node] == Q.INF:
            return np.zeros((0, 2)), []
        path, rows = [pts[node]], []
        while dist[node] != 0.0:
            row = [dist[p] + Q.norm2(pts[p], pts[node]) for p in adj[node]]
            rows.append(row)
            node = adj[node][int(np.argmin(row))]              # argmin: the first minimum
            path.append(pts[node])
            assert len(path) <= len(pts), "the walk circles"
        return np.array(path, dtype=np.float64).reshape(-1, 2), rows


def qmdp_world_walk_rows(q, start, belief, horizon):
    """the lists that the per-world walks of react_qmdp (qmdp_policy_extractor.rs:51-62, 110-123) take their first minimum of, for a
    planned qmdp_ref.Qmdp: per step the children's costs-to-goal in list order, all worlds one after the other"""
    _, at = q.get_common_path(q.nearest(start), [float(b) for b in belief], float(horizon))
    rows = []
    for world in range(q.n_worlds):
        cost, i, steps = q.cost_to_goals[world], at, 0
        while cost[i] > 0.0 and steps < q.max_states:
            rows.append([cost[c] for c in q.children[i]])
            i = q.get_best_child(i, world)
            steps += 1
    return rows
