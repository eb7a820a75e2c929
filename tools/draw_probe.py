"""The reference's figures on the device against the same pictures drawn by the single-thread C++ restatement on the host (tests/draw_ref_line.cpp,
the download it needs first included): draw_tree on a bench-size tree, draw_full_graph on the bench's 200 000-sample roadmap, and the
driver's sequence (pto.rs:313-317) on map_4, all at factor 5.  Per run: lines, fragments, passes, the heaviest pixel, device milliseconds per
stage, and whether the two images are the same bytes.  Writes profiles/draw.json (or --out).
usage: python tools/draw_probe.py [--reps 3] [--skip-host] [--only tree,roadmap,driver] [--out PATH]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import cases  # noqa: E402
import draw_ref as dr  # noqa: E402
import po_rrt_amd  # noqa: E402

FACTOR = 5


def ms(info):
    return {k.replace("s_", "ms_", 1): 1e3 * v for k, v in info.items() if k.startswith("s_")}


def device(draw, e, reps, graph=False):
    """the picture on a fresh canvas (the first call: it allocates the canvas's buffers and, for a graph whose adjacency order the context has
    not made yet, makes it, ranks on the device), then the median of reps calls on a second canvas whose buffers are warm, and for a graph one
    more call there after the context's adjacency order was thrown away (setting option host_ranks does that)"""
    cv = e.canvas(FACTOR)
    t = time.perf_counter()
    draw(cv)
    first = time.perf_counter() - t
    tc = e.canvas(FACTOR)
    draw(tc)
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        infos = draw(tc)
        runs.append((time.perf_counter() - t, infos))
    wall, infos = sorted(runs, key=lambda r: r[0])[len(runs) // 2]
    res = {"ms_wall": 1e3 * wall, "first_call_ms_wall": 1e3 * first,
           "calls": [dict({k: v for k, v in i.items() if not k.startswith("s_")}, **ms(i)) for i in infos]}
    if graph:
        e.set_option("host_ranks", 1)
        t = time.perf_counter()
        draw(tc)
        res["ms_wall_adjacency_order_not_cached"] = 1e3 * (time.perf_counter() - t)
    return cv, res


def graph_lines(xy, ef, et):
    """the lines of draw_full_graph in draw order, from the forward edges in the reference's order"""
    E = len(ef)
    owner = np.concatenate([et, ef]).astype(np.int64)
    other = np.concatenate([ef, et]).astype(np.int64)
    order = np.lexsort((np.concatenate([np.arange(E), np.arange(E)]), np.concatenate([np.zeros(E, np.int8), np.ones(E, np.int8)]), owner))
    return np.ascontiguousarray(np.concatenate([xy[owner[order]], xy[other[order]]], axis=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--only", default="tree,roadmap,driver")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draw.json"))
    a = ap.parse_args()
    lib = dr.build_line_lib(tempfile.mkdtemp())
    out = {"factor": FACTOR}

    def host(name, grid, low, up, fetch, draw):
        if a.skip_host:
            return None
        t = time.perf_counter()
        data = fetch()
        t_fetch = time.perf_counter() - t
        c = dr.FastCanvas(lib, grid, low, up, FACTOR)
        t = time.perf_counter()
        draw(c, data)
        t_draw = time.perf_counter() - t
        out[name]["host"] = {"ms_download_and_lists": 1e3 * t_fetch, "ms_draw": 1e3 * t_draw, "fragments": int(c.count.sum())}
        return c

    if "tree" in a.only:
        case = cases.cfg2(125000)
        e = cases.configure(po_rrt_amd.Engine(0), case)
        cases.grow(e, case, K=1024)
        cv, out["tree"] = device(lambda cv: [cv.draw_tree(e), cv.info()][1:], e, a.reps)
        out["tree"]["nodes"] = e.num_nodes()

        def tree_lines():
            xy, parent, _ = e.tree()
            k = np.nonzero(parent >= 0)[0]
            return np.ascontiguousarray(np.concatenate([xy[parent[k]], xy[k]], axis=1))
        c = host("tree", cases.load_map(case.grid), (-1, -1), (1, 1), tree_lines, lambda c, ab: c.draw_lines(ab, dr.TEAL, 0.3))
        if c is not None:
            out["tree"]["same_bytes"] = bool(np.array_equal(cv.rgb(), c.img))
        print(json.dumps(out["tree"]), flush=True)

    if "roadmap" in a.only:
        e = po_rrt_amd.Engine(0)
        grid = cases.load_map("map_benchmark_like")
        e.set_grid(grid, (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
        e.set_sampler((-1.0, -1.0), (1.0, 1.0), 3)
        e.grow_prm((0.0, -0.8), 0.1, 2.0, 200000)
        cv, out["roadmap"] = device(lambda cv: [cv.draw_full_graph(e), cv.info()][1:], e, a.reps, graph=True)

        def road_lines():
            xy = e.tree()[0]
            ef, et, _ = e.edges()
            return graph_lines(xy, ef, et)
        c = host("roadmap", grid, (-1, -1), (1, 1), road_lines, lambda c, ab: c.draw_lines(ab, dr.GRAY5, 0.25))
        if c is not None:
            out["roadmap"]["same_bytes"] = bool(np.array_equal(cv.rgb(), c.img))
        print(json.dumps(out["roadmap"]), flush=True)

    if "driver" in a.only:
        case = cases.cfg_map4(5000)
        e = cases.configure(po_rrt_amd.Engine(0), case)
        cases.grow(e, case, K=256)
        nw = e.n_worlds()
        e.build_belief_graph([1.0 / nw] * nw)
        e.compute_expected_costs()
        e.extract_policy()
        (pxy, _, ppar, _), _ = e.refine_policy(0)

        def sequence(cv):
            infos = []
            for call in (lambda: cv.draw_full_graph(e), cv.draw_zones_observability, lambda: cv.draw_policy(pxy, ppar)):
                call()
                infos.append(cv.info())
            return infos
        cv, out["driver"] = device(sequence, e, a.reps, graph=True)
        out["driver"].update(nodes=e.num_nodes(), policy_nodes=len(ppar))

        def driver_data():
            xy = e.tree()[0]
            ef, et, _ = e.edges()
            return graph_lines(xy, ef, et)

        def driver_draw(c, ab):
            c.draw_lines(ab, dr.GRAY5, 0.15)
            c.draw_zones_observability(e.zone_positions(), case.visibility)
            c.draw_policy(pxy, ppar)
        c = host("driver", cases.load_map(case.grid), (-1, -1), (1, 1), driver_data, driver_draw)
        if c is not None:
            out["driver"]["same_bytes"] = bool(np.array_equal(cv.rgb(), c.img))
        print(json.dumps(out["driver"]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
