"""The reference's figures drawn on the device (porrt_canvas_*, po_rrt_amd/csrc/porrt_draw.hpp) against the sequential restatement
(tests/draw_ref.py; its draw_line in C++, tests/draw_ref_line.cpp, for the large pictures): every image byte for byte.
tests/test_draw_cpu.py asserts that the crafted inputs have teeth (their image depends on the draw order, their hub pixels hold the
counts claimed here)."""
import os
import subprocess

import numpy as np
import pytest

import cases
import draw_inputs as di
import draw_ref as dr
from oracle import orc

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -5


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


@pytest.fixture(scope="module")
def line_lib(tmp_path_factory):
    return dr.build_line_lib(tmp_path_factory.mktemp("draw_ref"))


def small_engine(eng_mod, **options):
    e = eng_mod.Engine(0)
    e.set_grid(di.raster(), di.LOW, di.UP, eng_mod.DOMAIN_SHELF)
    for k, v in options.items():
        e.set_option(k, v)
    return e


def ref_image(lines, factor, alpha, color=di.COLOR):
    c = dr.RefCanvas(di.raster(), di.LOW, di.UP, factor)
    c.draw_lines(lines, color, alpha)
    return c


def device_image(eng_mod, lines, factor, alpha, color=di.COLOR, **options):
    cv = small_engine(eng_mod, **options).canvas(factor)
    cv.draw_lines(lines, color, alpha)
    return cv.rgb(), cv.info()


# ---- 1. crafted lines
@pytest.mark.parametrize("factor", [1, 3])
@pytest.mark.parametrize("alpha", [1.0, 0.3])
def test_crafted_lines(eng_mod, factor, alpha):
    lines = di.octant_lines()
    e = small_engine(eng_mod)
    cv = e.canvas(factor)
    assert cv.size() == (16 * factor, 16 * factor)
    assert np.array_equal(cv.rgb(), dr.RefCanvas(di.raster(), di.LOW, di.UP, factor).img), "the canvas before any line: the raster, block-replicated"
    cv.draw_lines(lines, di.COLOR, alpha)
    want = ref_image(lines, factor, alpha)
    assert np.array_equal(cv.rgb(), want.img)
    info = cv.info()
    assert info["lines"] == len(lines) and info["fragments"] == int(want.count.sum()) and info["passes"] == 1
    assert info["heaviest_pixel"] == int(want.count.max()) and info["gradient_by_f64"] == 0
    # one line at a time is the same picture (calls compose in order)
    one = e.canvas(factor)
    for l in lines:
        one.draw_lines([l], di.COLOR, alpha)
    assert np.array_equal(one.rgb(), want.img)


@pytest.mark.parametrize("factor", [1, 3])
def test_invalid_lines_leave_the_canvas(eng_mod, factor):
    cv = small_engine(eng_mod).canvas(factor)
    cv.draw_lines(di.octant_lines()[:9], di.COLOR, 0.3)
    before = cv.rgb()
    for lines, what in di.invalid_lines():
        with pytest.raises(eng_mod.PorrtError) as err:
            cv.draw_lines(lines, di.COLOR, 1.0)
        assert err.value.code == INVALID, what
        assert np.array_equal(cv.rgb(), before), what
    with pytest.raises(eng_mod.PorrtError) as err:
        cv.draw_path([(0.0, 0.0), (0.5, float("nan")), (0.2, 0.2)], di.COLOR)
    assert err.value.code == INVALID and np.array_equal(cv.rgb(), before)
    with pytest.raises(eng_mod.PorrtError) as err:
        cv.draw_circles([(0.0, 0.0), (float("inf"), 0.1)], 0.2, di.COLOR)
    assert err.value.code == INVALID and np.array_equal(cv.rgb(), before)
    cv.draw_lines(np.zeros((0, 4)), di.COLOR, 1.0)                  # no lines: nothing happens
    assert np.array_equal(cv.rgb(), before) and cv.info()["lines"] == 0


# ---- 2. order
def test_order_matters_and_is_kept(eng_mod):
    lines = di.octant_lines()
    fwd, _ = device_image(eng_mod, lines, 3, 0.3)
    rev, _ = device_image(eng_mod, lines[::-1], 3, 0.3)
    want_f, want_r = ref_image(lines, 3, 0.3).img, ref_image(lines[::-1], 3, 0.3).img
    assert not np.array_equal(want_f, want_r)
    assert np.array_equal(fwd, want_f) and np.array_equal(rev, want_r)


# ---- 3. hub pixels: either side of the lane / wave / workgroup boundaries, one trip and several trips of the workgroup form
@pytest.mark.parametrize("n,factor,alpha,heavy_cap,heavy", [
    (di.HUB_SMALL, 1, 0.3, 16, True),           # the default: the hub goes to the workgroup form, its neighbours of 17 .. 64 records to the one-wave form
    (di.HUB_SMALL, 1, 0.3, 69, True),           # 70 > 69: the hub alone is heavy
    (di.HUB_SMALL, 1, 0.3, 70, False),          # 70 <= 70: a lane resolves all of it
    (di.HUB_SMALL, 3, 1.0, 1, True),            # every pixel with two fragments leaves the lane form: lists of every small length through the one-wave form
    (di.HUB_LARGE, 3, 0.3, 16, True),           # 1100 > 1024: two trips (two sorted runs, merged) on the hub
    (di.HUB_LARGE, 3, 0.3, 1024, True),         # 1100 > 1024 again, with every other pixel resolved by a lane
    (di.HUB_HUGE, 3, 0.3, 16, True),            # 2100: three sorted runs (1024, 1024, 52), every record ranked against two other runs
    (di.HUB_HUGE, 3, 0.3, 64, True),            # the same with no pixel in the one-wave form
])
def test_hub_pixels(eng_mod, n, factor, alpha, heavy_cap, heavy):
    lines = di.hub_lines(n)
    want = ref_image(lines, factor, alpha)
    assert int(want.count.max()) == n
    got, info = device_image(eng_mod, lines, factor, alpha, draw_heavy_cap=heavy_cap)
    assert np.array_equal(got, want.img)
    assert info["heaviest_pixel"] == n and info["fragments"] == int(want.count.sum()) and info["passes"] == 1
    assert info["heavy_pixels"] == int((want.count > heavy_cap).sum()) and (info["heavy_pixels"] > 0) == heavy
    # of those, the pixels of at most 64 records take the one-wave form, the others the workgroup form
    assert info["wave_pixels"] == int(((want.count > heavy_cap) & (want.count <= 64)).sum())
    if n == di.HUB_SMALL and heavy_cap == 16:
        assert 0 < info["wave_pixels"] < info["heavy_pixels"], "both forms ran"


def test_hub_in_reverse_order(eng_mod):
    lines = di.hub_lines(di.HUB_LARGE)[::-1]
    got, _ = device_image(eng_mod, lines, 3, 0.3)
    assert np.array_equal(got, ref_image(lines, 3, 0.3).img)


# ---- 4. passes
@pytest.mark.parametrize("cap", [24, 64, 1])
def test_passes_compose(eng_mod, cap):
    lines = di.pass_lines()
    want = ref_image(lines, 1, 0.3)
    single, info1 = device_image(eng_mod, lines, 1, 0.3)
    assert info1["passes"] == 1 and np.array_equal(single, want.img)
    got, info = device_image(eng_mod, lines, 1, 0.3, draw_max_fragments=cap)
    assert np.array_equal(got, single)
    assert info["passes"] > 1 and info["fragments"] == info1["fragments"] == int(want.count.sum())
    # the passes the cut rule gives: as many whole lines as fit, one line at the least
    per_line = []
    for l in lines:
        c = dr.RefCanvas(di.raster(), di.LOW, di.UP, 1)
        c.draw_line((l[0], l[1]), (l[2], l[3]), di.COLOR, 0.3)
        per_line.append(int(c.count.sum()))
    assert max(per_line) > 24
    passes, k = 0, 0
    while k < len(per_line):
        s, k = per_line[k], k + 1
        while k < len(per_line) and s + per_line[k] <= cap:
            s, k = s + per_line[k], k + 1
        passes += 1
    assert info["passes"] == passes
    if cap == 1:
        assert passes == len(lines), "every line a pass of its own: every cut falls right after a hub line"


# ---- 5. draw_tree
def test_draw_tree(eng_mod, line_lib):
    case = cases.cfg2(1500)
    e = cases.configure(eng_mod.Engine(0), case)
    cases.grow(e, case, K=256)
    cv = e.canvas(3)
    cv.draw_tree(e)
    xy, parent, _ = e.tree()
    want = dr.FastCanvas(line_lib, cases.load_map(case.grid), factor=3)
    want.draw_tree(xy, parent)
    assert np.array_equal(cv.rgb(), want.img)
    info = cv.info()
    assert info["lines"] == len(parent) and info["fragments"] == int(want.count.sum()) and info["heaviest_pixel"] == int(want.count.max())
    # in several passes, and with every crowded pixel in the workgroup form
    e.set_option("draw_max_fragments", 5000)
    e.set_option("draw_heavy_cap", 4)
    cv2 = e.canvas(3)
    cv2.draw_tree(e)
    assert np.array_equal(cv2.rgb(), want.img) and cv2.info()["passes"] > 1 and cv2.info()["heavy_pixels"] > 0


# ---- 6. draw_full_graph
def oracle_children(o):
    """the children lists of the oracle's PTO graph in the reference's push order (pto.rs:103-120): the batched oracle keeps the edge SET of
    a step; new nodes ascending, the neighbours of one new node in the pre-order of the reference's kd-tree (oracle kdtree.c), as
    tests/test_gpu_parity.py orders them"""
    lib = orc.lib()
    xy = np.ascontiguousarray(o.tree()[0], dtype=np.float64)
    kd = lib.orc_kd_new(xy[0], 0)
    for j in range(1, len(xy)):
        lib.orc_kd_add(kd, xy[j], j)
    out = np.zeros(len(xy), dtype=np.uint64)
    assert lib.orc_kd_radius(kd, xy[0], 1e300, out, len(out)) == len(xy)
    lib.orc_kd_free(kd)
    rank = np.zeros(len(xy), dtype=np.int64)
    rank[out.astype(np.int64)] = np.arange(len(xy))
    ef, et, _ = o.edges()
    order = np.lexsort((rank[ef], et))
    return xy, ef[order], et[order]


def graph_case(name):
    if name == "shelf":
        return cases.cfg3(300, 300), False
    return cases.cfg_door(300, 300), True


@pytest.mark.parametrize("name", ["shelf", "door"])
def test_draw_full_graph(eng_mod, line_lib, name):
    case, door = graph_case(name)
    e = cases.configure(eng_mod.Engine(0), case)
    cases.grow(e, case, K=64)
    o = cases.configure(orc.Oracle(), case)
    cases.grow(o, case, K=64, algo=orc.ALGO_BATCHED_KD)
    xy, ef, et = oracle_children(o)
    children = dr.children_from_edges(len(xy), ef, et)
    cv = e.canvas(3)
    cv.draw_full_graph(e)
    want = dr.FastCanvas(line_lib, cases.load_map(case.grid), factor=3)
    want.draw_full_graph(xy, children, door=door)
    assert want.lines == 2 * len(ef) > 0
    assert np.array_equal(cv.rgb(), want.img)
    info = cv.info()
    assert info["lines"] == want.lines and info["fragments"] == int(want.count.sum()) and info["heaviest_pixel"] == int(want.count.max())


def test_draw_full_graph_of_a_roadmap(eng_mod, line_lib):
    case = cases.cfg2(400)
    e = cases.configure(eng_mod.Engine(0), case)
    e.grow_prm(case.start, 0.1, 2.0, 400)
    o = cases.configure(orc.Oracle(), case)
    o.grow_prm(case.start, 0.1, 2.0, 400)
    xy = o.tree()[0]
    ef, et, _ = o.edges()
    e.set_option("draw_max_fragments", 1500)
    cv = e.canvas(2)
    cv.draw_full_graph(e)
    want = dr.FastCanvas(line_lib, cases.load_map(case.grid), factor=2)
    want.draw_full_graph(xy, dr.children_from_edges(len(xy), ef, et))
    assert want.lines == 2 * len(ef) > 0
    assert np.array_equal(cv.rgb(), want.img)
    assert cv.info()["passes"] > 1 and cv.info()["fragments"] == int(want.count.sum())


# ---- 7. the driver's sequence (pto.rs:313-317)
def test_driver_sequence(eng_mod, line_lib, tmp_path):
    case = cases.cfg3_near(1500)
    e = cases.configure(eng_mod.Engine(0), case)
    cases.grow(e, case, K=64)
    e.build_belief_graph([0.5, 0.5])
    e.compute_expected_costs()
    e.extract_policy()
    (pxy, _, ppar, _), _ = e.refine_policy(500)
    assert max(np.bincount(ppar[ppar >= 0])) >= 2, "the policy branches: draw_policy draws a circle"
    cv = e.canvas(5)                                   # m.resize(5)
    cv.draw_full_graph(e)
    cv.draw_zones_observability()
    cv.draw_policy(pxy, ppar)
    path = str(tmp_path / "driver.png")
    cv.save_png(path)
    xy = e.tree()[0]
    ef, et, _ = e.edges()                              # (test 6 compares the lists with the oracle's)
    want = dr.FastCanvas(line_lib, cases.load_map(case.grid), factor=5)
    want.draw_full_graph(xy, dr.children_from_edges(len(xy), ef, et))
    want.draw_zones_observability(e.zone_positions(), case.visibility)
    want.draw_policy(pxy, ppar)
    assert np.array_equal(cv.rgb(), want.img)
    from PIL import Image                              # (a missing package is a failure, not a skip: the issue asks for this read-back)
    with Image.open(path) as im:
        assert im.mode == "RGB"
        back = np.array(im)
    assert np.array_equal(back, want.img)
    # draw_path, as rrt.rs:299-303 ends: a path over the same picture
    cv.draw_path(pxy[:5], eng_mod.colors.RED)
    want.draw_path(pxy[:5], eng_mod.colors.RED)
    assert np.array_equal(cv.rgb(), want.img)


def test_cpp_mirror_draws_the_driver_tail(eng_mod, line_lib, tmp_path):
    """examples/plan_pto.cpp with its sixth argument: m.resize(5); m.draw_full_graph(pto); m.draw_zones_observability(); m.draw_policy(policy);
    m.save(path) of include/porrt.hpp, against the same problem through the Python binding and the restatement"""
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "po_rrt_amd")
    exe, png = str(tmp_path / "plan_pto"), str(tmp_path / "pto.png")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(root, "examples", "plan_pto.cpp"),
                    "-L" + lib, "-lporrt_hip", "-Wl,-rpath," + lib], check=True)
    case = cases.cfg3(1500, 1500)
    out = subprocess.run([exe, os.path.join(cases.MAPS, case.grid + ".pgm"), os.path.join(cases.MAPS, case.zones + ".pgm"), "1500", "64", "0", png],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "picture" in out.stdout, out.stdout + out.stderr
    e = cases.configure(eng_mod.Engine(0), case)
    cases.grow(e, case, K=64)
    e.build_belief_graph([0.5, 0.5])
    e.compute_expected_costs()
    xy = e.tree()[0]
    ef, et, _ = e.edges()
    want = dr.FastCanvas(line_lib, cases.load_map(case.grid), factor=5)
    want.draw_full_graph(xy, dr.children_from_edges(len(xy), ef, et))
    want.draw_zones_observability(e.zone_positions(), case.visibility)
    n_policy = 0
    if np.isfinite(e.expected_cost_of(0)):
        (oid, par, _), _ = e.extract_policy()
        B = len(e.belief_graph(lists=False)[0])
        want.draw_policy(xy[(oid // np.uint64(B)).astype(np.int64)], par)
        n_policy = len(par)
    assert ("policy_nodes %d " % n_policy) in out.stdout and (" nodes %d beliefs" % len(xy)) in out.stdout, out.stdout
    with Image.open(png) as im:
        assert np.array_equal(np.array(im), want.img)


# ---- 8. errors
def test_errors(eng_mod):
    e = small_engine(eng_mod)
    with pytest.raises(eng_mod.PorrtError) as err:
        e.canvas(0)
    assert err.value.code == INVALID
    with pytest.raises(eng_mod.PorrtError) as err:
        e.canvas(1025)                                  # 16 400 pixels a side
    assert err.value.code == CAPACITY
    with pytest.raises(eng_mod.PorrtError) as err:
        eng_mod.Engine(0).canvas(1)                     # no grid
    assert err.value.code == INVALID
    cv = e.canvas(3)
    cv.draw_lines(di.octant_lines()[:5], di.COLOR, 0.3)
    before = cv.rgb()
    with pytest.raises(eng_mod.PorrtError) as err:
        cv.draw_tree(e)                                 # nothing grown
    assert err.value.code == INVALID and np.array_equal(cv.rgb(), before)
    with pytest.raises(eng_mod.PorrtError) as err:
        cv.draw_full_graph(e)
    assert err.value.code == INVALID and np.array_equal(cv.rgb(), before)
    case = cases.cfg2(300)
    other = cases.configure(eng_mod.Engine(0), case)    # another raster geometry
    cases.grow(other, case, K=64)
    with pytest.raises(eng_mod.PorrtError) as err:
        cv.draw_tree(other)
    assert err.value.code == INVALID and np.array_equal(cv.rgb(), before)
    with pytest.raises(eng_mod.PorrtError) as err:
        other.canvas(1).draw_full_graph(other)          # a tree is no graph
    assert err.value.code == INVALID
    with pytest.raises(eng_mod.PorrtError) as err:
        cv.draw_policy([(0.0, 0.0), (0.1, 0.1)], [-1, 5])
    assert err.value.code == INVALID and np.array_equal(cv.rgb(), before)
    for name, bad in (("draw_max_fragments", 0), ("draw_heavy_cap", 0), ("draw_heavy_cap", 1025), ("draw_max_fragments", (1 << 30) + 1)):
        with pytest.raises(eng_mod.PorrtError):
            e.set_option(name, bad)
    assert e.get_option("draw_max_fragments") == 1 << 24 and e.get_option("draw_heavy_cap") == 16
    # a context with the same geometry may be drawn from, and the canvas outlives its context
    twin = eng_mod.Engine(0)                            # (another raster of the same geometry: all free)
    twin.set_grid(np.full((16, 16), 255, dtype=np.uint8), di.LOW, di.UP, eng_mod.DOMAIN_SHELF)
    twin.set_sampler(di.LOW, di.UP, 3)
    twin.set_square_goal(np.array([[0.9, 0.9]]), np.array([1], dtype=np.uint64), 0.05)
    twin.grow((0.0, 0.0), 0.3, 1.0, 40, 40, batch_K=8, mode=eng_mod.MODE_RRT)
    e.close()
    cv.draw_tree(twin)
    xy, parent, _ = twin.tree()
    assert len(parent) > 10
    want = dr.RefCanvas(di.raster(), di.LOW, di.UP, 3)
    want.draw_lines(di.octant_lines()[:5], di.COLOR, 0.3)
    want.draw_tree(xy, parent)
    assert np.array_equal(cv.rgb(), want.img)
