"""CPU checks of the drawing restatement (tests/draw_ref.py), of the inputs the GPU tests draw (tests/draw_inputs.py) and of the PNG
writer (host code of the library: no device).  The Xiaolin Wu walk is recalled from the line_drawing crate and pinned by nothing in the
reference tree, so its basic properties are checked here before anything is compared with it."""
import math

import numpy as np
import pytest

import draw_inputs as di
import draw_ref as dr
from draw_ref import f32


def _walk(a, b):
    return dr.wu_walk((f32(a[0]), f32(a[1])), (f32(b[0]), f32(b[1])))


def _lines_for_walk():
    c = (20, 17)
    out = []
    for dx, dy in ((9, 4), (4, 9), (-4, 9), (-9, 4), (-9, -4), (-4, -9), (4, -9), (9, -4)):       # the eight octants
        out.append((c, (c[0] + dx, c[1] + dy)))
    out += [((3, 5), (14, 5)), ((14, 5), (3, 5)), ((6, 2), (6, 13)), ((2, 2), (11, 11)), ((11, 2), (2, 11)), ((7, 7), (7, 7))]
    return out


@pytest.mark.parametrize("a,b", _lines_for_walk())
def test_wu_walk_properties(a, b):
    w = _walk(a, b)
    pix = [p for p, _ in w]
    assert tuple(a) in pix and tuple(b) in pix, "both ends are part of the walk"
    assert len(set(pix)) == len(pix), "a line meets a pixel once"
    steep = abs(b[1] - a[1]) > abs(b[0] - a[0])
    major = 1 if steep else 0
    steps = {}
    for p, wt in w:
        assert 0.0 <= float(wt) <= 1.0
        steps.setdefault(p[major], []).append((p, wt))
    lo, hi = sorted((a[major], b[major]))
    assert sorted(steps) == list(range(lo, hi + 1)), "one step per unit of the major axis, ends included"
    for s in steps.values():
        assert len(s) in (1, 2)
        assert float(sum(f32(x) for _, x in s)) == pytest.approx(1.0, abs=1e-6), "a step's weights sum to 1"
        if len(s) == 2:
            assert s[1][0][1 - major] == s[0][0][1 - major] + 1, "the second pixel of a step is the next one across"
    back = _walk(b, a)
    assert set(p for p, _ in back) == set(pix), "reversed ends cover the same pixels"
    # the vectorised form is the same walk
    px, py, wt = dr.wu_arrays((f32(a[0]), f32(a[1])), (f32(b[0]), f32(b[1])))
    assert [(int(x), int(y)) for x, y in zip(px, py)] == pix
    assert np.array_equal(np.asarray(wt, dtype=f32).view(np.uint32), np.array([x for _, x in w], dtype=f32).view(np.uint32))


def test_wu_walk_special_lines():
    h = _walk((3, 5), (14, 5))
    assert [p for p, _ in h] == [(x, 5) for x in range(3, 15)] and all(float(x) == 1.0 for _, x in h), "a horizontal line stays on its row, full weight"
    v = _walk((6, 2), (6, 13))
    assert [p for p, _ in v] == [(6, y) for y in range(2, 14)] and all(float(x) == 1.0 for _, x in v)
    d = _walk((2, 2), (11, 11))
    assert [p for p, _ in d] == [(k, k) for k in range(2, 12)] and all(float(x) == 1.0 for _, x in d), "an exact diagonal is one pixel a step"
    z = _walk((7, 7), (7, 7))
    assert len(z) == 1 and z[0][0] == (7, 7) and float(z[0][1]) == 1.0, "zero length: one pixel, weight 1 (dx == 0 takes gradient 1, never a division)"
    s = _walk((0, 0), (3, 1))                     # gradient 1/3 in f32: fractions 0, 1/3, 2/3 and an accumulated y a hair from 1
    assert [p for p, _ in s][:5] == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1)]
    assert float(s[1][1]) == float(f32(1.0) - f32(f32(1.0) / f32(3.0))) and float(s[2][1]) == float(f32(f32(1.0) / f32(3.0)))


def test_blend_truncates():
    # By hand.  0.3f = 5033165 * 2^-24, so 1 - 0.3f = 11744051 * 2^-24 exactly (0.69999998807..).
    # * 200 = 139.9999976..; f32 has steps of 2^-16 there, the nearest is 140.0: f32 gives 140 where f64 arithmetic would give 139.
    assert dr.blend(200, 0, 0.3) == 140
    # * 255 = 178.4999969.. -> 178.5, and 0.3f * 255 = 76.5000030.. -> 76.5 (steps of 2^-17 there): the sum is 255 exactly.
    assert dr.blend(255, 255, 0.3) == 255
    assert dr.blend(100, 201, 0.5) == 150         # 50 + 100.5 = 150.5 exactly: truncated, not rounded
    assert dr.blend(10, 11, 0.999) == 10          # 0.00999987.. + 10.98900.. = 10.99899..: truncated
    assert dr.blend(0, 255, 1.0) == 255 and dr.blend(255, 0, 1.0) == 0
    assert dr.blend(77, 200, 0.0) == 77
    assert dr.f32_as_u8(float("nan")) == 0 and dr.f32_as_u8(-3.0) == 0 and dr.f32_as_u8(300.0) == 255 and dr.f32_as_u8(254.99) == 254


def test_resize_replicates_blocks():
    occ = di.raster()
    c = dr.RefCanvas(occ, di.LOW, di.UP, 3)
    assert c.img.shape == (48, 48, 3) and c.ppm == 24.0
    for i in range(48):
        for j in range(48):
            assert tuple(c.img[i, j]) == (occ[i // 3, j // 3],) * 3
    c1 = dr.RefCanvas(occ, di.LOW, di.UP, 1)
    assert np.array_equal(c1.img[:, :, 0], occ) and c1.ppm == 8.0
    # the transform uses the resized height
    assert c.to_pixel((-1.0, -1.0)) == (47, 0) and c1.to_pixel((-1.0, -1.0)) == (15, 0)
    assert c.to_pixel((-5.0, 5.0)) == (0, 0), "negative pixel coordinates saturate to 0"


def test_vectorised_line_is_the_scalar_line():
    for factor in (1, 3):
        a, b = dr.RefCanvas(di.raster(), di.LOW, di.UP, factor), dr.RefCanvas(di.raster(), di.LOW, di.UP, factor)
        for l in np.concatenate([di.octant_lines(), di.hub_lines(12)]):
            a.draw_line_scalar((l[0], l[1]), (l[2], l[3]), di.COLOR, 0.3)
            b.draw_line((l[0], l[1]), (l[2], l[3]), di.COLOR, 0.3)
        assert np.array_equal(a.img, b.img) and np.array_equal(a.count, b.count)


def test_cpp_line_is_the_scalar_line(tmp_path):
    """tests/draw_ref_line.cpp against the Python text, on every crafted set and on a policy with circles"""
    lib = dr.build_line_lib(tmp_path)
    for name, lines, factor, alpha, _ in di.CASES:
        if name in ("hub1100", "hub2100"):
            lines = lines[:150]
        a, b = dr.RefCanvas(di.raster(), di.LOW, di.UP, factor), dr.FastCanvas(lib, di.raster(), di.LOW, di.UP, factor)
        for l in lines:
            a.draw_line_scalar((l[0], l[1]), (l[2], l[3]), di.COLOR, alpha)
        b.draw_lines(lines, di.COLOR, alpha)
        assert np.array_equal(a.img, b.img) and np.array_equal(a.count, b.count), name
    a, b = dr.RefCanvas(di.raster(), di.LOW, di.UP, 5), dr.FastCanvas(lib, di.raster(), di.LOW, di.UP, 5)
    xy, parent = [(-0.5, -0.5), (-0.2, 0.0), (0.2, -0.3), (-0.4, 0.5), (0.0, 0.5), (0.6, 0.2)], [-1, 0, 0, 1, 1, 2]
    for c in (a, b):
        c.draw_zones_observability([(0.3, 0.3), (-0.9, 0.8)], 0.4)
        c.draw_policy(xy, parent)
    assert np.array_equal(a.img, b.img) and np.array_equal(a.count, b.count) and a.lines == b.lines


def _draw(lines, factor, alpha):
    c = dr.RefCanvas(di.raster(), di.LOW, di.UP, factor)
    c.draw_lines(lines, di.COLOR, alpha)
    return c


@pytest.mark.parametrize("name,lines,factor,alpha,heaviest", di.CASES, ids=["%s-f%d-a%g" % (c[0], c[2], c[3]) for c in di.CASES])
def test_gpu_inputs_have_teeth(name, lines, factor, alpha, heaviest):
    """the image depends on the draw order, and the hub pixel holds the count the GPU test claims"""
    fwd, rev = _draw(lines, factor, alpha), _draw(lines[::-1], factor, alpha)
    assert np.array_equal(fwd.count, rev.count)
    assert not np.array_equal(fwd.img, rev.img), "the order does not show"
    if heaviest is not None:
        assert int(fwd.count.max()) == heaviest
        assert int(fwd.count[fwd.to_pixel(di.HUB)]) == heaviest


def test_octant_lines_reach_the_edges():
    c = _draw(di.octant_lines(), 1, 1.0)
    assert c.count[:, 0].sum() > 0 and c.count[0, :].sum() > 0, "the saturated ends reach column 0 and row 0"
    assert c.count[:, 15].sum() > 0 and c.count[15, :].sum() > 0, "lines leave through the right and bottom edges"
    out = dr.RefCanvas(di.raster(), di.LOW, di.UP, 1)
    out.draw_lines(di.octant_lines()[-3:], di.COLOR, 1.0)
    assert int(out.count.sum()) == 1 and out.count[0, 0] == 1, "of the lines wholly outside only the one saturated into pixel (0, 0) leaves a fragment"


def test_pass_lines_hold_a_line_above_the_cap():
    c = dr.RefCanvas(di.raster(), di.LOW, di.UP, 1)
    l = di.pass_lines()[20]
    c.draw_line((l[0], l[1]), (l[2], l[3]), di.COLOR, 1.0)
    assert int(c.count.sum()) > 24, "the long line alone exceeds the cap of 24 fragments the GPU test sets"


def test_circle_and_policy_order():
    pts = dr.circle_points((0.1, 0.2), 0.5)
    assert len(pts) == 51 and pts[0] == (0.1 + 0.5 * math.cos(0.0), 0.2 + 0.5 * math.sin(0.0))
    assert len(dr.circle_lines((0.1, 0.2), 0.5)) == 50
    parent = [-1, 0, 0, 1, 1, 2]
    assert dr.policy_children(parent) == [[1, 2], [3, 4], [5], [], [], []]
    xy = [(-0.5, -0.5), (-0.2, 0.0), (0.2, -0.3), (-0.4, 0.5), (0.0, 0.5), (0.6, 0.2)]
    c = dr.RefCanvas(di.raster(), di.LOW, di.UP, 3)
    c.draw_policy(xy, parent)
    assert c.lines == 2 * 50 + 5, "two nodes with more than one child get a circle; five lines"


# ---- porrt_write_png: host code of the library
@pytest.fixture(scope="module")
def engine_mod():
    from po_rrt_amd import build, engine
    build.build()
    engine.load_library()
    return engine


@pytest.mark.parametrize("shape", [(21, 37), (160, 150), (1, 1)])
def test_write_png_reads_back(engine_mod, tmp_path, shape):
    """37 x 21, and an image whose rows exceed one stored block (160 rows of 451 bytes: 72 160 bytes > 65 535)"""
    from PIL import Image                     # (a missing package is a failure: this is the only check of the writer)
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    path = str(tmp_path / "out.png")
    engine_mod.write_png(path, img)
    with Image.open(path) as im:
        assert im.mode == "RGB" and im.size == (shape[1], shape[0])
        back = np.array(im)
    assert np.array_equal(back, img)


def test_write_png_errors(engine_mod, tmp_path):
    img = np.zeros((2, 2, 3), dtype=np.uint8)
    with pytest.raises(engine_mod.PorrtError) as e:
        engine_mod.write_png(str(tmp_path / "no_such_dir" / "x.png"), img)
    assert e.value.code == -7
