"""The reference's drawing functions, restated as plain sequential loops (map_shelves_io.rs:276-457; map_io.rs:303-479 is the same text
with alpha 0.15 in draw_full_graph): the canvas, resize, the pixel transform, the Xiaolin Wu walk, the blend, the circle and every draw
call.  Written from the algorithm; the device's images are compared with these byte for byte.

Two pieces are third-party arithmetic, recalled from the crates' published sources and not pinned by the reference tree:
  * line_drawing::XiaolinWu::<f32, i32> (wu_walk below): the walk this file states DEFINES the pixel walk of the project;
  * image::imageops::resize(.., FilterType::Nearest) at an integer factor: block replication, dst(j, i) = src(j // f, i // f).
All f32 arithmetic is numpy float32, one rounding per operation, no fused multiply-add.
"""
import ctypes
import math
import os
import subprocess

import numpy as np

f32 = np.float32

BLACK, TEAL, NAVY, GRAY5 = (0, 0, 0), (0, 128, 128), (0, 0, 128), (150, 150, 150)


def f64_as_u32(v):
    """Rust `f64 as u32`: toward zero, saturating, NaN -> 0"""
    if v != v or v <= 0.0:
        return 0
    if v >= 4294967295.0:
        return 4294967295
    return int(v)


def f32_as_u8(v):
    """Rust `f32 as u8`"""
    if v != v or v <= 0.0:
        return 0
    if v >= 255.0:
        return 255
    return int(v)


def blend(old, new, a):
    """((1.0 - alpha) * (old as f32) + alpha * (new as f32)) as u8 with alpha: f32 (map_shelves_io.rs:369-372)"""
    a = f32(a)
    keep = f32(f32(1.0) - a) * f32(old)
    add = a * f32(new)
    return f32_as_u8(float(f32(keep + add)))


def wu_walk(a, b):
    """XiaolinWu::<f32, i32>::new(a, b) as a list of ((x, y), weight): swap when steep, order by x, gradient = dy / dx (1 when dx == 0),
    start at round(x0) with y = y0; per x the pixel (x, y as i32) with weight 1 - fract(y), then, when fract(y) > 0, (x, that + 1) with weight
    fract(y); y += gradient in f32.  `y as i32` truncates toward zero (NumCast), which differs from floor only while y is in (-1, 0): an
    accumulated y that ends a hair below a line end on row or column 0."""
    ax, ay, bx, by = f32(a[0]), f32(a[1]), f32(b[0]), f32(b[1])
    steep = abs(f32(by - ay)) > abs(f32(bx - ax))
    if steep:
        ax, ay, bx, by = ay, ax, by, bx
    if ax > bx:
        ax, ay, bx, by = bx, by, ax, ay
    dx = f32(bx - ax)
    gradient = f32(1.0) if dx == 0 else f32(f32(by - ay) / dx)
    x, end_x, y = int(np.round(ax)), int(np.round(bx)), ay
    out = []
    while x <= end_x:
        fpart = f32(y - np.floor(y))
        yi = int(y)
        out.append(((yi, x) if steep else (x, yi), f32(f32(1.0) - fpart)))
        if fpart > 0:
            out.append(((yi + 1, x) if steep else (x, yi + 1), fpart))
        x += 1
        y = f32(y + gradient)
    return out


def wu_arrays(a, b):
    """the same walk as arrays (xs, ys, weights), vectorised over one line: np.add.accumulate adds strictly in sequence, in f32"""
    ax, ay, bx, by = f32(a[0]), f32(a[1]), f32(b[0]), f32(b[1])
    steep = abs(f32(by - ay)) > abs(f32(bx - ax))
    if steep:
        ax, ay, bx, by = ay, ax, by, bx
    if ax > bx:
        ax, ay, bx, by = bx, by, ax, ay
    dx = f32(bx - ax)
    gradient = f32(1.0) if dx == 0 else f32(f32(by - ay) / dx)
    x0, x1 = int(ax), int(bx)
    n = x1 - x0 + 1
    steps = np.full(n, gradient, dtype=f32)
    steps[0] = ay
    y = np.add.accumulate(steps, dtype=f32)
    fpart = (y - np.floor(y)).astype(f32)
    yi = np.trunc(y).astype(np.int64)
    xs = np.arange(x0, x1 + 1, dtype=np.int64)
    low = fpart > 0
    # the pairs of one x stand together: upper, then lower
    order = np.argsort(np.concatenate([2 * np.arange(n), 2 * np.arange(n)[low] + 1]), kind="stable")
    px = np.concatenate([xs, xs[low]])[order]
    py = np.concatenate([yi, yi[low] + 1])[order]
    w = np.concatenate([(f32(1.0) - fpart).astype(f32), fpart[low]])[order]
    return (py, px, w) if steep else (px, py, w)


def circle_points(xy, radius):
    """draw_circle's 51 points (map_shelves_io.rs:377-387), the host's libm"""
    pts = []
    for k in range(51):
        angle = float(k) * 2.0 * math.pi / 50.0
        pts.append((xy[0] + radius * math.cos(angle), xy[1] + radius * math.sin(angle)))
    return pts


def circle_lines(xy, radius):
    p = circle_points(xy, radius)
    return [(p[k - 1][0], p[k - 1][1], p[k][0], p[k][1]) for k in range(1, 51)]


def policy_children(parent):
    """children lists of a policy given by parents: ascending policy id (belief_graph.rs:203-207, pto_policy_refiner.rs:324-393)"""
    ch = [[] for _ in parent]
    for k, p in enumerate(parent):
        if p >= 0:
            ch[int(p)].append(k)
    return ch


def children_from_edges(n, efrom, eto):
    """PTOGraph's children lists from the forward edges in the reference's order (what porrt_graph_save_json writes): a node's neighbours at
    its creation first, then the later nodes that connected to it"""
    ch = [[] for _ in range(n)]
    for f, t in zip(efrom, eto):
        ch[int(t)].append(int(f))
    for f, t in zip(efrom, eto):
        ch[int(f)].append(int(t))
    return ch


class RefCanvas:
    """Map::open(..) + resize(factor): img as H x W x 3 uint8"""

    def __init__(self, occ, low=(-1.0, -1.0), up=(1.0, 1.0), factor=1):
        occ = np.asarray(occ, dtype=np.uint8)
        self.low = (float(low[0]), float(low[1]))
        self.ppm = float(occ.shape[1]) / (float(up[0]) - float(low[0]))
        gray = np.repeat(np.repeat(occ, factor, axis=0), factor, axis=1)            # Nearest at an integer factor
        self.ppm *= float(factor)
        self.img = np.repeat(gray[:, :, None], 3, axis=2).copy()
        self.H, self.W = gray.shape
        self.count = np.zeros((self.H, self.W), dtype=np.int64)                      # fragments per pixel since reset_count()
        self.lines = 0

    def reset_count(self):
        self.count[:] = 0
        self.lines = 0

    def to_pixel(self, xy):
        i = f64_as_u32(float(self.H - 1) - (xy[1] - self.low[1]) * self.ppm)
        j = f64_as_u32((xy[0] - self.low[0]) * self.ppm)
        return i, j

    def draw_line_scalar(self, a, b, color, alpha):
        """draw_line, pair by pair (the definition)"""
        ai, aj = self.to_pixel(a)
        bi, bj = self.to_pixel(b)
        self.lines += 1
        for (i, j), w in wu_walk((f32(ai), f32(aj)), (f32(bi), f32(bj))):
            if 0 <= i < self.H and 0 <= j < self.W:
                al = f32(f32(alpha) * w)
                for ch in range(3):
                    self.img[i, j, ch] = blend(self.img[i, j, ch], color[ch], al)
                self.count[i, j] += 1

    def draw_line(self, a, b, color, alpha):
        """draw_line with the pairs of the line blended at once (a line meets a pixel once, so they do not depend on each other)"""
        ai, aj = self.to_pixel(a)
        bi, bj = self.to_pixel(b)
        self.lines += 1
        pi, pj, w = wu_arrays((f32(ai), f32(aj)), (f32(bi), f32(bj)))
        ok = (pi >= 0) & (pi < self.H) & (pj >= 0) & (pj < self.W)
        pi, pj, w = pi[ok], pj[ok], w[ok]
        al = (f32(alpha) * w).astype(f32)
        old = self.img[pi, pj, :].astype(f32)
        keep = ((f32(1.0) - al).astype(f32)[:, None] * old).astype(f32)
        add = (al[:, None] * np.asarray(color, dtype=f32)[None, :]).astype(f32)
        v = (keep + add).astype(f32)
        self.img[pi, pj, :] = np.clip(np.trunc(v), 0, 255).astype(np.uint8)
        np.add.at(self.count, (pi, pj), 1)

    # ---- the draw calls
    def draw_lines(self, ab, color, alpha):
        for l in ab:
            self.draw_line((l[0], l[1]), (l[2], l[3]), color, alpha)

    def draw_path(self, path, color):
        for k in range(1, len(path)):
            self.draw_line(path[k - 1], path[k], color, 1.0)

    def draw_circle(self, xy, radius, color):
        for l in circle_lines(xy, radius):
            self.draw_line((l[0], l[1]), (l[2], l[3]), color, 1.0)

    def draw_tree(self, xy, parent):
        for k in range(len(parent)):
            if parent[k] >= 0:
                self.draw_line(xy[int(parent[k])], xy[k], TEAL, 0.3)

    def draw_full_graph(self, xy, children, door=False):
        for f in range(len(children)):
            for t in children[f]:
                self.draw_line(xy[f], xy[t], GRAY5, 0.15 if door else 0.25)

    def draw_policy(self, xy, parent):
        ch = policy_children(parent)
        for p in range(len(parent)):
            if len(ch[p]) > 1:
                self.draw_circle(xy[p], 0.025, NAVY)
            for c in ch[p]:
                self.draw_line(xy[p], xy[c], BLACK, 1.0)

    def draw_zones_observability(self, zone_positions, visibility):
        for z in zone_positions:
            self.draw_circle(z, visibility, TEAL)


def build_line_lib(out_dir):
    """tests/draw_ref_line.cpp (draw_line once more, in C++) as a shared object in out_dir"""
    here = os.path.dirname(os.path.abspath(__file__))
    so = os.path.join(str(out_dir), "libdraw_ref_line.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(here, "draw_ref_line.cpp")], check=True)
    lib = ctypes.CDLL(so)
    lib.draw_ref_line.restype = None
    lib.draw_ref_line.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float]
    lib.draw_ref_lines.restype = None
    lib.draw_ref_lines.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                   ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_float]
    return lib


class FastCanvas(RefCanvas):
    """RefCanvas whose draw_line is the C++ text: every draw call above stays the same Python loop"""

    def __init__(self, lib, occ, low=(-1.0, -1.0), up=(1.0, 1.0), factor=1):
        super().__init__(occ, low, up, factor)
        self._lib = lib
        self.img = np.ascontiguousarray(self.img)
        self._ab = np.zeros(4, dtype=np.float64)
        self._rgb = np.zeros(3, dtype=np.uint8)

    def draw_line(self, a, b, color, alpha):
        self.lines += 1
        self._ab[0], self._ab[1], self._ab[2], self._ab[3] = a[0], a[1], b[0], b[1]
        self._rgb[:] = color
        self._lib.draw_ref_line(self.img.ctypes.data, self.count.ctypes.data, self.W, self.H, self.low[0], self.low[1], self.ppm, self._ab.ctypes.data,
                                self._rgb.ctypes.data, float(alpha))

    def draw_lines(self, ab, color, alpha):
        ab = np.ascontiguousarray(ab, dtype=np.float64).reshape(-1, 4)
        self.lines += len(ab)
        self._rgb[:] = color
        self._lib.draw_ref_lines(self.img.ctypes.data, self.count.ctypes.data, self.W, self.H, self.low[0], self.low[1], self.ppm, ab.ctypes.data, len(ab),
                                 self._rgb.ctypes.data, float(alpha))
