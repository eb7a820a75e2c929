"""Crafted line sets for the drawing tests on a 16 x 16 raster over [-1, 1)^2 (ppm 8; ppm 24 at factor 3).  test_draw_cpu.py asserts from the
restatement that each set has teeth (its image depends on the draw order; its heaviest pixel holds the count claimed here);
test_gpu_draw.py draws the same sets on the device."""
import math

import numpy as np

LOW, UP = (-1.0, -1.0), (1.0, 1.0)
COLOR = (200, 30, 90)


def raster():
    """16 x 16 gray values that differ from pixel to pixel (so that a blend shows) with a few saturated ones"""
    i, j = np.mgrid[0:16, 0:16]
    occ = ((37 * i + 11 * j + 5 * i * j) % 256).astype(np.uint8)
    occ[0, 0], occ[15, 15], occ[7, 8] = 255, 0, 255
    return occ


def octant_lines():
    """from near the centre into all eight octants and back (reversed ends), horizontal, vertical, exact diagonals, zero length; lines partly
    and wholly outside: negative pixel coordinates saturate to 0, coordinates beyond the right and bottom edges stay outside"""
    c = (0.05, -0.05)
    lines = []
    for k in range(16):
        ang = (k + 0.5) * math.pi / 8.0                                            # two per octant, none on an axis or a diagonal
        e = (c[0] + 0.8 * math.cos(ang), c[1] + 0.8 * math.sin(ang))
        lines.append(c + e)
        lines.append(e + c)
    lines += [(-0.7, 0.3, 0.6, 0.3), (0.6, -0.4, -0.7, -0.4),                      # horizontal, both ways
              (0.2, -0.8, 0.2, 0.7), (-0.3, 0.7, -0.3, -0.8),                      # vertical
              (-0.8, -0.8, 0.7, 0.7), (0.7, -0.8, -0.8, 0.7),                      # exact diagonals
              (0.4, 0.4, 0.4, 0.4), (-0.55, 0.1, -0.5, 0.12)]                      # zero length: the same point, two points of one pixel
    lines += [(-1.6, 0.2, 0.3, 0.5), (0.1, 1.7, 0.5, -0.2),                        # left of the map / above it: the end saturates to 0
              (0.3, 0.1, 1.9, 0.6), (0.2, 0.3, -0.4, -1.8),                        # beyond the right edge / below the bottom: pairs outside are skipped
              (1.3, -0.5, 1.8, 0.4), (-0.5, -1.4, 0.6, -1.9),                      # wholly outside, right / below
              (-1.5, 1.5, -1.2, 1.9)]                                              # wholly outside the box, both ends saturate to pixel (0, 0)
    return np.array(lines, dtype=np.float64)


HUB = (0.3, 0.2)            # every hub line ends here
HUB_SMALL, HUB_LARGE, HUB_HUGE = 70, 1100, 2100          # one wave and more; two sorted runs of 1024; three


def hub_lines(n):
    """n lines from varied starts that all end at HUB: its pixel holds one fragment per line"""
    lines = []
    for k in range(n):
        ang = 2.0 * math.pi * ((k * 0.6180339887498949) % 1.0)
        r = 0.35 + 0.5 * ((k * 37) % 101) / 101.0
        lines.append((HUB[0] + r * math.cos(ang), HUB[1] + r * math.sin(ang), HUB[0], HUB[1]))
    return np.array(lines, dtype=np.float64)


def pass_lines():
    """for the several-pass test: the small hub set with three long lines in it (a corner-to-corner diagonal holds more fragments than the
    test's cap on its own)"""
    h = hub_lines(HUB_SMALL)
    long_lines = np.array([(-0.95, -0.9, 0.95, 0.8), (-0.9, 0.9, 0.9, -0.95), (0.9, 0.85, -0.95, -0.6)], dtype=np.float64)
    return np.concatenate([h[:20], long_lines[:1], h[20:50], long_lines[1:2], h[50:], long_lines[2:]])


def invalid_lines():
    """(lines, what): each set has one line the device refuses -- a non-finite coordinate, or a pixel end beyond 2^24"""
    ok = octant_lines()[:6]
    out = []
    for bad, what in (((0.1, float("nan"), 0.2, 0.3), "nan"), ((float("inf"), 0.0, 0.2, 0.3), "inf"), ((0.1, 0.1, 0.2, -float("inf")), "-inf"),
                      ((0.0, 0.0, 3.0e6, 0.0), "x beyond 2^24 pixels"), ((0.0, 0.0, 0.0, -3.0e6), "y beyond 2^24 pixels")):
        out.append((np.concatenate([ok[:3], np.array([bad]), ok[3:]]), what))
    return out


# (name, lines, factor, alpha, fragments on the heaviest pixel or None): every combination the GPU tests draw
CASES = [("octants", octant_lines(), f, a, None) for f in (1, 3) for a in (1.0, 0.3)] + [
    ("hub70", hub_lines(HUB_SMALL), 1, 0.3, HUB_SMALL), ("hub70", hub_lines(HUB_SMALL), 3, 1.0, HUB_SMALL),
    ("hub1100", hub_lines(HUB_LARGE), 3, 0.3, HUB_LARGE), ("hub2100", hub_lines(HUB_HUGE), 3, 0.3, HUB_HUGE), ("passes", pass_lines(), 1, 0.3, None)]
