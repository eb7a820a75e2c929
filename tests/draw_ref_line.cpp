// draw_ref_line.cpp -- draw_line of tests/draw_ref.py (RefCanvas.draw_line_scalar) once more in C++, for the tests whose pictures hold
// hundreds of thousands of lines: the same sequential loop, one pair at a time.  Built by the tests with g++ -O2 -ffp-contract=off as a
// shared object; tests/test_draw_cpu.py checks it against the Python text, which stays the definition.
#include <cmath>
#include <cstdint>

namespace {

uint32_t f64_as_u32(double v) {                      // Rust `f64 as u32`
    if (!(v == v) || v <= 0.0) return 0u;
    if (v >= 4294967295.0) return 4294967295u;
    return (uint32_t)v;
}
uint8_t f32_as_u8(float v) {                         // Rust `f32 as u8`
    if (!(v == v) || v <= 0.0f) return 0;
    if (v >= 255.0f) return 255;
    return (uint8_t)v;
}

} // namespace

extern "C" void draw_ref_line(uint8_t *img, int64_t *count, uint32_t W, uint32_t H, double low0, double low1, double ppm, const double *ab, const uint8_t *rgb,
                              float alpha) {
    const uint32_t ai = f64_as_u32((double)(H - 1) - (ab[1] - low1) * ppm), aj = f64_as_u32((ab[0] - low0) * ppm);
    const uint32_t bi = f64_as_u32((double)(H - 1) - (ab[3] - low1) * ppm), bj = f64_as_u32((ab[2] - low0) * ppm);
    float ax = (float)ai, ay = (float)aj, bx = (float)bi, by = (float)bj;
    const bool steep = std::fabs(by - ay) > std::fabs(bx - ax);
    if (steep) { float t = ax; ax = ay; ay = t; t = bx; bx = by; by = t; }
    if (ax > bx) { float t = ax; ax = bx; bx = t; t = ay; ay = by; by = t; }
    const float dx = bx - ax;
    const float gradient = dx == 0.0f ? 1.0f : (by - ay) / dx;
    const long end_x = std::lround(bx);
    float y = ay;
    for (long x = std::lround(ax); x <= end_x; ++x) {
        const float fpart = y - std::floor(y);
        const long yi = (long)y;
        for (int lower = 0; lower < 2; ++lower) {
            if (lower && !(fpart > 0.0f)) break;
            const long yy = yi + lower, i = steep ? yy : x, j = steep ? x : yy;
            const float line_alpha = lower ? fpart : 1.0f - fpart;
            if (0 <= i && i < (long)H && 0 <= j && j < (long)W) {
                uint8_t *px = img + 3 * ((size_t)i * W + (size_t)j);
                const float a = alpha * line_alpha;
                for (int ch = 0; ch < 3; ++ch) {
                    const float keep = (1.0f - a) * (float)px[ch], add = a * (float)rgb[ch];
                    px[ch] = f32_as_u8(keep + add);
                }
                if (count) ++count[(size_t)i * W + (size_t)j];
            }
        }
        y += gradient;
    }
}

// n lines (4 doubles each) of one colour, in order: the loop of a draw call (tools/draw_probe.py times it as the host baseline)
extern "C" void draw_ref_lines(uint8_t *img, int64_t *count, uint32_t W, uint32_t H, double low0, double low1, double ppm, const double *ab, uint64_t n,
                               const uint8_t *rgb, float alpha) {
    for (uint64_t k = 0; k < n; ++k) draw_ref_line(img, count, W, H, low0, low1, ppm, ab + 4 * k, rgb, alpha);
}
