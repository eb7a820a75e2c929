// porrt_draw.hpp -- the reference's figures on the device: the canvas of MapShelfDomain / Map (map_shelves_io.rs:276-457,
// map_io.rs:303-479: resize, draw_line, draw_circle, draw_tree, draw_full_graph, draw_policy, draw_path,
// draw_zones_observability) as a deterministic, ordered scatter-and-composite.
//
// draw_line blends every pixel of a Xiaolin Wu walk into the image in f32 and truncates to u8, so what a pixel ends as depends on
// the ORDER in which the lines of a call reach it.  Every draw call is therefore an ordered list of lines (line k's key is its
// place in the reference's loop) and runs store-then-resolve, never read-modify-write on the image:
//   count    one lane per line walks the iterator (it is sequential in f32: y += gradient) and counts the fragments of every pixel
//            (integer atomics) and of every line;
//   scan     the pixels' counts become the pixels' segments of one record array;
//   scatter  the same walk stores (key, alpha * line_alpha) into the pixel's segment, in whatever order the atomics hand out;
//   resolve  every pixel puts its records into key order and applies the blends in that order to its three channels.  A line meets a
//            pixel at most once, so the key alone orders a pixel's records.
// Pixels are very unequal (the bench tree has some 900 copies of the goal point: a thousand fragments on one pixel, a dozen on most):
// a pixel of at most "draw_heavy_cap" records is resolved by one lane (it picks the next key among its records again and again);
// a longer one of at most 64 records goes to a list and gets one wave (a record a lane, ranked by shuffles, applied from LDS in
// order by one lane); a longer one still goes to a second list and gets a workgroup: runs of kDrawTrip records are sorted in LDS (bitonic); a list of one run is
// applied from LDS, a longer one has its sorted runs written back, every record finds its place among all runs (its place in its
// own run + binary searches in the others) in a second array, and that array is applied a trip at a time through LDS.
// A call whose fragments exceed "draw_max_fragments" runs in several passes over consecutive ranges of lines, cut at line
// boundaries by the per-line counts (a single line above the cap is a pass of its own; nothing is truncated): a pass blends onto
// the image the pass before left, so passes in draw order compose exactly.
//
// Third-party arithmetic, recalled from the crates' published sources and not pinned by the reference tree (README, parity):
// line_drawing::XiaolinWu<f32, i32> (swap when steep, order by x, gradient = dy / dx or 1 when dx == 0, start at round(x0) with
// y = y0; per x the pixel (x, y as i32) with weight 1 - fract and, when fract > 0, (x, that + 1) with weight fract; y += gradient)
// and image's Nearest resize at an integer factor (block replication).  tests/draw_ref.py is the restatement the device must match.
//
// Ours, not the reference's: a line with a non-finite coordinate, or whose pixel end lies beyond 2^24 (the reference would walk
// billions of pixels), is PORRT_ERR_INVALID and the canvas is left as it was; a canvas of more than kDrawMaxSide pixels a side is
// PORRT_ERR_CAPACITY.
#pragma once

namespace porrt {

constexpr uint32_t kDrawMaxSide = 16384;
constexpr uint32_t kDrawMaxPixel = 1u << 24;
constexpr uint32_t kDrawTrip = 1024;                    // records of one LDS sort of the heavy form
// (kDrawHeavyCapDefault / Limit and kDrawMaxFragmentsDefault / Limit stand before the context, in porrt_engine.hip)
constexpr uint32_t kDrawNoLine = 0x80000000u;           // DrawLine::i0 of a place in the order that draws nothing (a node without parent)

struct DrawGeom { double low0, low1, ppm; uint32_t W, H; };
struct DrawLine { int i0, j0, i1, j1; };
struct DrawStats { uint32_t heaviest, n_heavy, n_wave, pad; };
constexpr uint32_t kDrawWave = 64;                      // records of the one-wave form

// Rust `f32 as u8`: truncate toward zero, saturate, NaN -> 0
__device__ __forceinline__ uint32_t f32_as_u8(float v) {
    if (!(v == v)) return 0u;
    if (v <= 0.0f) return 0u;
    if (v >= 255.0f) return 255u;
    return (uint32_t)v;
}
// pixel.apply2(&color, |old, new| ((1.0 - alpha) * (old as f32) + alpha * (new as f32)) as u8), map_shelves_io.rs:369-372
__device__ __forceinline__ uint32_t draw_blend(uint32_t old, uint32_t nw, float a) {
    const float keep = (1.0f - a) * (float)old, add = a * (float)nw;
    return f32_as_u8(keep + add);
}

// to_pixel_coordinates (map_shelves_io.rs:165-170) on the canvas: its ppm and its height
__device__ __forceinline__ bool draw_to_pixel(const DrawGeom &g, double x, double y, int &i, int &j, uint32_t &bad) {
    if (!(x - x == 0.0) || !(y - y == 0.0)) { bad |= 1u; return false; }
    const double t = (y - g.low1) * g.ppm;
    const uint32_t ui = f64_as_u32((double)(g.H - 1) - t), uj = f64_as_u32((x - g.low0) * g.ppm);
    if (ui > kDrawMaxPixel || uj > kDrawMaxPixel) { bad |= 2u; return false; }
    i = (int)ui; j = (int)uj;
    return true;
}
__device__ __forceinline__ void draw_make_line(const DrawGeom &g, double ax, double ay, double bx, double by, DrawLine &l, uint32_t *bad) {
    uint32_t b = 0;
    l.i0 = (int)kDrawNoLine; l.j0 = l.i1 = l.j1 = 0;
    int i0, j0, i1, j1;
    if (draw_to_pixel(g, ax, ay, i0, j0, b) & draw_to_pixel(g, bx, by, i1, j1, b)) { l.i0 = i0; l.j0 = j0; l.i1 = i1; l.j1 = j1; }
    if (b) atomicOr(bad, b);
}

// line_drawing::XiaolinWu::<f32, i32>::new((i0, j0), (i1, j1)) walked to its end: emit(pixel index, line_alpha) for every pair inside
// the image.  Returns the number of pairs emitted.  div64: the gradient through the f64 divide (exact for f32 operands: 53 >= 2 * 24 + 2
// bits make the second rounding innocuous), for a device whose f32 divide did not pass the canvas's sweep.
template <class F>
__device__ __forceinline__ uint32_t draw_wu_walk(const DrawLine &l, uint32_t W, uint32_t H, uint32_t div64, F emit) {
    float ax = (float)l.i0, ay = (float)l.j0, bx = (float)l.i1, by = (float)l.j1;
    const bool steep = fabsf(by - ay) > fabsf(bx - ax);
    if (steep) { float t = ax; ax = ay; ay = t; t = bx; bx = by; by = t; }
    if (ax > bx) { float t = ax; ax = bx; bx = t; t = ay; ay = by; by = t; }
    const float dx = bx - ax;
    float gradient = 1.0f;
    if (dx != 0.0f) gradient = div64 ? (float)((double)(by - ay) / (double)dx) : (by - ay) / dx;
    const int end_x = (int)bx;
    float y = ay;
    uint32_t n = 0;
    for (int x = (int)ax; x <= end_x; ++x) {
        const float fpart = y - floorf(y);
        const int yi = (int)y;                                  // O::cast(self.y): toward zero
        for (int lower = 0; lower < 2; ++lower) {
            if (lower && !(fpart > 0.0f)) break;
            const int yy = yi + lower;
            const int pi = steep ? yy : x, pj = steep ? x : yy;
            if (pi >= 0 && pi < (int)H && pj >= 0 && pj < (int)W) { emit((uint32_t)pi * W + (uint32_t)pj, lower ? fpart : 1.0f - fpart); ++n; }
        }
        y += gradient;
    }
    return n;
}

// Map::open + resize(factor): the occupancy raster as RGB8 (DynamicImage::ImageLuma8(img).to_rgb8()), Nearest at an integer factor
__global__ __launch_bounds__(256) void k_draw_canvas(const uint8_t *__restrict__ occ, uint32_t W0, uint32_t factor, uint32_t W, uint32_t H, uint8_t *__restrict__ rgb) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (size_t)W * H) return;
    const uint32_t i = (uint32_t)(p / W), j = (uint32_t)(p % W);
    const uint8_t v = occ[(size_t)(i / factor) * W0 + j / factor];
    rgb[3 * p] = v; rgb[3 * p + 1] = v; rgb[3 * p + 2] = v;
}

__global__ __launch_bounds__(256) void k_draw_divtest(const float *__restrict__ num, const float *__restrict__ den, float *__restrict__ out, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = num[t] / den[t];
}

// ---- the lines of a call, in draw order
__global__ __launch_bounds__(256) void k_draw_lines_host(const double *__restrict__ ab, uint32_t n, DrawGeom g, DrawLine *__restrict__ out, uint32_t *__restrict__ bad) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    DrawLine l;
    draw_make_line(g, ab[4 * (size_t)k], ab[4 * (size_t)k + 1], ab[4 * (size_t)k + 2], ab[4 * (size_t)k + 3], l, bad);
    out[k] = l;
}
// draw_tree (map_shelves_io.rs:313-321): nodes in id order, parent -> node; a node without parent holds its place and draws nothing
__global__ __launch_bounds__(256) void k_draw_lines_tree(const double *__restrict__ nx, const double *__restrict__ ny, const int *__restrict__ parent, uint32_t n, DrawGeom g,
                                                         DrawLine *__restrict__ out, uint32_t *__restrict__ bad) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    DrawLine l;
    l.i0 = (int)kDrawNoLine; l.j0 = l.i1 = l.j1 = 0;
    const int p = parent[k];
    if (p >= 0 && (uint32_t)p < n) draw_make_line(g, nx[p], ny[p], nx[k], ny[k], l, bad);
    out[k] = l;
}
// draw_full_graph (:389-400): nodes in id order, each node's children in push order -- slot k of the adjacency lists, whose owner is
// the last node whose offset is at or below k
__global__ __launch_bounds__(256) void k_draw_lines_graph(const double *__restrict__ nx, const double *__restrict__ ny, const unsigned long long *__restrict__ adj_off,
                                                          const uint32_t *__restrict__ adj_id, uint32_t N, uint32_t n, DrawGeom g, DrawLine *__restrict__ out,
                                                          uint32_t *__restrict__ bad) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    uint32_t lo = 0, hi = N;                                    // adj_off[lo] <= k < adj_off[hi]
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (adj_off[mid] <= k) lo = mid; else hi = mid; }
    const uint32_t to = adj_id[k];
    DrawLine l;
    l.i0 = (int)kDrawNoLine; l.j0 = l.i1 = l.j1 = 0;
    if (to < N) draw_make_line(g, nx[lo], ny[lo], nx[to], ny[to], l, bad);
    out[k] = l;
}

// ---- count, cut, scatter
__global__ __launch_bounds__(256) void k_draw_count(const DrawLine *__restrict__ lines, uint32_t s, uint32_t e, uint32_t W, uint32_t H, uint32_t div64,
                                                    uint32_t *__restrict__ cnt, uint32_t *__restrict__ line_frag) {
    const uint32_t k = s + blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= e) return;
    const DrawLine l = lines[k];
    uint32_t n = 0;
    if ((uint32_t)l.i0 != kDrawNoLine) n = draw_wu_walk(l, W, H, div64, [&](uint32_t p, float) { atomicAdd(&cnt[p], 1u); });
    if (line_frag) line_frag[k] = n;
}
// the end of the pass that begins at line s: the most lines whose fragments stay at or below cap, one line at the least
__global__ void k_draw_cut(const unsigned long long *__restrict__ line_off, uint32_t s, uint32_t n, unsigned long long cap, unsigned long long *__restrict__ out) {
    if (blockIdx.x || threadIdx.x) return;
    const unsigned long long base = line_off[s];
    uint32_t lo = s + 1, hi = n;                                // the answer lies in [lo, hi]
    while (lo < hi) { const uint32_t mid = lo + (hi - lo + 1) / 2; if (line_off[mid] - base <= cap) lo = mid; else hi = mid - 1; }
    out[0] = lo; out[1] = line_off[lo] - base;
}
__global__ __launch_bounds__(256) void k_draw_scatter(const DrawLine *__restrict__ lines, const uint8_t *__restrict__ style, uint32_t s, uint32_t e, uint32_t W, uint32_t H,
                                                      uint32_t div64, float alpha, const unsigned long long *__restrict__ off, uint32_t *__restrict__ cur,
                                                      uint2 *__restrict__ rec) {
    const uint32_t k = s + blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= e) return;
    const DrawLine l = lines[k];
    if ((uint32_t)l.i0 == kDrawNoLine) return;
    const uint32_t key = ((k - s) << 1) | (style ? (uint32_t)style[k] : 0u);
    draw_wu_walk(l, W, H, div64, [&](uint32_t p, float line_alpha) {
        const unsigned long long at = off[p] + atomicAdd(&cur[p], 1u);
        rec[at] = make_uint2(key, __float_as_uint(alpha * line_alpha));                // let alpha = alpha * line_alpha
    });
}

// ---- resolve
struct DrawColors { uint32_t rgb[2][3]; };
__device__ __forceinline__ void draw_apply(uint32_t (&px)[3], const DrawColors &col, uint2 r) {
    const float a = __uint_as_float(r.y);
    const uint32_t st = r.x & 1u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) px[ch] = draw_blend(px[ch], col.rgb[st][ch], a);
}
// one lane per pixel: a pixel of at most heavy_cap records takes the least key above the last one applied, again and again; a longer
// one is listed for k_draw_resolve_wave (up to 64 records) or for k_draw_resolve_heavy
__global__ __launch_bounds__(256) void k_draw_resolve_light(const unsigned long long *__restrict__ off, const uint2 *__restrict__ rec, uint32_t P, uint32_t heavy_cap,
                                                            DrawColors col, uint8_t *__restrict__ rgb, uint32_t *__restrict__ heavy, uint32_t *__restrict__ medium,
                                                            DrawStats *__restrict__ stats) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long a = 0;
    uint32_t L = 0;
    if (p < P) { a = off[p]; L = (uint32_t)(off[p + 1] - a); }
    uint32_t mx = L;
    for (uint32_t s = 32; s >= 1; s >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)mx, (int)s); mx = o > mx ? o : mx; }
    if ((threadIdx.x & 63u) == 0 && mx) atomicMax(&stats->heaviest, mx);
    if (!L) return;
    if (L > heavy_cap) {
        if (L <= kDrawWave) medium[atomicAdd(&stats->n_wave, 1u)] = p;
        else heavy[atomicAdd(&stats->n_heavy, 1u)] = p;
        return;
    }
    uint32_t px[3] = {rgb[3 * (size_t)p], rgb[3 * (size_t)p + 1], rgb[3 * (size_t)p + 2]};
    long long last = -1;
    for (uint32_t t = 0; t < L; ++t) {
        uint2 best = make_uint2(0xFFFFFFFFu, 0u);
        for (uint32_t q = 0; q < L; ++q) {
            const uint2 r = rec[a + q];
            if ((long long)r.x > last && r.x <= best.x) best = r;
        }
        draw_apply(px, col, best);
        last = (long long)best.x;
    }
    rgb[3 * (size_t)p] = (uint8_t)px[0]; rgb[3 * (size_t)p + 1] = (uint8_t)px[1]; rgb[3 * (size_t)p + 2] = (uint8_t)px[2];
}
// one wave per listed pixel of at most 64 records: a lane holds a record, counts the keys below its own (the others' keys come by
// shuffle) and puts the record at that place in LDS; one lane applies them.  The grid covers the list's bound; waves beyond its length leave.
__global__ __launch_bounds__(256) void k_draw_resolve_wave(const unsigned long long *__restrict__ off, const uint2 *__restrict__ rec, const uint32_t *__restrict__ medium,
                                                           const DrawStats *__restrict__ stats, DrawColors col, uint8_t *__restrict__ rgb) {
    __shared__ uint2 s_rec[4][kDrawWave];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t idx = blockIdx.x * 4u + wv;
    if (idx >= stats->n_wave) return;
    const uint32_t p = medium[idx];
    const unsigned long long a = off[p];
    const uint32_t L = (uint32_t)(off[p + 1] - a);
    const uint2 me = lane < L ? rec[a + lane] : make_uint2(0xFFFFFFFFu, 0u);
    uint32_t rank = 0;
    for (uint32_t j = 0; j < L; ++j) rank += ((uint32_t)__shfl((int)me.x, (int)j) < me.x) ? 1u : 0u;
    if (lane < L) s_rec[wv][rank] = me;
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        uint32_t px[3] = {rgb[3 * (size_t)p], rgb[3 * (size_t)p + 1], rgb[3 * (size_t)p + 2]};
        for (uint32_t i = 0; i < L; ++i) draw_apply(px, col, s_rec[wv][i]);
        rgb[3 * (size_t)p] = (uint8_t)px[0]; rgb[3 * (size_t)p + 1] = (uint8_t)px[1]; rgb[3 * (size_t)p + 2] = (uint8_t)px[2];
    }
}
// one workgroup per listed pixel (the grid covers the list's bound; workgroups beyond its length leave)
__global__ __launch_bounds__(256) void k_draw_resolve_heavy(const unsigned long long *__restrict__ off, uint2 *rec, uint2 *rec2, const uint32_t *__restrict__ heavy,
                                                            const DrawStats *__restrict__ stats, DrawColors col, uint8_t *__restrict__ rgb) {
    __shared__ uint2 s_rec[kDrawTrip];
    __shared__ uint32_t s_px[3];
    if (blockIdx.x >= stats->n_heavy) return;
    const uint32_t p = heavy[blockIdx.x], tid = threadIdx.x;
    const unsigned long long a = off[p];
    const uint32_t L = (uint32_t)(off[p + 1] - a);
    const uint32_t n_runs = (L + kDrawTrip - 1) / kDrawTrip;
    if (tid < 3) s_px[tid] = rgb[3 * (size_t)p + tid];
    for (uint32_t r = 0; r < n_runs; ++r) {
        const uint32_t base = r * kDrawTrip, len = L - base < kDrawTrip ? L - base : kDrawTrip;
        uint32_t n2 = 2;
        while (n2 < len) n2 <<= 1;
        __syncthreads();
        for (uint32_t i = tid; i < n2; i += blockDim.x) s_rec[i] = i < len ? rec[a + base + i] : make_uint2(0xFFFFFFFFu, 0u);
        __syncthreads();
        for (uint32_t k = 2; k <= n2; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t i = tid; i < n2; i += blockDim.x) {
                    const uint32_t x = i ^ j;
                    if (x > i) {
                        const uint2 u = s_rec[i], v = s_rec[x];
                        if ((u.x > v.x) == ((i & k) == 0)) { s_rec[i] = v; s_rec[x] = u; }
                    }
                }
                __syncthreads();
            }
        if (n_runs == 1) {
            if (tid == 0) {
                uint32_t px[3] = {s_px[0], s_px[1], s_px[2]};
                for (uint32_t i = 0; i < len; ++i) draw_apply(px, col, s_rec[i]);
                rgb[3 * (size_t)p] = (uint8_t)px[0]; rgb[3 * (size_t)p + 1] = (uint8_t)px[1]; rgb[3 * (size_t)p + 2] = (uint8_t)px[2];
            }
            return;
        }
        for (uint32_t i = tid; i < len; i += blockDim.x) rec[a + base + i] = s_rec[i];
    }
    __threadfence_block();
    __syncthreads();
    // every record's place among all runs: its place in its own run + the keys below it in each of the others (keys are distinct)
    for (uint32_t i = tid; i < L; i += blockDim.x) {
        const uint2 me = rec[a + i];
        const uint32_t own = i / kDrawTrip;
        uint32_t rank = i % kDrawTrip;
        for (uint32_t r = 0; r < n_runs; ++r) {
            if (r == own) continue;
            const uint32_t base = r * kDrawTrip, len = L - base < kDrawTrip ? L - base : kDrawTrip;
            uint32_t lo = 0, hi = len;                          // records of run r below me.x
            while (lo < hi) { const uint32_t mid = (lo + hi) / 2; if (rec[a + base + mid].x < me.x) lo = mid + 1; else hi = mid; }
            rank += lo;
        }
        rec2[a + rank] = me;
    }
    __threadfence_block();
    __syncthreads();
    for (uint32_t t0 = 0; t0 < L; t0 += kDrawTrip) {
        const uint32_t len = L - t0 < kDrawTrip ? L - t0 : kDrawTrip;
        __syncthreads();
        for (uint32_t i = tid; i < len; i += blockDim.x) s_rec[i] = rec2[a + t0 + i];
        __syncthreads();
        if (tid == 0) {
            uint32_t px[3] = {s_px[0], s_px[1], s_px[2]};
            for (uint32_t i = 0; i < len; ++i) draw_apply(px, col, s_rec[i]);
            s_px[0] = px[0]; s_px[1] = px[1]; s_px[2] = px[2];
        }
    }
    if (tid == 0) { rgb[3 * (size_t)p] = (uint8_t)s_px[0]; rgb[3 * (size_t)p + 1] = (uint8_t)s_px[1]; rgb[3 * (size_t)p + 2] = (uint8_t)s_px[2]; }
}

} // namespace porrt

// ---------------------------------------------------------------------------------------------------------------- host side
struct porrt_canvas {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    void set_err(const std::string &s) { err = s; }
    // the context's raster geometry (what a context drawn from must share) and the canvas's own
    uint32_t W0 = 0, H0 = 0, factor = 1, W = 0, H = 0;
    double low[2] = {0, 0}, ppm0 = 0, ppm = 0;
    int domain = 0;
    int n_zones = 0;
    double zone_pos[64][2];
    double visibility = 0;
    uint64_t max_fragments = porrt::kDrawMaxFragmentsDefault;
    uint32_t heavy_cap = porrt::kDrawHeavyCapDefault;
    uint32_t div64 = 0;                    // 1: the f32 divide of this device failed the sweep, gradients go through the f64 divide
    uint8_t *d_rgb = nullptr;
    GrowScratch sc;                        // 0 lines, 1 styles, 2 bad flag + cut + stats, 3 per-line counts, 4 their scan, 5 scan totals, 6 pixel counts / cursors,
                                           // 7 pixel offsets, 8 records, 9 records in order (heavy pixels of several runs), 10 heavy pixel list, 11 host coordinates,
                                           // 12 the list of the one-wave form
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    struct porrt_draw_info info = {};
    porrt::DrawGeom geom() const { return porrt::DrawGeom{low[0], low[1], ppm, W, H}; }
};

namespace porrt {

#define DRAW_HIP(expr) HIPCHK_CTX(cv, expr)

// the f32 divide against the host's, on the quotients a gradient can be: integer-valued operands up to 2^24
static int draw_div_sweep(porrt_canvas *cv) {
    const uint32_t n = 1u << 16;
    std::vector<float> num(n), den(n), out(n);
    Pcg64 r;
    r.seed_from_u64(2024);
    uint32_t t = 0;
    for (int dy = -64; dy <= 64 && t < n / 2; ++dy)
        for (int dx = 1; dx <= 254 && t < n / 2; ++dx) { num[t] = (float)dy; den[t] = (float)dx; ++t; }
    for (; t < n; ++t) {
        const uint32_t sh = (uint32_t)(r.next_u64() % 24);
        den[t] = (float)(1 + (r.next_u64() >> 40 >> sh));                       // 1 .. 2^24
        const int64_t d = (int64_t)den[t];
        num[t] = (float)((int64_t)(r.next_u64() % (uint64_t)(2 * d + 1)) - d);                   // |dy| <= dx
    }
    float *dn, *dd, *dq;
    DRAW_HIP(cv->sc.get(11, dn, 3 * (size_t)n));
    dd = dn + n; dq = dd + n;
    DRAW_HIP(hipMemcpyAsync(dn, num.data(), n * sizeof(float), hipMemcpyHostToDevice, cv->stream));
    DRAW_HIP(hipMemcpyAsync(dd, den.data(), n * sizeof(float), hipMemcpyHostToDevice, cv->stream));
    hipLaunchKernelGGL(k_draw_divtest, dim3(n / 256), dim3(256), 0, cv->stream, (const float *)dn, (const float *)dd, dq, n);
    DRAW_HIP(hipMemcpyAsync(out.data(), dq, n * sizeof(float), hipMemcpyDeviceToHost, cv->stream));
    DRAW_HIP(hipStreamSynchronize(cv->stream));
    uint32_t bad = 0;
    for (uint32_t k = 0; k < n; ++k) {
        volatile float q = num[k] / den[k];
        const float h = q;
        bad += memcmp(&h, &out[k], 4) ? 1u : 0u;
    }
    cv->div64 = bad ? 1u : 0u;
    return PORRT_OK;
}

// The lines stand in slot 0 (n of them, with their styles in slot 1 when two colours share the call) and have been checked: run the
// call.  alpha is the call's; col its one or two colours.
static int draw_run(porrt_canvas *cv, uint32_t n, bool styled, float alpha, const DrawColors &col, double t0) {
    struct porrt_draw_info &in = cv->info;
    in = porrt_draw_info{};
    in.lines = n;
    in.gradient_by_f64 = cv->div64;
    if (!n) { in.s_total = now_s() - t0; return PORRT_OK; }
    const uint32_t P = cv->W * cv->H;
    DrawLine *lines; uint8_t *style = nullptr; unsigned long long *small; uint32_t *line_frag, *cnt, *heavy, *medium; unsigned long long *line_off, *tot, *off; uint2 *rec, *rec2;
    const size_t scan_n = std::max<size_t>(n, P) + 1;
    DRAW_HIP(cv->sc.get(0, lines, n));
    if (styled) DRAW_HIP(cv->sc.get(1, style, n));
    DRAW_HIP(cv->sc.get(2, small, 8));
    DRAW_HIP(cv->sc.get(3, line_frag, n)); DRAW_HIP(cv->sc.get(4, line_off, (size_t)n + 1)); DRAW_HIP(cv->sc.get(5, tot, (scan_n + kScanTile - 1) / kScanTile + 2));
    DRAW_HIP(cv->sc.get(6, cnt, (size_t)P + 1)); DRAW_HIP(cv->sc.get(7, off, (size_t)P + 2));
    unsigned long long *d_cut = small + 2;
    DrawStats *d_stats = (DrawStats *)(small + 4);                      // (16 bytes: small[4], small[5])
    hipStream_t st = cv->stream;
    const dim3 block(256);
    auto grid = [](size_t m) { return dim3((unsigned)((std::max<size_t>(m, 1) + 255) / 256)); };
    float ms = 0;
    // the whole call counted at once: the per-line counts cut the passes, and the pixels' counts are those of the only pass when one is enough
    DRAW_HIP(hipEventRecord(cv->ev[0], st));
    DRAW_HIP(hipMemsetAsync(cnt, 0, ((size_t)P + 1) * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_draw_count, grid(n), block, 0, st, (const DrawLine *)lines, 0u, n, cv->W, cv->H, cv->div64, cnt, line_frag);
    bg_scan(line_frag, n, tot, line_off, st);
    DRAW_HIP(hipEventRecord(cv->ev[1], st));
    unsigned long long total = 0;
    DRAW_HIP(hipMemcpyAsync(&total, line_off + n, sizeof total, hipMemcpyDeviceToHost, st));
    DRAW_HIP(hipStreamSynchronize(st));
    DRAW_HIP(hipEventElapsedTime(&ms, cv->ev[0], cv->ev[1]));
    in.s_count += 1e-3 * ms;
    in.fragments = total;
    const bool one_pass = total <= cv->max_fragments;
    uint32_t s = 0;
    size_t rec_cap = 0, heavy_n = 0, medium_n = 0;
    while (s < n) {
        uint32_t e = n;
        unsigned long long frags = total;
        if (!one_pass) {
            hipLaunchKernelGGL(k_draw_cut, dim3(1), dim3(1), 0, st, (const unsigned long long *)line_off, s, n, (unsigned long long)cv->max_fragments, d_cut);
            unsigned long long h_cut[2];
            DRAW_HIP(hipMemcpyAsync(h_cut, d_cut, sizeof h_cut, hipMemcpyDeviceToHost, st));
            DRAW_HIP(hipStreamSynchronize(st));
            e = (uint32_t)h_cut[0]; frags = h_cut[1];
        }
        ++in.passes;
        if (frags) {
            if (frags > rec_cap) {
                DRAW_HIP(cv->sc.get(8, rec, (size_t)frags)); DRAW_HIP(cv->sc.get(9, rec2, (size_t)frags));
                rec_cap = (size_t)frags;
            }
            // the lists' bounds: a listed pixel holds more than heavy_cap records, one of the workgroup form more than 64 as well
            const size_t mn = std::min<size_t>(P, (size_t)(frags / ((unsigned long long)cv->heavy_cap + 1)) + 1);
            const size_t hn = std::min<size_t>(P, (size_t)(frags / ((unsigned long long)std::max(cv->heavy_cap, kDrawWave) + 1)) + 1);
            if (hn > heavy_n) { DRAW_HIP(cv->sc.get(10, heavy, hn)); heavy_n = hn; }
            if (mn > medium_n) { DRAW_HIP(cv->sc.get(12, medium, mn)); medium_n = mn; }
            DRAW_HIP(hipEventRecord(cv->ev[0], st));
            if (!one_pass) {
                DRAW_HIP(hipMemsetAsync(cnt, 0, ((size_t)P + 1) * sizeof(uint32_t), st));
                hipLaunchKernelGGL(k_draw_count, grid(e - s), block, 0, st, (const DrawLine *)lines, s, e, cv->W, cv->H, cv->div64, cnt, (uint32_t *)nullptr);
            }
            DRAW_HIP(hipEventRecord(cv->ev[1], st));
            bg_scan(cnt, P, tot, off, st);
            DRAW_HIP(hipMemsetAsync(cnt, 0, ((size_t)P + 1) * sizeof(uint32_t), st));               // the counts have become offsets: the array is the cursors now
            DRAW_HIP(hipMemsetAsync(d_stats, 0, sizeof(DrawStats), st));
            DRAW_HIP(hipEventRecord(cv->ev[2], st));
            hipLaunchKernelGGL(k_draw_scatter, grid(e - s), block, 0, st, (const DrawLine *)lines, (const uint8_t *)style, s, e, cv->W, cv->H, cv->div64, alpha,
                               (const unsigned long long *)off, cnt, rec);
            DRAW_HIP(hipEventRecord(cv->ev[3], st));
            hipLaunchKernelGGL(k_draw_resolve_light, grid(P), block, 0, st, (const unsigned long long *)off, (const uint2 *)rec, P, cv->heavy_cap, col, cv->d_rgb, heavy,
                               medium, d_stats);
            // (no host round trip between the forms: the grids cover the lists' bounds and the kernels read the lengths)
            if (cv->heavy_cap < kDrawWave)
                hipLaunchKernelGGL(k_draw_resolve_wave, dim3((unsigned)((mn + 3) / 4)), block, 0, st, (const unsigned long long *)off, (const uint2 *)rec, (const uint32_t *)medium,
                                   (const DrawStats *)d_stats, col, cv->d_rgb);
            hipLaunchKernelGGL(k_draw_resolve_heavy, dim3((unsigned)hn), block, 0, st, (const unsigned long long *)off, rec, rec2, (const uint32_t *)heavy,
                               (const DrawStats *)d_stats, col, cv->d_rgb);
            DRAW_HIP(hipEventRecord(cv->ev[4], st));
            DrawStats hs;
            DRAW_HIP(hipMemcpyAsync(&hs, d_stats, sizeof hs, hipMemcpyDeviceToHost, st));
            DRAW_HIP(hipStreamSynchronize(st));
            DRAW_HIP(hipGetLastError());
            if (!one_pass) { DRAW_HIP(hipEventElapsedTime(&ms, cv->ev[0], cv->ev[1])); in.s_count += 1e-3 * ms; }
            DRAW_HIP(hipEventElapsedTime(&ms, cv->ev[1], cv->ev[2])); in.s_scan += 1e-3 * ms;
            DRAW_HIP(hipEventElapsedTime(&ms, cv->ev[2], cv->ev[3])); in.s_scatter += 1e-3 * ms;
            DRAW_HIP(hipEventElapsedTime(&ms, cv->ev[3], cv->ev[4])); in.s_resolve += 1e-3 * ms;
            in.heaviest_pixel = std::max<uint64_t>(in.heaviest_pixel, hs.heaviest);
            in.heavy_pixels += (uint64_t)hs.n_heavy + hs.n_wave;
            in.wave_pixels += hs.n_wave;
        }
        s = e;
    }
    in.s_total = now_s() - t0;
    return PORRT_OK;
}

// the flag the line kernels raise (slot 2, word 0): cleared before them, read after them -- before anything touches the image
static int draw_flag_clear(porrt_canvas *cv, uint32_t *&bad) {
    unsigned long long *small;
    DRAW_HIP(cv->sc.get(2, small, 8));
    bad = (uint32_t *)small;
    DRAW_HIP(hipMemsetAsync(bad, 0, sizeof(unsigned long long), cv->stream));
    return PORRT_OK;
}
static int draw_flag_check(porrt_canvas *cv, const uint32_t *bad, const char *who) {
    uint32_t h = 0;
    DRAW_HIP(hipMemcpyAsync(&h, bad, sizeof h, hipMemcpyDeviceToHost, cv->stream));
    DRAW_HIP(hipStreamSynchronize(cv->stream));
    DRAW_HIP(hipGetLastError());
    if (h & 1u) { cv->set_err(std::string(who) + ": a line with a non-finite coordinate; nothing was drawn"); return PORRT_ERR_INVALID; }
    if (h & 2u) { cv->set_err(std::string(who) + ": a line end beyond pixel 2^24; nothing was drawn"); return PORRT_ERR_INVALID; }
    return PORRT_OK;
}

// n lines given as host coordinates ab (4 per line: a, b), with their styles (0 / 1: which of the call's two colours) or null
static int draw_host_lines(porrt_canvas *cv, const char *who, const double *ab, const uint8_t *styles, uint64_t n, float alpha, const DrawColors &col) {
    const double t0 = now_s();
    if (n >= (1ull << 31)) { cv->set_err(std::string(who) + ": 2^31 lines or more in one call"); return PORRT_ERR_CAPACITY; }
    DRAW_HIP(hipSetDevice(cv->device));
    if (!n) return draw_run(cv, 0, false, alpha, col, t0);
    DrawLine *lines; double *d_ab; uint8_t *style; uint32_t *bad;
    DRAW_HIP(cv->sc.get(0, lines, (size_t)n)); DRAW_HIP(cv->sc.get(11, d_ab, 4 * (size_t)n));
    DRAW_HIP(hipMemcpyAsync(d_ab, ab, 4 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, cv->stream));
    if (styles) { DRAW_HIP(cv->sc.get(1, style, (size_t)n)); DRAW_HIP(hipMemcpyAsync(style, styles, (size_t)n, hipMemcpyHostToDevice, cv->stream)); }
    int r = draw_flag_clear(cv, bad);
    if (r) return r;
    hipLaunchKernelGGL(k_draw_lines_host, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cv->stream, (const double *)d_ab, (uint32_t)n, cv->geom(), lines, bad);
    if ((r = draw_flag_check(cv, bad, who))) return r;
    return draw_run(cv, (uint32_t)n, styles != nullptr, alpha, col, t0);
}

static DrawColors draw_colors(const uint8_t a[3], const uint8_t b[3]) {
    DrawColors c;
    for (int k = 0; k < 3; ++k) { c.rgb[0][k] = a[k]; c.rgb[1][k] = b[k]; }
    return c;
}

// draw_circle (map_shelves_io.rs:377-387): 50 segments between xy + r * (cos, sin)(k * 2 pi / 50), the host's libm
static void draw_circle_lines(const double xy[2], double radius, std::vector<double> &ab) {
    double pt[51][2];
    for (int k = 0; k <= 50; ++k) {
        const double angle = (double)k * 2.0 * 3.14159265358979323846 / 50.0;
        pt[k][0] = xy[0] + radius * std::cos(angle); pt[k][1] = xy[1] + radius * std::sin(angle);
    }
    for (int k = 1; k <= 50; ++k) { ab.push_back(pt[k - 1][0]); ab.push_back(pt[k - 1][1]); ab.push_back(pt[k][0]); ab.push_back(pt[k][1]); }
}

static bool draw_same_geometry(const porrt_canvas *cv, const porrt_ctx *c) {
    return c->has_grid && c->device == cv->device && c->W == cv->W0 && c->H == cv->H0 && c->low[0] == cv->low[0] && c->low[1] == cv->low[1] && c->ppm == cv->ppm0 &&
           c->domain == cv->domain;
}

static const uint8_t kDrawTeal[3] = {0, 128, 128}, kDrawNavy[3] = {0, 0, 128}, kDrawBlack[3] = {0, 0, 0}, kDrawGray5[3] = {150, 150, 150};

} // namespace porrt

extern "C" {

porrt_canvas *porrt_canvas_create(const porrt_ctx *cc, uint32_t factor) {
    porrt_ctx *c = const_cast<porrt_ctx *>(cc);
    if (!c) return nullptr;
    porrt_canvas *cv = nullptr;
    // (a failed creation has no canvas to ask: the code goes to the context, porrt_get_option "draw_create_status", the text to porrt_last_error)
    auto fail = [&](int code, const char *msg) -> porrt_canvas * { porrt_canvas_destroy(cv); c->set_err(msg); c->draw_create_status = code; return nullptr; };
    if (!c->has_grid) return fail(PORRT_ERR_INVALID, "porrt_canvas_create: set the grid first (porrt_set_grid)");
    if (!factor) return fail(PORRT_ERR_INVALID, "porrt_canvas_create: factor 0");
    if ((uint64_t)c->W * factor > kDrawMaxSide || (uint64_t)c->H * factor > kDrawMaxSide) return fail(PORRT_ERR_CAPACITY, "porrt_canvas_create: more than 16384 pixels a side");
    try { cv = new porrt_canvas(); } catch (...) { return fail(PORRT_ERR_NOMEM, "porrt_canvas_create: out of memory"); }
    auto fail_dev = [&](const char *msg) -> porrt_canvas * { return fail(PORRT_ERR_DEVICE, msg); };
    cv->device = c->device;
    cv->W0 = c->W; cv->H0 = c->H; cv->factor = factor; cv->W = c->W * factor; cv->H = c->H * factor;
    cv->low[0] = c->low[0]; cv->low[1] = c->low[1]; cv->ppm0 = c->ppm;
    cv->ppm = c->ppm;
    if (factor != 1) cv->ppm *= (double)factor;                  // self.ppm *= factor as f64
    cv->domain = c->domain;
    cv->n_zones = c->n_zones; cv->visibility = c->visibility;
    memcpy(cv->zone_pos, c->zone_pos, sizeof cv->zone_pos);
    cv->max_fragments = c->opt_draw_max_fragments; cv->heavy_cap = c->opt_draw_heavy_cap;
    if (hipSetDevice(cv->device) != hipSuccess || hipStreamCreateWithFlags(&cv->stream, hipStreamNonBlocking) != hipSuccess) { cv->stream = nullptr; return fail_dev("porrt_canvas_create: stream"); }
    for (hipEvent_t &e : cv->ev) if (hipEventCreate(&e) != hipSuccess) { e = nullptr; return fail_dev("porrt_canvas_create: events"); }
    const size_t P = (size_t)cv->W * cv->H;
    uint8_t *d_occ = nullptr;
    if (hipMalloc((void **)&cv->d_rgb, 3 * P) != hipSuccess) { cv->d_rgb = nullptr; return fail(PORRT_ERR_CAPACITY, "porrt_canvas_create: no device memory for the image"); }
    if (cv->sc.get(11, d_occ, c->occ.size()) != hipSuccess || hipMemcpyAsync(d_occ, c->occ.data(), c->occ.size(), hipMemcpyHostToDevice, cv->stream) != hipSuccess)
        return fail_dev("porrt_canvas_create: raster upload");
    hipLaunchKernelGGL(k_draw_canvas, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, cv->stream, (const uint8_t *)d_occ, cv->W0, factor, cv->W, cv->H, cv->d_rgb);
    if (hipStreamSynchronize(cv->stream) != hipSuccess || hipGetLastError() != hipSuccess) return fail_dev("porrt_canvas_create: k_draw_canvas");
    if (draw_div_sweep(cv) != PORRT_OK) return fail_dev("porrt_canvas_create: the f32 divide sweep");
    c->draw_create_status = PORRT_OK;
    return cv;
}

void porrt_canvas_destroy(porrt_canvas *cv) {
    if (!cv) return;
    (void)hipSetDevice(cv->device);
    if (cv->stream) (void)hipStreamSynchronize(cv->stream);
    for (hipEvent_t e : cv->ev) if (e) (void)hipEventDestroy(e);
    if (cv->d_rgb) (void)hipFree(cv->d_rgb);
    cv->sc.free_all();
    if (cv->stream) (void)hipStreamDestroy(cv->stream);
    delete cv;
}

const char *porrt_canvas_last_error(const porrt_canvas *cv) { return cv ? cv->err.c_str() : "null canvas"; }

int porrt_canvas_size(const porrt_canvas *cv, uint32_t *W, uint32_t *H) {
    if (!cv) return PORRT_ERR_INVALID;
    if (W) *W = cv->W;
    if (H) *H = cv->H;
    return PORRT_OK;
}

int porrt_canvas_draw_lines(porrt_canvas *cv, const double *ab, uint64_t n, const uint8_t rgb[3], float alpha) {
    if (!cv || !rgb || (n && !ab)) return PORRT_ERR_INVALID;
    return abi_guard([&]() -> int { return draw_host_lines(cv, "porrt_canvas_draw_lines", ab, nullptr, n, alpha, draw_colors(rgb, rgb)); });
}

int porrt_canvas_draw_path(porrt_canvas *cv, const double *xy, uint64_t n, const uint8_t rgb[3]) {
    if (!cv || !rgb || (n && !xy)) return PORRT_ERR_INVALID;
    return abi_guard([&]() -> int {
        std::vector<double> ab;
        for (uint64_t i = 1; i < n; ++i) { ab.push_back(xy[2 * i - 2]); ab.push_back(xy[2 * i - 1]); ab.push_back(xy[2 * i]); ab.push_back(xy[2 * i + 1]); }
        return draw_host_lines(cv, "porrt_canvas_draw_path", ab.data(), nullptr, ab.size() / 4, 1.0f, draw_colors(rgb, rgb));
    });
}

int porrt_canvas_draw_circles(porrt_canvas *cv, const double *xy, uint64_t n, double radius, const uint8_t rgb[3]) {
    if (!cv || !rgb || (n && !xy)) return PORRT_ERR_INVALID;
    return abi_guard([&]() -> int {
        std::vector<double> ab;
        for (uint64_t i = 0; i < n; ++i) draw_circle_lines(xy + 2 * i, radius, ab);
        return draw_host_lines(cv, "porrt_canvas_draw_circles", ab.data(), nullptr, ab.size() / 4, 1.0f, draw_colors(rgb, rgb));
    });
}

int porrt_canvas_draw_zones_observability(porrt_canvas *cv) {
    if (!cv) return PORRT_ERR_INVALID;
    return abi_guard([&]() -> int {
        std::vector<double> ab;
        for (int z = 0; z < cv->n_zones; ++z) draw_circle_lines(cv->zone_pos[z], cv->visibility, ab);
        return draw_host_lines(cv, "porrt_canvas_draw_zones_observability", ab.data(), nullptr, ab.size() / 4, 1.0f, draw_colors(kDrawTeal, kDrawTeal));
    });
}

int porrt_canvas_draw_policy(porrt_canvas *cv, const double *xy, const int64_t *parent, uint64_t n) {
    if (!cv || (n && (!xy || !parent))) return PORRT_ERR_INVALID;
    return abi_guard([&]() -> int {
        // children in ascending policy id: extract_policy and recompose number a node's children as they add them
        std::vector<uint64_t> off(n + 2, 0), ids(n);
        for (uint64_t k = 0; k < n; ++k) {
            if (parent[k] >= (int64_t)n || parent[k] < -1) { cv->set_err("porrt_canvas_draw_policy: a parent out of range"); return PORRT_ERR_INVALID; }
            if (parent[k] >= 0) ++off[(uint64_t)parent[k] + 2];
        }
        for (uint64_t k = 0; k < n; ++k) off[k + 2] += off[k + 1];
        for (uint64_t k = 0; k < n; ++k) if (parent[k] >= 0) ids[off[(uint64_t)parent[k] + 1]++] = k;
        std::vector<double> ab;
        std::vector<uint8_t> styles;
        for (uint64_t p = 0; p < n; ++p) {
            const uint64_t a = off[p], b = off[p + 1];
            if (b - a > 1) { draw_circle_lines(xy + 2 * p, 0.025, ab); styles.resize(ab.size() / 4, 0); }
            for (uint64_t q = a; q < b; ++q) { ab.push_back(xy[2 * p]); ab.push_back(xy[2 * p + 1]); ab.push_back(xy[2 * ids[q]]); ab.push_back(xy[2 * ids[q] + 1]); }
            styles.resize(ab.size() / 4, 1);
        }
        return draw_host_lines(cv, "porrt_canvas_draw_policy", ab.data(), styles.data(), ab.size() / 4, 1.0f, draw_colors(kDrawNavy, kDrawBlack));
    });
}

int porrt_canvas_draw_tree(porrt_canvas *cv, const porrt_ctx *c) {
    if (!cv || !c) return PORRT_ERR_INVALID;
    return abi_guard([&]() -> int {
        const double t0 = now_s();
        if (!draw_same_geometry(cv, c)) { cv->set_err("porrt_canvas_draw_tree: the context is on another device or has another raster geometry"); return PORRT_ERR_INVALID; }
        if (!c->have_results || c->mm.valid || c->mode != PORRT_MODE_RRT) { cv->set_err("porrt_canvas_draw_tree: the context holds no tree (porrt_grow, mode PORRT_MODE_RRT)"); return PORRT_ERR_INVALID; }
        DRAW_HIP(hipSetDevice(cv->device));
        DRAW_HIP(hipStreamSynchronize(c->stream));
        const uint32_t n = (uint32_t)c->n_nodes;
        DrawLine *lines; uint32_t *bad;
        DRAW_HIP(cv->sc.get(0, lines, n));
        int r = draw_flag_clear(cv, bad);
        if (r) return r;
        hipLaunchKernelGGL(k_draw_lines_tree, dim3((n + 255) / 256), dim3(256), 0, cv->stream, (const double *)c->d_nx.p, (const double *)c->d_ny.p, (const int *)c->d_parent.p, n,
                           cv->geom(), lines, bad);
        if ((r = draw_flag_check(cv, bad, "porrt_canvas_draw_tree"))) return r;
        return draw_run(cv, n, false, 0.3f, draw_colors(kDrawTeal, kDrawTeal), t0);
    });
}

int porrt_canvas_draw_full_graph(porrt_canvas *cv, const porrt_ctx *cc) {
    porrt_ctx *c = const_cast<porrt_ctx *>(cc);
    if (!cv || !c) return PORRT_ERR_INVALID;
    return abi_guard([&]() -> int {
        const double t0 = now_s();
        if (!draw_same_geometry(cv, c)) { cv->set_err("porrt_canvas_draw_full_graph: the context is on another device or has another raster geometry"); return PORRT_ERR_INVALID; }
        if (!c->have_results || c->mm.valid || (c->mode != PORRT_MODE_PTO && c->mode != PORRT_MODE_PRM)) {
            cv->set_err("porrt_canvas_draw_full_graph: the context holds no PTO graph or PRM roadmap");
            return PORRT_ERR_INVALID;
        }
        // the lists porrt_graph_save_json writes and the belief-graph build reads; when the context has not made them yet they are made here
        // with the kd pre-order ranks built on the device (k_kd1_*), so that no node or edge array goes to the host for a picture
        int r = c->ensure_edge_order(/*ranks_on_device=*/true);
        if (r) { cv->set_err("porrt_canvas_draw_full_graph: " + c->err); return r; }
        const uint64_t n64 = 2 * (uint64_t)c->eo.E;              // both directions: every edge stands in two lists
        if (n64 >= (1ull << 31)) { cv->set_err("porrt_canvas_draw_full_graph: 2^31 lines or more in one call"); return PORRT_ERR_CAPACITY; }
        DRAW_HIP(hipSetDevice(cv->device));
        const uint32_t n = (uint32_t)n64;
        DrawLine *lines; uint32_t *bad;
        DRAW_HIP(cv->sc.get(0, lines, n));
        if ((r = draw_flag_clear(cv, bad))) return r;
        if (n) hipLaunchKernelGGL(k_draw_lines_graph, dim3((n + 255) / 256), dim3(256), 0, cv->stream, (const double *)c->d_nx.p, (const double *)c->d_ny.p,
                                  (const unsigned long long *)c->eo.d_adj_off, (const uint32_t *)c->eo.d_adj_id, (uint32_t)c->eo.N, n, cv->geom(), lines, bad);
        if ((r = draw_flag_check(cv, bad, "porrt_canvas_draw_full_graph"))) return r;
        return draw_run(cv, n, false, cv->domain == PORRT_DOMAIN_DOOR ? 0.15f : 0.25f, draw_colors(kDrawGray5, kDrawGray5), t0);
    });
}

int porrt_canvas_get_rgb(const porrt_canvas *cv, uint8_t *rgb) {
    if (!cv || !rgb) return PORRT_ERR_INVALID;
    if (hipSetDevice(cv->device) != hipSuccess || hipStreamSynchronize(cv->stream) != hipSuccess ||
        hipMemcpy(rgb, cv->d_rgb, 3 * (size_t)cv->W * cv->H, hipMemcpyDeviceToHost) != hipSuccess)
        return PORRT_ERR_DEVICE;
    return PORRT_OK;
}

int porrt_canvas_save_png(const porrt_canvas *cv, const char *path) {
    if (!cv || !path) return PORRT_ERR_INVALID;
    return abi_guard([&]() -> int {
        std::vector<uint8_t> px(3 * (size_t)cv->W * cv->H);
        const int r = porrt_canvas_get_rgb(cv, px.data());
        return r ? r : porrt_write_png(path, px.data(), cv->W, cv->H);
    });
}

int porrt_canvas_get_info(const porrt_canvas *cv, struct porrt_draw_info *out) {
    if (!cv || !out) return PORRT_ERR_INVALID;
    *out = cv->info;
    return PORRT_OK;
}

} // extern "C"
