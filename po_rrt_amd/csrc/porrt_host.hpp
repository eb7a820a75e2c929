// porrt_host.hpp -- host utilities the engine and the subsystem headers share: the HIP error checks, the clock, the reference's
// random number generator and the two owners of device memory that outlive or accompany a call.
#pragma once
#include "../../include/porrt_hip.h"
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

typedef unsigned __int128 u128;

#define HIPCHK_CTX(ctx, expr)                                                                      \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            (ctx)->set_err(std::string(#expr) + ": " + hipGetErrorString(e_));                     \
            return PORRT_ERR_DEVICE;                                                               \
        }                                                                                          \
    } while (0)

#define HIPCHK(expr) HIPCHK_CTX(this, expr)         // in a method of the context
// in a free function that reports through a string `err`
#define HIPCHK_ERR(expr)                                                                           \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) { err = std::string(#expr) + ": " + hipGetErrorString(e_); return PORRT_ERR_DEVICE; } \
    } while (0)

namespace {

double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- rand_pcg 0.3 Pcg64 (Lcg128Xsl64) + rand_core 0.6 seed_from_u64 + rand 0.8 gen_range on the host.
// The device generates the continuous stream (k_gen_samples); the host keeps the authoritative state,
// draws the rejection-sampled world indices and is the exact fallback when a float draw would retry.
const u128 PCG_MULT = (((u128)0x2360ED051FC65DA4ULL) << 64) | (u128)0x4385DF649FCCF645ULL;
struct Pcg64 {
    u128 state, inc;
    void from_state_incr(u128 s, u128 i) {
        state = s; inc = i;
        state += inc;
        step();
    }
    void step() { state = state * PCG_MULT + inc; }
    void seed_from_u64(uint64_t s) {
        const uint64_t MUL = 6364136223846793005ULL, INC = 11634580027462260723ULL;
        uint32_t w[8];
        for (int c = 0; c < 8; ++c) {
            s = s * MUL + INC;
            uint32_t xs = (uint32_t)(((s >> 18) ^ s) >> 27), rot = (uint32_t)(s >> 59);
            w[c] = (xs >> rot) | (xs << ((32 - rot) & 31));
        }
        uint64_t q[4];
        for (int i = 0; i < 4; ++i) q[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
        from_state_incr((u128)q[0] | ((u128)q[1] << 64), ((u128)q[2] | ((u128)q[3] << 64)) | 1);
    }
    uint64_t next_u64() {
        step();
        uint32_t rot = (uint32_t)(state >> 122);
        uint64_t xsl = (uint64_t)(state >> 64) ^ (uint64_t)state;
        return (xsl >> rot) | (xsl << ((64 - rot) & 63));
    }
    void advance(u128 delta) {
        u128 am = 1, ap = 0, cm = PCG_MULT, cp = inc;
        while (delta > 0) {
            if (delta & 1) { am *= cm; ap = ap * cm + cp; }
            cp = (cm + 1) * cp;
            cm *= cm;
            delta >>= 1;
        }
        state = am * state + ap;
    }
    double gen_range_f64(double low, double high) {
        double scale = high - low;
        for (;;) {
            uint64_t bits = (next_u64() >> 12) | 0x3FF0000000000000ULL;
            double v12;
            memcpy(&v12, &bits, 8);
            volatile double prod = (v12 - 1.0) * scale;
            double res = prod + low;
            if (res < high) return res;
        }
    }
    uint64_t gen_range_usize(uint64_t n) {
        if (n == 0) return next_u64();
        uint64_t zone = (n << __builtin_clzll(n)) - 1;
        for (;;) {
            u128 m = (u128)next_u64() * (u128)n;
            if ((uint64_t)m <= zone) return (uint64_t)(m >> 64);
        }
    }
};

uint64_t ones(int n) { return n >= 64 ? ~0ULL : ((1ULL << n) - 1); }

} // namespace

// Device scratch that outlives a call: numbered slots that only grow (a caller that builds roadmaps again and again pays for its
// buffers once: a dozen hipMalloc / hipFree pairs cost more than the kernels they serve).
struct GrowScratch {
    std::vector<std::pair<void *, size_t>> slots;
    template <class T> hipError_t get(size_t slot, T *&p, size_t n) {
        if (slots.size() <= slot) slots.resize(slot + 1, {nullptr, 0});
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        if (slots[slot].second < bytes) {
            if (slots[slot].first) (void)hipFree(slots[slot].first);
            slots[slot] = {nullptr, 0};
            void *q = nullptr;
            const hipError_t e = hipMalloc(&q, bytes + bytes / 8);
            if (e != hipSuccess) return e;
            slots[slot] = {q, bytes + bytes / 8};
        }
        p = (T *)slots[slot].first;
        return hipSuccess;
    }
    void free_all() { for (auto &sl : slots) if (sl.first) (void)hipFree(sl.first); slots.clear(); }
    GrowScratch() = default;
    GrowScratch(const GrowScratch &) = delete;
    GrowScratch &operator=(const GrowScratch &) = delete;
    ~GrowScratch() { free_all(); }                                   // (a context frees its slots in porrt_destroy, with its device current)
};

// The device copies of one call's host arrays (the entry points that take an explicit graph): up() allocates n elements (at least
// 8 bytes), fills them from src when there is one, and returns nullptr on a device error; the destructor frees every buffer,
// whichever way the call ends.
struct DeviceUploads {
    std::vector<void *> owned;
    template <class T> T *up(const void *src, size_t n) {
        void *d = nullptr;
        if (hipMalloc(&d, std::max<size_t>(n * sizeof(T), 8)) != hipSuccess) return nullptr;
        owned.push_back(d);
        if (n && src && hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return (T *)d;
    }
    DeviceUploads() { owned.reserve(16); }                          // (more than any caller uploads: recording a buffer does not allocate)
    DeviceUploads(const DeviceUploads &) = delete;
    DeviceUploads &operator=(const DeviceUploads &) = delete;
    ~DeviceUploads() { for (void *d : owned) (void)hipFree(d); }
};
