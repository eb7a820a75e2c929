// porrt_host.hpp -- host utilities the engine and the subsystem headers share: the HIP error checks, the clock, the reference's
// random number generator (porrt_pcg64.hpp) and the two owners of device memory that outlive or accompany a call.
#pragma once
#include "../../include/porrt_hip.h"
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "porrt_pcg64.hpp"

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
