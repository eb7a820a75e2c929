// porrt_pcg64.hpp -- the reference's random number generator on the host.  Plain C++, no HIP: the host-only search headers
// (porrt_bnb_search.hpp) draw from it in programs the host compiler builds alone.
#pragma once

#include <cstdint>
#include <cstring>

typedef unsigned __int128 u128;

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
