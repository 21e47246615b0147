// bandits_core.h — the bandits family's shared core: the stream view of a wave (Streams), the task draw (sample_task),
// BanditsK and the host checks. bandits.hip, bandits_policy.hip and bandits_learner.hip include it; each keeps its own
// copy (anonymous namespace) and defines the kernels it launches. The streams and the mapping are described in bandits.hip.
#pragma once
#include <cmath>

#include "mg_common.h"
#include "mg_mt19937.h"

namespace {

using mt::MTN;
constexpr int REC = MTN + 1;   // u32 words per stream record: key, pos

struct BanditsK {
    int K, max_steps, auto_reset, dist;
    double mean, dev, lo, hi;
    uint32_t rng_idx, mask_idx;   // bounded(K-2)
};

// numpy's clip for doubles: min(max(x, 0), 1), NaN passing through
__device__ __forceinline__ double clip01(double x) {
    if (isnan(x)) return x;
    const double y = x > 0.0 ? x : 0.0;
    return y < 1.0 ? y : 1.0;
}

// One wave's view of its 64 streams; every member function is called by all lanes together (refills are collective).
struct Streams {
    uint32_t *mt;     // all records
    uint32_t *lds;    // [624] refill scratch
    int e0, lane, n;  // first env of the wave, this lane, number of envs
    int pos;          // this lane's read position (624: refill before the next draw)

    __device__ __forceinline__ uint32_t *key() const { return mt + (size_t)(e0 + lane) * REC; }

    __device__ void refill_lanes(uint64_t bal) {
        while (bal) {
            const int j = __builtin_ctzll(bal);
            bal &= bal - 1;
            uint32_t *k = mt + (size_t)(e0 + j) * REC;
            for (int i = lane; i < MTN; i += 64) lds[i] = k[i];
            __syncthreads();
            mt::refill(lds, lane);
            for (int i = lane; i < MTN; i += 64) k[i] = lds[i];
            __threadfence_block();   // the block is read back by lane j through the same CU's cache
            __syncthreads();
        }
    }

    // one tempered word for the lanes with `act`; 0 elsewhere
    __device__ __forceinline__ uint32_t next(bool act) {
        const uint64_t bal = __ballot(act && pos >= MTN);
        if (bal) {
            refill_lanes(bal);
            if (act && pos >= MTN) pos = 0;
        }
        uint32_t w = 0;
        if (act) w = mt::temper(key()[pos++]);
        return w;
    }

    __device__ __forceinline__ double next_double(bool act) {
        const uint32_t a = next(act);
        return mt::to_double(a, next(act));
    }

    // randint's masked rejection on [0, rng]
    __device__ uint32_t bounded(bool act, uint32_t rng, uint32_t mask) {
        if (rng == 0) return 0;   // consumes nothing
        bool pending = act;
        uint32_t r = 0;
        while (__ballot(pending)) {
            const uint32_t d = next(pending) & mask;
            if (pending && d <= rng) { r = d; pending = false; }
        }
        return r;
    }
};

// Bandits.sample_task for the lanes with `act`, into row[0..K)
__device__ void sample_task(const BanditsK &k, Streams &g, bool act, int &has_gauss, double &gauss, double *row) {
    if (k.dist == MG_BANDITS_CLASSICAL) {
        const int idx = (int)g.bounded(act, k.rng_idx, k.mask_idx);
        if (act)
            for (int i = 0; i < k.K; ++i) row[i] = i == idx ? k.hi : k.lo;
    } else if (k.dist == MG_BANDITS_UNIFORM) {
        for (int i = 0; i < k.K; ++i) {
            const double d = g.next_double(act);
            if (act) row[i] = clip01((d - 0.5) * 3.464 + k.mean);
        }
    } else if (k.dist == MG_BANDITS_GAUSSIAN) {
        for (int i = 0; i < k.K; ++i) {
            double v = 0.0;
            bool pending = act && !has_gauss;
            if (act && has_gauss) {           // legacy_gauss: the cached value, then the cache is cleared
                v = gauss;
                has_gauss = 0;
                gauss = 0.0;
            }
            while (__ballot(pending)) {
                const double x1 = 2.0 * g.next_double(pending) - 1.0;
                const double x2 = 2.0 * g.next_double(pending) - 1.0;
                const double r2 = x1 * x1 + x2 * x2;
                if (pending && r2 < 1.0 && r2 != 0.0) {
                    const double f = sqrt(-2.0 * log(r2) / r2);
                    gauss = f * x1;
                    has_gauss = 1;
                    v = f * x2;
                    pending = false;
                }
            }
            if (act) row[i] = clip01(k.mean + k.dev * v);
        }
    }
}

int check_config(const mg_bandits_config *c, const char *fn) {
    // the reference's assert (bandits_env.py:32): K > 1 and max_steps > 1
    if (!(c->arms > 1)) return mg::set_error(MG_ERR_BAD_CONFIG, "%s: arms = %d (need arms > 1)", fn, c->arms);
    if (!(c->max_steps > 1))
        return mg::set_error(MG_ERR_BAD_CONFIG, "%s: max_steps = %d (need max_steps > 1)", fn, c->max_steps);
    if (c->distribution < MG_BANDITS_NONE || c->distribution > MG_BANDITS_GAUSSIAN)
        return mg::set_error(MG_ERR_BAD_CONFIG, "%s: distribution = %d (need 0..3)", fn, c->distribution);
    return MG_OK;
}

BanditsK fold(const mg_bandits_config *c) {
    BanditsK k{};
    k.K = c->arms; k.max_steps = c->max_steps; k.auto_reset = c->auto_reset != 0; k.dist = c->distribution;
    k.mean = c->mean; k.dev = c->dev; k.lo = c->classical_lo; k.hi = c->classical_hi;
    k.rng_idx = (uint32_t)(c->arms - 2); k.mask_idx = mt::bound_mask(k.rng_idx);
    return k;
}

}  // namespace

#define MG_REQUIRE_STATE(s)                                                                                   \
    do {                                                                                                      \
        MG_REQUIRE_PTR(s);                                                                                    \
        MG_REQUIRE_PTR((s)->mt); MG_REQUIRE_PTR((s)->has_gauss); MG_REQUIRE_PTR((s)->gauss);                  \
        MG_REQUIRE_PTR((s)->gains); MG_REQUIRE_PTR((s)->steps); MG_REQUIRE_PTR((s)->over);                    \
    } while (0)
