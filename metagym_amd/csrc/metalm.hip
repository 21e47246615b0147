// metalm.hip — MetaLM sequence batches (reference metagym/metalm/metalm.py) generated on the device, bit for bit.
//
// A row is what MetaLM(V, n, l, e, L).data_generator() returns. Every draw comes from numpy's legacy MT19937 stream
// (RandomState): masked-rejection randint on 32-bit draws, the 53-bit double (a >> 5, b >> 6), the legacy Poisson
// (PTRS for l >= 10, multiplication below). The accounting, draw by draw (tests/metalm_oracle.py draw_level_row):
//   elements  n times: l_r = max(3, poisson(l)), then l_r tokens 1 + bounded(V-2)
//   chunks    while cur < L+1: idx = bounded(n-2) (randint(0, n-1): the last element is never chosen); for the chosen
//             element of length m: m noise values 1 + bounded(V-2), then m doubles < e (noise), then m doubles
//             < mask_ratio (mask); feature = noise ? value : token, 0 where noise and mask; label = token; then the
//             separator V+1 in both streams, cur += m+1. The last chunk is drawn in full.
//   output    features = stream[0, L), labels = stream[1, L+1).
//
// Mapping: one wave (one workgroup of 64) per row; the generator key, the element table and a chunk scratch sit in LDS.
// The draw-heavy parts are lane-parallel over the generator's 624-word block:
//   refill      the 624 new words in three segments that are each independent inside themselves: [0,227) reads old
//               words only, [227,454) reads the new words i-227 of the first segment, [454,624) those of the second
//               and (word 623) the new word 0.
//   tempering   on the read: every word is tempered by the lane that consumes it (no second buffer of outputs).
//   bounded     64 draws per step, acceptance per lane, ballot + mbcnt place the accepted values in their output slots;
//               the read position advances only to the draw that completes the quota.
//   doubles     lane j reads draws 2j, 2j+1; a pair that straddles a refill is drawn on its own.
// The choice of the chunk's element and the Poisson loop are short and run wave-uniformly. Every batch of draws stops
// at the end of the 624-word block (`take`, `avail` below): a refill never happens inside one.
//
// Two launches of the same row program: seeded (row t from init_genrand(seeds[t] or seed_base + t), a grid of rows) and
// chained (one wave, rows 0..B-1 from the caller's stream in order, the final stream written back).
#include <climits>
#include <cmath>

#include "mg_common.h"
#include "mg_mt19937.h"

namespace {

using mt::MTN;
using mt::refill;
using mt::temper;
constexpr size_t LDS_LIMIT = 160 * 1024;               // gfx950: LDS per CU, the most one workgroup can have

struct MetaLMK {
    int V, n, L, cap;
    uint32_t rng_tok, mask_tok;   // bounded(V-2)
    uint32_t rng_idx, mask_idx;   // bounded(n-2)
    double lam, e, mask_ratio;
    int ptrs;                     // l >= 10
    // host-computed (glibc, like numpy) Poisson constants
    double loglam, b, a, log_invalpha, vr, enlam;
    uint32_t seed_base;
};

struct Stream {
    uint32_t *key;   // LDS [624]
    int pos;         // wave-uniform; 624 = refill before the next draw
    int lane;

    // one draw, the same for every lane
    __device__ __forceinline__ uint32_t next() {
        if (pos >= MTN) { refill(key, lane); pos = 0; }
        return temper(key[pos++]);
    }
    __device__ __forceinline__ double next_double() {
        const uint32_t a = next();
        return mt::to_double(a, next());
    }
    __device__ __forceinline__ uint32_t bounded(uint32_t rng, uint32_t mask) {
        if (rng == 0) return 0;                   // consumes nothing
        uint32_t d = next() & mask;
        while (d > rng) d = next() & mask;
        return d;
    }

    // dst[0..count) = 1 + bounded(rng) each, in stream order. Caller: barrier before other lanes read dst.
    __device__ void bulk_tokens(int count, uint32_t rng, uint32_t mask, int32_t *dst) {
        if (rng == 0) {
            for (int k = lane; k < count; k += 64) dst[k] = 1;
            return;
        }
        int done = 0;
        while (done < count) {
            if (pos >= MTN) { refill(key, lane); pos = 0; }
            const int take = min(64, MTN - pos);                     // never past the end of the block
            const uint32_t d = temper(key[pos + min(lane, take - 1)]) & mask;
            const bool acc = lane < take && d <= rng;
            const uint64_t bal = __ballot(acc);
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            const int need = count - done, total = __popcll(bal);
            int used = take;
            if (total >= need) {                                     // the quota fills inside this batch: stop after
                const uint64_t last = __ballot(acc && rank == need - 1);   // the draw that fills it (rejected draws
                used = __builtin_ctzll(last) + 1;                          // behind it belong to the next sampler)
            }
            if (acc && rank < need) dst[done + rank] = (int32_t)(1u + d);
            done += min(total, need);
            pos += used;
        }
    }

    // up to min(want, 64) doubles; lane j < return value holds double j in `d`
    __device__ __forceinline__ int doubles(int want, double &d) {
        if (pos >= MTN) { refill(key, lane); pos = 0; }
        const int avail = MTN - pos;
        if (avail == 1) {                                            // the pair straddles the refill
            const uint32_t a = temper(key[MTN - 1]);
            refill(key, lane);
            const uint32_t b = temper(key[0]);
            pos = 1;
            d = mt::to_double(a, b);
            return 1;
        }
        const int cnt = min(want, min(64, avail >> 1));
        const int j = pos + 2 * min(lane, cnt - 1);
        d = mt::to_double(temper(key[j]), temper(key[j + 1]));
        pos += 2 * cnt;
        return cnt;
    }
};

// numpy's random_loggam
__device__ double loggam(double x) {
    const double a[10] = {8.333333333333333e-02, -2.777777777777778e-03, 7.936507936507937e-04, -5.952380952380952e-04,
                          8.417508417508418e-04, -1.917526917526918e-03, 6.410256410256410e-03, -2.955065359477124e-02,
                          1.796443723688307e-01, -1.39243221690590e+00};
    if (x == 1.0 || x == 2.0) return 0.0;
    const int64_t n = x < 7.0 ? (int64_t)(7 - x) : 0;
    double x0 = x + (double)n;
    const double x2 = (1.0 / x0) * (1.0 / x0);
    double gl0 = a[9];
    for (int k = 8; k >= 0; --k) {
        gl0 *= x2;
        gl0 += a[k];
    }
    double gl = gl0 / x0 + 0.5 * 1.8378770664093453e+00 + (x0 - 0.5) * log(x0) - x0;
    for (int64_t k = 1; k <= n; ++k) {
        gl -= log(x0 - 1.0);
        x0 -= 1.0;
    }
    return gl;
}

// numpy's legacy poisson: random_poisson_ptrs (l >= 10) / random_poisson_mult
__device__ int64_t poisson(Stream &g, const MetaLMK &k) {
    if (k.ptrs) {
        for (;;) {
            const double U = g.next_double() - 0.5;
            const double V = g.next_double();
            const double us = 0.5 - fabs(U);
            const int64_t x = (int64_t)floor((2 * k.a / us + k.b) * U + k.lam + 0.43);
            if (us >= 0.07 && V <= k.vr) return x;
            if (x < 0 || (us < 0.013 && V > us)) continue;
            if (log(V) + k.log_invalpha - log(k.a / (us * us) + k.b) <= -k.lam + (double)x * k.loglam - loggam((double)(x + 1)))
                return x;
        }
    }
    int64_t x = 0;
    double prod = 1.0;
    for (;;) {
        prod *= g.next_double();
        if (prod > k.enlam) ++x;
        else return x;
    }
}

// One row. Returns false (nothing more drawn, nothing written) when the elements need more than k.cap tokens.
__device__ bool metalm_row(const MetaLMK &k, Stream &g, int32_t *len, int32_t *off, int32_t *tok, int32_t *scratch,
                           int32_t *feat, int32_t *lab) {
    const int lane = g.lane;
    int total = 0;
    for (int i = 0; i < k.n; ++i) {
        int64_t m = poisson(g, k);
        m = m < 3 ? 3 : m;
        if (m > (int64_t)(k.cap - total)) return false;
        if (lane == 0) { len[i] = (int32_t)m; off[i] = total; }
        g.bulk_tokens((int)m, k.rng_tok, k.mask_tok, tok + total);
        total += (int)m;
    }
    __syncthreads();
    const int L = k.L;
    for (int cur = 0; cur < L + 1;) {
        const int idx = (int)g.bounded(k.rng_idx, k.mask_idx);
        const int m = len[idx];
        const int32_t *seq = tok + off[idx];
        g.bulk_tokens(m, k.rng_tok, k.mask_tok, scratch);                  // noise values
        __syncthreads();
        for (int k0 = 0; k0 < m;) {                                         // noise flags: value | bit 31, or the token
            double d;
            const int c = g.doubles(m - k0, d);
            const int q = k0 + lane;
            if (lane < c) scratch[q] = d < k.e ? (int32_t)((uint32_t)scratch[q] | 0x80000000u) : seq[q];
            k0 += c;
        }
        __syncthreads();
        for (int k0 = 0; k0 < m;) {                                         // mask flags, then the output
            double d;
            const int c = g.doubles(m - k0, d);
            const int q = k0 + lane;
            if (lane < c) {
                const int32_t s = scratch[q];
                const int32_t f = (s < 0 && d < k.mask_ratio) ? 0 : (s & 0x7fffffff);
                const int p = cur + q;
                if (p < L) feat[p] = f;
                if (p >= 1 && p <= L) lab[p - 1] = seq[q];
            }
            k0 += c;
        }
        if (lane == 0) {                                                    // separator
            const int p = cur + m;
            if (p < L) feat[p] = k.V + 1;
            if (p <= L) lab[p - 1] = k.V + 1;
        }
        cur += m + 1;
        __syncthreads();                                                    // scratch is rewritten by the next chunk
    }
    return true;
}

struct Lds {
    uint32_t *key;
    int32_t *len, *off, *tok, *scratch;
};

__device__ __forceinline__ Lds carve(unsigned char *smem, const MetaLMK &k) {
    Lds s;
    s.key = reinterpret_cast<uint32_t *>(smem);
    s.len = reinterpret_cast<int32_t *>(s.key + MTN);
    s.off = s.len + k.n;
    s.tok = s.off + k.n;
    s.scratch = s.tok + k.cap;
    return s;
}

__global__ __launch_bounds__(64) void metalm_seeded_kernel(MetaLMK k, int batch, const uint32_t *seeds, int32_t *features,
                                                           int32_t *labels, int32_t *overflow_row) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int row = blockIdx.x, lane = threadIdx.x;
    if (row >= batch) return;
    Lds s = carve(smem, k);
    const uint32_t seed = seeds != nullptr ? seeds[row] : k.seed_base + (uint32_t)row;
    if (lane == 0) {                                                        // init_genrand
        uint32_t p = seed;
        s.key[0] = p;
        for (int i = 1; i < MTN; ++i) {
            p = mt::seed_step(p, i);
            s.key[i] = p;
        }
    }
    __syncthreads();
    Stream g{s.key, MTN, lane};
    const size_t base = (size_t)row * (size_t)k.L;
    if (!metalm_row(k, g, s.len, s.off, s.tok, s.scratch, features + base, labels + base) && lane == 0)
        atomicMin(overflow_row, row);
}

// mt_state: [624 key words, pos]; read at the start, written back after the last row (left alone on overflow)
__global__ __launch_bounds__(64) void metalm_chained_kernel(MetaLMK k, int batch, uint32_t *mt_state, int32_t *features,
                                                            int32_t *labels, int32_t *overflow_row) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    Lds s = carve(smem, k);
    for (int i = lane; i < MTN; i += 64) s.key[i] = mt_state[i];
    const uint32_t pos = mt_state[MTN];
    __syncthreads();
    Stream g{s.key, pos > (uint32_t)MTN ? MTN : (int)pos, lane};
    for (int row = 0; row < batch; ++row) {
        const size_t base = (size_t)row * (size_t)k.L;
        if (!metalm_row(k, g, s.len, s.off, s.tok, s.scratch, features + base, labels + base)) {
            if (lane == 0) atomicMin(overflow_row, row);
            return;
        }
    }
    __syncthreads();
    for (int i = lane; i < MTN; i += 64) mt_state[i] = s.key[i];
    if (lane == 0) mt_state[MTN] = (uint32_t)g.pos;
}

// generator key, element lengths and offsets, element tokens, chunk scratch (an element is at most `cap` long)
size_t lds_bytes(int64_t n, int64_t cap) { return sizeof(uint32_t) * MTN + sizeof(int32_t) * (2 * n + 2 * cap); }

}  // namespace

extern "C" int mg_metalm_generate(const mg_metalm_params *p, int32_t batch, uint32_t seed_base, const uint32_t *seeds,
                                  uint32_t *mt_state, int32_t element_capacity, int32_t *features, int32_t *labels,
                                  int32_t *overflow_row, void *stream) {
    MG_REQUIRE_PTR(p);
    MG_REQUIRE_PTR(features); MG_REQUIRE_PTR(labels); MG_REQUIRE_PTR(overflow_row);
    if (batch <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "mg_metalm_generate: batch = %d", batch);
    // the reference's assert (metalm.py:49): n > 1 and V > 1 and l > 1 and e > 0 and e < 1 and L > 1
    if (!(p->n > 1)) return mg::set_error(MG_ERR_BAD_CONFIG, "mg_metalm_generate: n = %d (need n > 1)", p->n);
    if (!(p->V > 1)) return mg::set_error(MG_ERR_BAD_CONFIG, "mg_metalm_generate: V = %d (need V > 1)", p->V);
    if (!(p->l > 1) || !std::isfinite(p->l))
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_metalm_generate: l = %g (need 1 < l < inf)", p->l);
    if (!(p->e > 0 && p->e < 1)) return mg::set_error(MG_ERR_BAD_CONFIG, "mg_metalm_generate: e = %g (need 0 < e < 1)", p->e);
    if (!(p->L > 1)) return mg::set_error(MG_ERR_BAD_CONFIG, "mg_metalm_generate: L = %d (need L > 1)", p->L);
    if (p->V >= INT32_MAX)        // the separator V+1 is an int32 token
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_metalm_generate: V = %d (need V + 1 < 2^31)", p->V);
    if (std::isnan(p->mask_ratio)) return mg::set_error(MG_ERR_BAD_CONFIG, "mg_metalm_generate: mask_ratio is NaN");
    if ((int64_t)element_capacity < 3 * (int64_t)p->n)
        return mg::set_error(MG_ERR_BAD_SIZE, "mg_metalm_generate: element_capacity = %d < 3 n = %d", element_capacity,
                             3 * p->n);
    const size_t lds = lds_bytes(p->n, element_capacity);
    if (lds > LDS_LIMIT)
        return mg::set_error(MG_ERR_UNSUPPORTED,
                             "mg_metalm_generate: n = %d, element_capacity = %d need %zu B of LDS per row; the limit is "
                             "%zu B (2496 + 8 (n + element_capacity) <= 160 KiB)", p->n, element_capacity, lds, LDS_LIMIT);
    if (mt_state != nullptr && seeds != nullptr)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_metalm_generate: seeds and mt_state are exclusive (seeded / chained)");

    MetaLMK k{};
    k.V = p->V; k.n = p->n; k.L = p->L; k.cap = element_capacity;
    k.rng_tok = (uint32_t)(p->V - 2); k.mask_tok = mt::bound_mask(k.rng_tok);
    k.rng_idx = (uint32_t)(p->n - 2); k.mask_idx = mt::bound_mask(k.rng_idx);
    k.lam = p->l; k.e = p->e; k.mask_ratio = p->mask_ratio;
    k.ptrs = p->l >= 10;
    // random_poisson_ptrs' per-call constants and random_poisson_mult's exp(-lam), with the host's libm as numpy has them
    k.loglam = std::log(k.lam);
    k.b = 0.931 + 2.53 * std::sqrt(k.lam);
    k.a = -0.059 + 0.02483 * k.b;
    const double invalpha = 1.1239 + 1.1328 / (k.b - 3.4);
    k.log_invalpha = std::log(invalpha);
    k.vr = 0.9277 - 3.6224 / (k.b - 2);
    k.enlam = std::exp(-k.lam);
    k.seed_base = seed_base;

    mg::DeviceGuard guard(mg::device_of(features));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = mg::check_hip(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(overflow_row), INT32_MAX, 1, s),
                           "hipMemsetD32Async(overflow_row)");
    if (rc != MG_OK) return rc;
    const void *fn = mt_state != nullptr ? reinterpret_cast<const void *>(metalm_chained_kernel)
                                         : reinterpret_cast<const void *>(metalm_seeded_kernel);
    if (lds > 64 * 1024) {
        rc = mg::check_hip(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                           "hipFuncSetAttribute(metalm kernel)");
        if (rc != MG_OK) return rc;
    }
    if (mt_state != nullptr) {
        hipLaunchKernelGGL(metalm_chained_kernel, dim3(1), dim3(64), lds, s, k, batch, mt_state, features, labels,
                           overflow_row);
        return mg::check_launch("metalm_chained_kernel");
    }
    hipLaunchKernelGGL(metalm_seeded_kernel, dim3(batch), dim3(64), lds, s, k, batch, seeds, features, labels, overflow_row);
    return mg::check_launch("metalm_seeded_kernel");
}
