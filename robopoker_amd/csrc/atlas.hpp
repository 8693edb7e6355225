// atlas.hpp — the kernels of rp_atlas (include/rp_mi355x.h "abstraction atlas"): the reference's derived tables over one street's
// (isomorphism -> abstraction) lookup and the batched queries of its abstraction explorer.
// Reference: crates/daybook/src/schema.rs:78-173 (abstraction table, get_equity), crates/lloyd/src/lookup.rs:86-119
// (isomorphism.position), crates/portal/src/topology/api.rs:46-869 (TopologyAPI).  Model: tests/atlas_model.py.
//
// MI355X mapping.
//  * The (abs, obs) order.  All observations of a street have the same number of card bytes, each 1..52, so the BIGINT order of `obs`
//    is the order of the 6-bit codes of its bytes, first byte most significant: key = abs << 6c | codes (c = 2, 5, 6, 7 cards: 20, 38,
//    44, 50 bits).  The key is never stored: k_atlas_digits computes up to 27 bits of it per row straight from (obs, abs) — in table
//    order for the low bits, through the permutation of the first round for the high bits — and sortscan.hpp's stable LSD passes
//    (9 or 8 bits each, 27-bit row indices as values) sort the digits.  DESIGN.md §4e has the byte count against a 64-bit-key pass.
//  * population: LDS histogram per workgroup, 256 global atomics each; offset: one workgroup's scan; position: one scattered store
//    per sorted slot.
//  * equity: one wavefront per bucket.  The transition rows of a bucket are its centroid's bins with a count, by density descending,
//    stable over the bin: every lane ranks four bins by counting the bins in front of them (no sort), lane 0 folds in that order.
//  * queries: one lane per query, except neighbours and histograms (one wavefront per query: four candidate buckets / bins a lane).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "obs.hpp"
#include "rp_internal.h"
#include "sortscan.hpp"

namespace rp {
namespace atlas {

constexpr uint32_t MAX_K = 256;
constexpr uint32_t MAX_NEIGHBORS = 16;
constexpr uint32_t MAX_WINDOW = 16;

// what the query kernels read: device pointers owned by the handle (keys / abs by its rp_lookup)
struct View {
    const uint64_t* keys;      // the lookup's search keys, table order
    const uint8_t* abs_;       // [n]
    const int64_t* obs;        // [n]
    const uint32_t* population;  // [K]
    const uint32_t* offset;    // [K + 1]
    const uint32_t* members;   // [n] rows by (abs, obs)
    const uint32_t* position;  // [n]
    const float* equity;       // [K]
    const float* fold;         // [K] un-normalised fold of dx * next.equity (NULL on the river)
    const uint32_t* rows;      // [K] transition rows of the bucket (NULL on the river)
    const float* tri;          // [K (K - 1) / 2] or NULL
    const float* row_equity;   // [n] or NULL
    const uint32_t* future;    // [K][bins] or NULL
    const uint64_t* weight;    // [K] or NULL
    uint64_t n;
    uint32_t K, bins, street, n_cards;
    float n_observations, n_isomorphisms, n_children;
};

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Pair::merge (lloyd/src/pair.rs:59-62) for a != b
__device__ __forceinline__ uint32_t tri_index(uint32_t a, uint32_t b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    return hi * (hi - 1u) / 2u + lo;
}
// RANDOM() * population: u = (draw >> 11) * 2^-53, floor(u * population) — below population for every draw (u <= 1 - 2^-53 and
// the product rounds to population only if population * 2^-53 is under half an ulp of it, which it never is); min() guards the index
__device__ __forceinline__ uint32_t draw_index(uint64_t draw, uint32_t population) {
    const double u = (double)(draw >> 11) * 0x1.0p-53;
    const uint32_t i = (uint32_t)(u * (double)population);
    return i < population ? i : population - 1u;
}
__device__ __forceinline__ rp_atlas_sample zero_sample() {
    rp_atlas_sample s;
    s.obs = 0, s.equity = s.density = s.distance = 0.0f, s.position = s.population = 0u, s.abs = 0, s.reserved[0] = s.reserved[1] = 0;
    return s;
}
// the row of an observation under any suit labelling, -1 if it is no observation of the street or not in the table
__device__ __forceinline__ int64_t find_row(const View& v, int64_t obs) {
    uint64_t po, pu, cp, cb;
    obs_decode(obs, &po, &pu);
    if (__popcll(po) != 2 || (uint32_t)__popcll(pu) + 2u != v.n_cards || (po & pu)) return -1;
    canonical(po, pu, &cp, &cb);
    return table_find(v.keys, v.n, search_key(cp, cb));
}

// ---- the derivation ------------------------------------------------------------------------------------------------------
// bits [shift, shift + width) of the row's (abs, obs) key; perm == NULL: table order, and vals gets the row indices
static __global__ __launch_bounds__(256) void k_atlas_digits(const int64_t* obs, const uint8_t* abs_, const uint32_t* perm, uint32_t n, uint32_t n_cards,
                                                             uint32_t shift, uint32_t width, uint32_t* keys, uint32_t* vals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t row = perm ? perm[i] : i;
    const uint64_t o = (uint64_t)obs[row];
    uint64_t key = abs_[row];
    for (uint32_t c = n_cards; c-- > 0u;) key = key << 6 | ((o >> (8u * c)) & 63u);  // a card byte is 1..52: its low six bits
    keys[i] = (uint32_t)(key >> shift) & ((1u << width) - 1u);
    if (!perm) vals[i] = i;
}
// population[k] += rows with abs == k; *bad += rows with abs >= K.  population and bad are zero on entry
static __global__ __launch_bounds__(256) void k_atlas_population(const uint8_t* abs_, uint32_t n, uint32_t K, uint32_t* population, uint32_t* bad) {
    __shared__ uint32_t h[MAX_K];
    h[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) atomicAdd(&h[abs_[i]], 1u);
    __syncthreads();
    const uint32_t c = h[threadIdx.x];
    if (c) atomicAdd(threadIdx.x < K ? &population[threadIdx.x] : bad, c);
}
static __global__ __launch_bounds__(256) void k_atlas_offsets(const uint32_t* population, uint32_t K, uint32_t* offset) {
    __shared__ uint64_t wt[4];
    const uint32_t c = threadIdx.x < K ? population[threadIdx.x] : 0u;
    uint64_t tot;
    const uint64_t at = ss::block_exscan64(c, wt, &tot);
    if (threadIdx.x < K) offset[threadIdx.x] = (uint32_t)at;
    if (threadIdx.x == 0) offset[K] = (uint32_t)tot;
}
static __global__ __launch_bounds__(256) void k_atlas_position(const uint32_t* members, const uint8_t* abs_, const uint32_t* offset, uint32_t n,
                                                               uint32_t* position) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t row = members[j];
    position[row] = j - offset[abs_[row]];
}
static __global__ __launch_bounds__(256) void k_atlas_river_equity(uint32_t K, float* equity) {
    if (threadIdx.x < K) equity[threadIdx.x] = (float)threadIdx.x / 100.0f;
}
// get_equity (schema.rs:100-107) of bucket blockIdx.x: SUM(dx * next.equity) / SUM(dx) over its transition rows, each SUM a left fold
// in f32 from 0 in the order rp_artifact_write_transitions writes the rows
static __global__ __launch_bounds__(64) void k_atlas_equity(const uint32_t* future, const uint64_t* weight, uint32_t bins, const float* next_equity,
                                                            float* equity, float* fold, uint32_t* rows) {
    __shared__ float dx[MAX_K];
    __shared__ uint32_t order[MAX_K];
    const uint32_t k = blockIdx.x, ln = threadIdx.x;
    const float w = (float)weight[k];
    for (uint32_t b = ln; b < MAX_K; b += 64u) {
        const uint32_t c = b < bins ? future[(size_t)k * bins + b] : 0u;
        dx[b] = c ? (float)c / w : -1.0f;  // a density is positive; -1 marks a bin with no row
    }
    wave_lds_sync();
    uint32_t mine = 0;
    for (uint32_t b = ln; b < bins; b += 64u) {
        const float d = dx[b];
        if (d < 0.0f) continue;
        uint32_t rank = 0;
        for (uint32_t o = 0; o < bins; ++o) rank += (dx[o] > d || (dx[o] == d && o < b)) ? 1u : 0u;
        order[rank] = b;
        mine += 1u;
    }
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    wave_lds_sync();
    if (ln != 0) return;
    float num = 0.0f, den = 0.0f;
    for (uint32_t r = 0; r < mine; ++r) {
        const float d = dx[order[r]];
        num = num + d * next_equity[order[r]];
        den = den + d;
    }
    equity[k] = (mine == 0u || den == 0.0f) ? 0.0f : num / den;
    fold[k] = num;
    rows[k] = mine;
}

// ---- the queries ------------------------------------------------------------------------------------------------------------
// the member of bucket k at position i, as a record (density over n_isomorphisms, api.rs:299)
__device__ __forceinline__ rp_atlas_sample member_sample(const View& v, uint32_t k, uint32_t i, uint32_t population) {
    rp_atlas_sample s = zero_sample();
    s.abs = (int16_t)(v.street << 8 | k);
    s.equity = v.equity[k];
    s.population = population;
    s.density = (float)population / v.n_isomorphisms;
    if (population) {
        s.position = i;
        s.obs = v.obs[v.members[v.offset[k] + i]];
    }
    return s;
}
static __global__ __launch_bounds__(256) void k_atlas_describe(View v, uint64_t n, const int64_t* obs, const uint8_t* wrt, rp_atlas_sample* out,
                                                               uint8_t* status) {
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= n) return;
    rp_atlas_sample s = zero_sample();
    uint8_t st = RP_ATLAS_OK;
    const int64_t row = find_row(v, obs[q]);
    if (row < 0) {
        st = RP_ATLAS_MISS;
    } else if (wrt && wrt[q] >= v.K) {
        st = RP_ATLAS_RANGE;
    } else {
        const uint32_t k = v.abs_[row];
        s.obs = v.obs[row];
        s.abs = (int16_t)(v.street << 8 | k);
        s.equity = v.equity[k];
        s.population = v.population[k];
        s.position = v.position[row];
        s.density = (float)s.population / v.n_observations;  // api.rs:266
        if (wrt) {
            if (wrt[q] == k) st = RP_ATLAS_SAME;
            else s.distance = v.tri[tri_index(k, wrt[q])];
        }
    }
    out[q] = s;
    status[q] = st;
}
static __global__ __launch_bounds__(256) void k_atlas_obs_equity(View v, uint64_t n, const int64_t* obs, float* out, uint8_t* status) {
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= n) return;
    const int64_t row = find_row(v, obs[q]);
    float e = 0.0f;
    uint8_t st = RP_ATLAS_OK;
    if (row < 0) st = RP_ATLAS_MISS;
    else if (v.row_equity) e = v.row_equity[row];
    else if (v.rows[v.abs_[row]] == 0u) st = RP_ATLAS_EMPTY;
    else e = v.fold[v.abs_[row]];
    out[q] = e;
    status[q] = st;
}
static __global__ __launch_bounds__(256) void k_atlas_pick(View v, uint64_t n, const uint8_t* abs_, const uint64_t* draw, rp_atlas_sample* out,
                                                           uint8_t* status) {
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= n) return;
    const uint32_t k = abs_[q];
    if (k >= v.K) {
        out[q] = zero_sample();
        status[q] = RP_ATLAS_RANGE;
        return;
    }
    const uint32_t population = v.population[k];
    out[q] = member_sample(v, k, population ? draw_index(draw[q], population) : 0u, population);
    status[q] = population ? RP_ATLAS_OK : RP_ATLAS_EMPTY;
}
// one wavefront per query: lane l holds the candidates l, l + 64, l + 128, l + 192; a candidate's slot is the number of candidates
// in front of it (nearer / farther, ties to the smaller index)
static __global__ __launch_bounds__(256) void k_atlas_neighbors(View v, uint64_t n, const uint8_t* wrt, uint32_t k, int farthest, const uint64_t* draws,
                                                                rp_atlas_sample* out, uint8_t* status) {
    __shared__ float dist[4][MAX_K];
    const uint32_t ln = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t q = (uint64_t)blockIdx.x * 4u + wv;
    if (q >= n) return;  // whole wavefronts leave
    const uint32_t w = wrt[q];
    if (w >= v.K) {
        if (ln < k) {
            out[q * k + ln] = zero_sample();
            status[q * k + ln] = RP_ATLAS_RANGE;
        }
        return;
    }
    for (uint32_t c = ln; c < v.K; c += 64u) dist[wv][c] = c == w ? 0.0f : v.tri[tri_index(c, w)];
    wave_lds_sync();
    for (uint32_t c = ln; c < v.K; c += 64u) {
        if (c == w) continue;
        const float d = dist[wv][c];
        uint32_t rank = 0;
        for (uint32_t o = 0; o < v.K; ++o) {
            if (o == w) continue;
            const float e = dist[wv][o];
            rank += ((farthest ? e > d : e < d) || (e == d && o < c)) ? 1u : 0u;
        }
        if (rank >= k) continue;
        const uint32_t population = v.population[c];
        rp_atlas_sample s = member_sample(v, c, draws && population ? draw_index(draws[q * k + rank], population) : 0u, draws ? population : 0u);
        s.population = population;
        s.density = (float)population / v.n_isomorphisms;
        s.distance = d;
        out[q * k + rank] = s;
        status[q * k + rank] = draws && !population ? RP_ATLAS_EMPTY : RP_ATLAS_OK;
    }
}
static __global__ __launch_bounds__(256) void k_atlas_distance(View v, uint64_t n, const uint8_t* a, const uint8_t* b, float* out) {
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= n) return;
    const uint32_t x = a[q], y = b[q];
    out[q] = (x >= v.K || y >= v.K) ? __uint_as_float(0x7fc00000u) : (x == y ? 0.0f : v.tri[tri_index(x, y)]);
}
static __global__ __launch_bounds__(256) void k_atlas_members(View v, uint64_t n, const uint8_t* abs_, const uint32_t* start, uint32_t count, int64_t* out,
                                                              uint8_t* got) {
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= n) return;
    const uint32_t k = abs_[q], population = k < v.K ? v.population[k] : 0u, s = start[q];
    const uint32_t have = s < population ? (population - s < count ? population - s : count) : 0u;
    for (uint32_t j = 0; j < count; ++j) out[q * count + j] = j < have ? v.obs[v.members[v.offset[k] + s + j]] : 0;
    got[q] = (uint8_t)have;
}
// one wavefront per query; OBS: lane 0 finds the row, the wavefront shares its bucket
static __global__ __launch_bounds__(256) void k_atlas_histograms(View v, uint64_t n, int kind, const void* ids, uint32_t* counts, uint8_t* status) {
    const uint32_t ln = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t q = (uint64_t)blockIdx.x * 4u + wv;
    if (q >= n) return;
    uint32_t k = v.K;
    uint8_t st = RP_ATLAS_OK;
    if (ln == 0) {
        if (kind == RP_ATLAS_HIST_ABS) {
            k = static_cast<const uint8_t*>(ids)[q];
            if (k >= v.K) st = RP_ATLAS_RANGE;
        } else {
            const int64_t row = find_row(v, static_cast<const int64_t*>(ids)[q]);
            if (row < 0) st = RP_ATLAS_MISS;
            else k = v.abs_[row];
        }
        if (st == RP_ATLAS_OK && v.rows[k] == 0u) st = RP_ATLAS_EMPTY;
        status[q] = st;
    }
    k = __shfl(k, 0, 64);
    st = (uint8_t)__shfl((uint32_t)st, 0, 64);
    const bool live = st == RP_ATLAS_OK || st == RP_ATLAS_EMPTY;
    const float w = live ? (float)v.weight[k] : 1.0f;
    for (uint32_t b = ln; b < v.bins; b += 64u) {
        const uint32_t c = live ? v.future[(size_t)k * v.bins + b] : 0u;
        const float dx = c ? (float)c / w : 0.0f;
        counts[q * v.bins + b] = kind == RP_ATLAS_HIST_ABS ? (uint32_t)(dx * 1000.0f) : (uint32_t)roundf(dx * v.n_children);
    }
}

}  // namespace atlas
}  // namespace rp
