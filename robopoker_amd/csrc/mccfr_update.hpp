// mccfr_update.hpp — the update kernels of mccfr.hip (Solver::update_*, solver.rs:143-192): the stable counting sort of a batch's
// Decisions (k_count / k_scan / k_compact, k_count_small / k_compact_small), the ordered chains (k_chain), the block maps of the
// composed update (k_block_maps, k_chunk_maps), their two-level fold (k_combine2) and the multi-GPU exchange (k_fold, k_accumulate).
#ifndef RP_MCCFR_UPDATE_HPP
#define RP_MCCFR_UPDATE_HPP

#include "mccfr_kernels.hpp"
#include "mccfr_traverse.hpp"  // lane_of, DevInfoTab, prepare_one

namespace rp {

// ------------------------------------------------------------------------------------------------
// Update pipeline (Solver::update_{regret,weight,payoff,visits}, solver.rs:96-105,143-192):
//   k_count    per (infoset, 1024-tree chunk): how many trees of the chunk produced Decisions for it
//   k_scan     per infoset: exclusive scan of the chunk counts -> offsets, segment length
//   k_compact  scatter the Decisions into ONE tree-id-ordered segment per infoset (stable counting sort)
//   k_chain    per infoset: stream the segment through LDS tiles and apply the touches sequentially,
//              one lane per table cell (the reference's order-dependent semantics, bit for bit)
// ------------------------------------------------------------------------------------------------
// CH_TREES (trees per compaction chunk), SM_WORDS and DevSorted live in mccfr_kernels.hpp
#define CH_THREADS 256u   // small-game kernels: one tree per thread
#define SLOT_THREADS (CH_TREES / 4u)  // slot-map kernels: four slot-map bytes per thread

__device__ __forceinline__ uint32_t chunk_slots(const DevDecisions& dc, uint32_t info, uint32_t t0, uint32_t batch) {
    uint32_t slots = 0;
    if (t0 + 4 <= batch) {
        slots = *reinterpret_cast<const uint32_t*>(&dc.slotmap[(size_t)info * dc.stride + t0]);
    } else {
        for (uint32_t k = 0; k < 4; ++k)
            if (t0 + k < batch) slots |= (uint32_t)dc.slotmap[(size_t)info * dc.stride + t0 + k] << (8 * k);
    }
    return slots;
}
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t v) {
    return ((v & 0xffu) != 0) + ((v & 0xff00u) != 0) + ((v & 0xff0000u) != 0) + ((v & 0xff000000u) != 0);
}
// block-wide exclusive scan over the blockDim.x threads in thread order; returns (exclusive prefix, total)
__device__ __forceinline__ uint32_t block_exscan(uint32_t v, uint32_t* wave_tot, uint32_t* total) {
    const uint32_t tid = threadIdx.x;
    uint32_t incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, 64);
        if ((int)(tid & 63) >= d) incl += o;
    }
    if ((tid & 63) == 63) wave_tot[tid >> 6] = incl;
    __syncthreads();
    uint32_t wbase = 0, tot = 0;
    for (uint32_t w = 0; w < blockDim.x / 64; ++w) {
        const uint32_t c = wave_tot[w];
        if (w < (tid >> 6)) wbase += c;
        tot += c;
    }
    __syncthreads();
    *total = tot;
    return wbase + incl - v;
}

__global__ __launch_bounds__(SLOT_THREADS) void k_count(DevGame g, DevDecisions dc, DevSorted so, StepParams p) {
    __shared__ uint32_t wave_tot[CH_THREADS / 64];
    const uint32_t info = blockIdx.y, chunk = blockIdx.x;
    if (g.info_player[info] != p.walker) return;
    const uint32_t t0 = chunk * CH_TREES + threadIdx.x * 4;
    uint32_t cnt = nonzero_bytes(chunk_slots(dc, info, t0, p.batch));
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (uint32_t w = 0; w < blockDim.x / 64; ++w) c += wave_tot[w];
        so.counts[(size_t)info * so.n_chunks + chunk] = c;
    }
}

__global__ __launch_bounds__(CH_THREADS) void k_scan(DevGame g, DevSorted so, StepParams p) {
    __shared__ uint32_t wave_tot[CH_THREADS / 64];
    const uint32_t info = blockIdx.x;
    if (g.info_player[info] != p.walker) {
        if (threadIdx.x == 0) so.total[info] = 0;
        return;
    }
    uint32_t carry = 0;
    for (uint32_t base = 0; base < so.n_chunks; base += CH_THREADS) {
        const uint32_t c = base + threadIdx.x;
        const uint32_t v = c < so.n_chunks ? so.counts[(size_t)info * so.n_chunks + c] : 0u;
        uint32_t tot;
        const uint32_t ex = block_exscan(v, wave_tot, &tot);
        if (c < so.n_chunks) so.offs[(size_t)info * so.n_chunks + c] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) so.total[info] = carry;
}

__global__ __launch_bounds__(SLOT_THREADS) void k_compact(DevGame g, DevDecisions dc, DevSorted so, StepParams p) {
    __shared__ uint32_t wave_tot[CH_THREADS / 64];
    __shared__ uint32_t sh_base;
    const uint32_t info = blockIdx.y, chunk = blockIdx.x;
    if (g.info_player[info] != p.walker) return;
    // segment base = sum of the lengths of all lower infosets
    uint32_t part = 0;
    for (uint32_t i = threadIdx.x; i < info; i += blockDim.x) part += so.total[i];
    for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d, 64);
    if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t b0 = so.offs[(size_t)info * so.n_chunks + chunk];
        for (uint32_t w = 0; w < blockDim.x / 64; ++w) b0 += wave_tot[w];
        sh_base = b0;
    }
    __syncthreads();
    const uint32_t A = g.A, nact = g.info_actions[info];
    const uint32_t t0 = chunk * CH_TREES + threadIdx.x * 4;
    const uint32_t slots = chunk_slots(dc, info, t0, p.batch);
    uint32_t tot;
    uint32_t rank = block_exscan(nonzero_bytes(slots), wave_tot, &tot);
    const float tf = (float)p.epoch;
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t sl = (slots >> (8 * k)) & 0xffu;
        if (!sl) continue;
        const uint32_t tree = t0 + k, slot = sl - 1;
        const size_t pos = (size_t)sh_base + rank;
        for (uint32_t a = 0; a < A; ++a) {  // the scatter, as in k_compact_small: behind a shared call both kernels compile differently
            float rd = 0.0f, wd = 0.0f;
            if (a < nact) {
                rd = dc.regret[(slot * A + a) * dc.stride + tree];
                const float sg = dc.policy[(slot * A + a) * dc.stride + tree];
                wd = weight_delta(p.W, sg, tf);
            }
            so.rw[pos * 2 * A + a] = rd;
            so.rw[pos * 2 * A + A + a] = wd;
        }
        so.mask[pos] = dc.mask[slot * dc.stride + tree];
        so.payoff[pos] = dc.payoff[slot * dc.stride + tree];
        rank += 1;
    }
}

// ---- games whose per-chunk bitmap fits in LDS (56 B per infoset): the same stable counting sort without the
// per-infoset slot map in HBM --------
// One workgroup per chunk of CH_TREES trees.  A tree's Decisions are marked in an LDS bitmap [infoset][tree]; the
// rank of a Decisions inside its (chunk, infoset) bucket — its place in tree-id order — is a prefix popcount of that
// bitmap row.  Every Decisions is read once; nothing is scanned per infoset.
#define CM_PASSES 4u  // k_chunk_maps: infosets per thread; 4 * 256 infosets * 56 B is past its 64 KB LDS budget
__device__ __forceinline__ void chunk_bitmap(const DevDecisions& dc, uint32_t n_infos, uint32_t chunk, uint32_t batch,
                                             uint32_t* bits) {
    for (uint32_t e = threadIdx.x; e < n_infos * SM_WORDS; e += CH_THREADS) bits[e] = 0;
    __syncthreads();
    for (uint32_t lt = threadIdx.x; lt < CH_TREES; lt += CH_THREADS) {
        const uint32_t tree = chunk * CH_TREES + lt;  // coalesced over threads
        if (tree >= batch) continue;
        const uint32_t nd = dc.ndec[tree];
        for (uint32_t slot = 0; slot < nd; ++slot)
            atomicOr(&bits[dc.info[slot * dc.stride + tree] * SM_WORDS + (lt >> 5)], 1u << (lt & 31u));
    }
    __syncthreads();
}
// exclusive scan of in[0..n) into out[0..n) (both LDS), any n, by the whole workgroup
__device__ __forceinline__ void lds_exscan(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* wave_tot) {
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += blockDim.x) {
        const uint32_t i = b0 + threadIdx.x;
        uint32_t tot;
        const uint32_t ex = block_exscan(i < n ? in[i] : 0u, wave_tot, &tot);
        if (i < n) out[i] = carry + ex;
        carry += tot;
    }
    __syncthreads();
}
__global__ __launch_bounds__(CH_THREADS) void k_count_small(DevGame g, DevDecisions dc, DevSorted so, StepParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sm_lds[];
    uint32_t* bits = sm_lds;  // [n_infos][SM_WORDS]
    const uint32_t chunk = blockIdx.x;
    chunk_bitmap(dc, g.n_infos, chunk, p.batch, bits);
    for (uint32_t info = threadIdx.x; info < g.n_infos; info += CH_THREADS) {
        uint32_t c = 0;
        for (uint32_t w = 0; w < SM_WORDS; ++w) c += __popc(bits[info * SM_WORDS + w]);
        so.counts[(size_t)info * so.n_chunks + chunk] = c;
    }
}
__global__ __launch_bounds__(CH_THREADS) void k_compact_small(DevGame g, DevDecisions dc, DevSorted so, StepParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sm_lds[];
    __shared__ uint32_t wave_tot[CH_THREADS / 64];
    const uint32_t NI = g.n_infos;
    uint32_t* bits = sm_lds;                                        // [NI][SM_WORDS]
    uint32_t* base = bits + NI * SM_WORDS;                          // [NI] first position of the (chunk, infoset) bucket
    uint32_t* tots = base + NI;                                     // [NI] segment lengths
    uint16_t* pre = reinterpret_cast<uint16_t*>(tots + NI);         // [NI][SM_WORDS] trees before word w that visited the infoset
    const uint32_t chunk = blockIdx.x;
    chunk_bitmap(dc, g.n_infos, chunk, p.batch, bits);
    for (uint32_t info = threadIdx.x; info < g.n_infos; info += CH_THREADS) {  // list_prefix; the row's count is not needed here
        uint32_t run = 0;
        for (uint32_t w = 0; w < SM_WORDS; ++w) {
            pre[info * SM_WORDS + w] = (uint16_t)run;
            run += __popc(bits[info * SM_WORDS + w]);
        }
    }
    // bucket base = sum of the lengths of all lower infosets + this chunk's offset inside the infoset's segment
    for (uint32_t info = threadIdx.x; info < NI; info += CH_THREADS) tots[info] = so.total[info];
    __syncthreads();
    lds_exscan(tots, base, NI, wave_tot);
    for (uint32_t info = threadIdx.x; info < NI; info += CH_THREADS) base[info] += so.offs[(size_t)info * so.n_chunks + chunk];
    __syncthreads();
    const uint32_t A = g.A;
    const float tf = (float)p.epoch;
    for (uint32_t lt = threadIdx.x; lt < CH_TREES; lt += CH_THREADS) {
        const uint32_t tree = chunk * CH_TREES + lt;
        if (tree >= p.batch) continue;
        const uint32_t nd = dc.ndec[tree];
        for (uint32_t slot = 0; slot < nd; ++slot) {
            const uint32_t info = dc.info[slot * dc.stride + tree];
            const uint32_t nact = g.info_actions[info];
            const size_t pos = (size_t)base[info] + list_rank(bits, pre, info, lt);
            for (uint32_t a = 0; a < A; ++a) {  // the scatter of k_compact, kept equal to it
                float rd = 0.0f, wd = 0.0f;
                if (a < nact) {
                    rd = dc.regret[(slot * A + a) * dc.stride + tree];
                    const float sg = dc.policy[(slot * A + a) * dc.stride + tree];
                    wd = weight_delta(p.W, sg, tf);
                }
                so.rw[pos * 2 * A + a] = rd;
                so.rw[pos * 2 * A + A + a] = wd;
            }
            so.mask[pos] = dc.mask[slot * dc.stride + tree];
            so.payoff[pos] = dc.payoff[slot * dc.stride + tree];
        }
    }
}

// per-epoch discount constants of a RegretSchedule (regret/{linear,discounted,asymmetric}.rs)
struct Discount {
    float pos, neg, zero;
};
__device__ __forceinline__ Discount regret_discount(int R, float t, float pow15, float pow05) {
    Discount d{1.0f, 1.0f, 1.0f};
    const float lin = t / (t + 1.0f);
    if (R == RP_REGRET_LINEAR) d = Discount{lin, lin, lin};
    else if (R == RP_REGRET_ASYMMETRIC) d = Discount{1.0f, lin, lin};
    else if (R == RP_REGRET_DISCOUNTED) {
        const float xp = pow15, xn = pow05, xz = t / 1.0f;
        d = Discount{xp / (xp + 1.0f), xn / (xn + 1.0f), xz / (xz + 1.0f)};
    }
    return d;
}
__device__ __forceinline__ uint32_t seg_base(const DevSorted& so, uint32_t info) {
    uint32_t part = 0;
    for (uint32_t i = lane_of(); i < info; i += 64) part += so.total[i];
    for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d, 64);
    return part;
}

#define TILE_FLOATS 1024u  // regret/weight deltas per LDS tile (16 per lane)
#define TILE_REGS (TILE_FLOATS / 64u)
#define TILE_PAD 4u        // row padding of the stream-major tile (keeps 16-B alignment, staggers banks)
#define PTILE 1024u        // payoffs per LDS tile

// LDS carve of k_chain (bytes): regret/weight tiles, mask tiles, payoff / reciprocal / divisor tiles
#define CHAIN_TILE_WORDS (TILE_FLOATS + 2u * RP_MAX_ACTIONS * TILE_PAD)
#define CHAIN_LDS_WORDS (2u * CHAIN_TILE_WORDS + 2u * (TILE_FLOATS / 2u) + 7u * PTILE)

// wave 0: regret + weight cells, universal op acc <- max(acc * d + delta, floor) (x * 1.0f is exact, so Summed /
// Floored / Constant / Linear-weight schedules are the same instruction stream with d = 1).  wave 1: payoff + visits.
// Tiles are double buffered: the global loads of tile t+1 are issued into registers BEFORE the chain over tile t
// and committed to LDS after it, so HBM/L2 latency hides under the serial chain.  In LDS a tile is stream-major
// ([cell][entry]) so each chain lane reads its own stream 4 entries at a time (ds_read_b128), 16 entries ahead.
template <bool SIGNED, bool PRUNED>
__global__ __launch_bounds__(128) void k_chain(DevGame g, DevTables t, DevSorted so, StepParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t info = blockIdx.x;
    if (g.info_player[info] != p.walker) return;
    const uint32_t len = so.total[info];
    if (len == 0) return;
    const uint32_t A = g.A, nact = g.info_actions[info], W2 = 2 * A;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const size_t base = seg_base(so, info);
    const float tf = (float)p.epoch;
    float* tile = reinterpret_cast<float*>(smem);                                  // [2][CHAIN_TILE_WORDS]
    uint32_t* mtile = reinterpret_cast<uint32_t*>(tile + 2 * CHAIN_TILE_WORDS);    // [2][TILE_FLOATS / 2]
    float* ptile = reinterpret_cast<float*>(mtile + TILE_FLOATS);                  // [2][3][PTILE]: payoff, 1/b, b
    if (wave == 0) {
        const uint32_t T = (TILE_FLOATS / W2) & ~3u;  // Decisions per tile, multiple of 4
        const uint32_t TP = T + TILE_PAD;             // row stride of the stream-major tile
        const bool isreg = lane < A;
        const uint32_t a = lane % A;
        const bool chain = lane < W2 && a < nact;
        const size_t cell = (size_t)info * A + a;
        float acc = 0.0f, fl = RP_EPSILON;
        Discount d{1.0f, 1.0f, 1.0f};
        if (chain) {
            if (isreg) {
                acc = t.regret[cell];
                fl = regret_floor_of(p.R, p.regret_min);
                d = regret_discount(p.R, tf, p.pow15, p.pow05);
            } else {
                acc = t.weight[cell];
                const float dw = p.W == RP_WEIGHT_EXPONENTIAL ? 0.9999f : 1.0f;
                d = Discount{dw, dw, dw};
            }
        }
        const uint32_t ntiles = (len + T - 1) / T;
        float rg[TILE_REGS];
        uint32_t mk[TILE_REGS / 2];
        auto issue = [&](uint32_t tl) {
            const size_t e0 = (base + (size_t)tl * T) * W2;
            const uint32_t ne = min(T, len - tl * T), nfl = ne * W2;
#pragma unroll
            for (uint32_t r = 0; r < TILE_REGS; ++r) {
                const uint32_t k = lane + 64 * r;
                rg[r] = k < nfl ? so.rw[e0 + k] : 0.0f;
            }
            if (PRUNED) {
#pragma unroll
                for (uint32_t r = 0; r < TILE_REGS / 2; ++r) {
                    const uint32_t k = lane + 64 * r;
                    mk[r] = k < ne ? so.mask[base + (size_t)tl * T + k] : 0u;
                }
            }
        };
        auto commit = [&](uint32_t buf) {  // entry-major registers -> stream-major LDS
#pragma unroll
            for (uint32_t r = 0; r < TILE_REGS; ++r) {
                const uint32_t k = lane + 64 * r;
                if (k < T * W2) tile[buf * CHAIN_TILE_WORDS + (k % W2) * TP + k / W2] = rg[r];
            }
            if (PRUNED) {
#pragma unroll
                for (uint32_t r = 0; r < TILE_REGS / 2; ++r) mtile[buf * (TILE_FLOATS / 2) + lane + 64 * r] = mk[r];
            }
        };
        auto step = [&](float delta, uint32_t m) {
            float dd = d.zero;
            if (SIGNED) dd = acc > 0.0f ? d.pos : (acc < 0.0f ? d.neg : d.zero);
            const float nv = rp_maxf(acc * dd + delta, fl);
            if (PRUNED) acc = (isreg && !((m >> a) & 1u)) ? acc : nv;
            else acc = nv;
        };
        issue(0);
        commit(0);
        __builtin_amdgcn_wave_barrier();
        for (uint32_t tl = 0; tl < ntiles; ++tl) {
            const uint32_t buf = tl & 1u;
            const bool more = tl + 1 < ntiles;
            if (more) issue(tl + 1);
            const uint32_t n = min(T, len - tl * T);
            const float* row = tile + buf * CHAIN_TILE_WORDS + (chain ? lane : 0u) * TP;
            const uint32_t* mrow = mtile + buf * (TILE_FLOATS / 2);
            if (chain) {
                const uint32_t n16 = n & ~15u;
                uint32_t i = 0;
                if (n16) {
                    float4 c0 = *reinterpret_cast<const float4*>(row + 0), c1 = *reinterpret_cast<const float4*>(row + 4);
                    float4 c2 = *reinterpret_cast<const float4*>(row + 8), c3 = *reinterpret_cast<const float4*>(row + 12);
                    for (; i < n16; i += 16) {
                        float4 x0 = c0, x1 = c1, x2 = c2, x3 = c3;
                        if (i + 16 < n16) {  // the next 16 entries travel from LDS while these 16 are chained
                            c0 = *reinterpret_cast<const float4*>(row + i + 16);
                            c1 = *reinterpret_cast<const float4*>(row + i + 20);
                            c2 = *reinterpret_cast<const float4*>(row + i + 24);
                            c3 = *reinterpret_cast<const float4*>(row + i + 28);
                        }
                        uint32_t m[16];
#pragma unroll
                        for (uint32_t q = 0; q < 16; ++q) m[q] = PRUNED ? mrow[i + q] : 0xffffffffu;
                        step(x0.x, m[0]); step(x0.y, m[1]); step(x0.z, m[2]); step(x0.w, m[3]);
                        step(x1.x, m[4]); step(x1.y, m[5]); step(x1.z, m[6]); step(x1.w, m[7]);
                        step(x2.x, m[8]); step(x2.y, m[9]); step(x2.z, m[10]); step(x2.w, m[11]);
                        step(x3.x, m[12]); step(x3.y, m[13]); step(x3.z, m[14]); step(x3.w, m[15]);
                    }
                }
                for (; i < n; ++i) step(row[i], PRUNED ? mrow[i] : 0xffffffffu);
            }
            if (more) commit(buf ^ 1u);
            __builtin_amdgcn_wave_barrier();
        }
        if (chain) {
            if (isreg) t.regret[cell] = acc;
            else t.weight[cell] = acc;
        }
    } else {
        // Welford mean with the pre-increment visit count (solver.rs:174-192): ev += (payoff - ev) / (n + 1).
        // The divisor sequence is known in advance, so the whole wave precomputes b = (float)(n+1) and the
        // correctly rounded 1/b per entry; the serial chain then needs mul + 2 fma per division
        // (rp_div_by_recip1) and each quotient carries an exact off-path proof that it equals IEEE a / b.
        const bool chain = lane < nact;
        const size_t cell = (size_t)info * A + lane;
        float ev = 0.0f;
        uint32_t visits = 0;
        if (chain) {
            ev = t.payoff[cell];
            visits = t.visits[cell];
        }
        const uint32_t v0 = __shfl(visits, 0, 64);
        const float ev0 = __shfl(ev, 0, 64);
        // every edge of an infoset is always visited together, so all its (payoff, visits) cells hold the same
        // value and ONE chain serves them; anything else (a hand-made import: test_non_uniform_infosets_take_the_plain_path) takes the plain path below
        const bool uniform = __all(!chain || (visits == v0 && rp_f2u(ev) == rp_f2u(ev0)));
        float* hist = ptile + 6 * PTILE;  // [PTILE] ev after each touch of the current tile
        if (uniform) ev = ev0;
        const float ev_start = ev;
        if (uniform) {
            const uint32_t ntiles = (len + PTILE - 1) / PTILE;
            float rg[PTILE / 64];
            auto issue = [&](uint32_t tl) {
                const uint32_t n = min(PTILE, len - tl * PTILE);
#pragma unroll
                for (uint32_t r = 0; r < PTILE / 64; ++r) {
                    const uint32_t k = lane + 64 * r;
                    rg[r] = k < n ? so.payoff[base + (size_t)tl * PTILE + k] : 0.0f;
                }
            };
            auto commit = [&](uint32_t tl, uint32_t buf) {
                float* pt = ptile + buf * 3 * PTILE;
#pragma unroll
                for (uint32_t r = 0; r < PTILE / 64; ++r) {
                    const uint32_t k = lane + 64 * r;
                    const float b = (float)(v0 + tl * PTILE + k + 1u);  // (n + 1) as f32 (solver.rs:179)
                    pt[k] = rg[r];
                    pt[PTILE + k] = 1.0f / b;
                    pt[2 * PTILE + k] = b;
                }
            };
            issue(0);
            commit(0, 0);
            __builtin_amdgcn_wave_barrier();
            for (uint32_t tl = 0; tl < ntiles; ++tl) {
                const uint32_t buf = tl & 1u;
                const bool more = tl + 1 < ntiles;
                if (more) issue(tl + 1);
                const uint32_t n = min(PTILE, len - tl * PTILE);
                const float* pt = ptile + buf * 3 * PTILE;
#ifndef RP_EXPERIMENT_SKIP_PAYOFF
                // (1) the serial chain: 5 VALU ops per touch (sub, mul, fma, fma, add); lane 0 logs ev after each touch
                const float ev_tile = ev;
                {
                    auto fast = [&](float pv, float rv, float bv) {
                        const float s = pv - ev;
                        const float q0 = s * rv;
                        const float e0 = fmaf(-bv, q0, s);
                        ev += fmaf(e0, rv, q0);
                        return ev;
                    };
                    const uint32_t n4 = n & ~3u;
                    uint32_t i = 0;
                    for (; i < n4; i += 4) {
                        const float4 pv = *reinterpret_cast<const float4*>(pt + i);
                        const float4 rv = *reinterpret_cast<const float4*>(pt + PTILE + i);
                        const float4 bv = *reinterpret_cast<const float4*>(pt + 2 * PTILE + i);
                        float4 h;
                        h.x = fast(pv.x, rv.x, bv.x); h.y = fast(pv.y, rv.y, bv.y);
                        h.z = fast(pv.z, rv.z, bv.z); h.w = fast(pv.w, rv.w, bv.w);
                        if (lane == 0) *reinterpret_cast<float4*>(hist + i) = h;
                    }
                    for (; i < n; ++i) {
                        const float e = fast(pt[i], pt[PTILE + i], pt[2 * PTILE + i]);
                        if (lane == 0) hist[i] = e;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                // (2) the proof, lane-parallel and off the chain: every touch's quotient is re-derived from the logged
                //     ev and checked with the exact-residual criterion of rp_div_by_recip1 (== IEEE s / b when proven)
                bool bad = false;
                for (uint32_t k = lane; k < n; k += 64) {
                    const float prev = k ? hist[k - 1] : ev_tile;
                    int proven;
                    const float q = rp_div_by_recip1(pt[k] - prev, pt[2 * PTILE + k], pt[PTILE + k], &proven);
                    bad |= !proven || (prev + q != hist[k]);
                }
                if (__any(bad)) {  // rare (a quotient below 2^-97, or on a rounding tie): redo this tile with IEEE divisions.  Run by tests/test_gpu_resumed_update.py
                                   // (every tile, walker 0's tiles only, a few tiles of a hydrated table), inputs proven by tests/welford_witness.py
                    ev = ev_tile;
                    for (uint32_t k = 0; k < n; ++k) ev += (pt[k] - ev) / pt[2 * PTILE + k];
                }
                __builtin_amdgcn_wave_barrier();
#endif
                if (more) commit(tl + 1, buf ^ 1u);
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (chain) {
            if (!uniform) {  // cells of one infoset that differ in visits or in payoff bits: only after a hand-made import (rp_mccfr_import;
                             // test_non_uniform_infosets_take_the_plain_path steps such tables)
                ev = ev_start;
                uint32_t v = visits;
                for (uint32_t i = 0; i < len; ++i) {
                    ev += (so.payoff[base + i] - ev) / (float)(v + 1u);
                    v += 1u;
                }
            }
            t.payoff[cell] = ev;
            t.visits[cell] = visits + len;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Composed update (include/rp_mi355x.h rp_compose_block; oracle: ora_mccfr_step_local): the serial chain of the
// ordered mode is replaced by a two-level composition of per-cell maps F(x) = max(a x + b, m).
//   k_block_maps  one workgroup per (infoset, block of T consecutive Decisions): sequential composition inside the
//                 block, all blocks of all infosets in parallel
//   k_combine2    (group, infoset tile) workgroups: block maps -> group maps -> Cell / InfoSum blob, or straight into the tables
//   k_fold_groups batches of many groups: the group maps -> ... as a launch of its own, one workgroup per infoset
// ------------------------------------------------------------------------------------------------
// Map / map_compose live in mccfr_kernels.hpp
// block = the Decisions of infoset blockIdx.y produced by chunk blockIdx.x (RP_COMPOSE_CHUNK == CH_TREES trees):
// in the sorted layout a contiguous group.  Large games (per-infoset slot map); small games fuse the sort away, below.
template <bool PRUNED>
__global__ __launch_bounds__(128) void k_block_maps(DevGame g, DevSorted so, StepParams p, Map* bmaps) {
    __shared__ __attribute__((aligned(16))) float tile[TILE_FLOATS + 2 * RP_MAX_ACTIONS * TILE_PAD];
    __shared__ uint32_t mtile[TILE_FLOATS / 2];
    __shared__ __attribute__((aligned(16))) float ptile[TILE_FLOATS / 2];
    const uint32_t info = blockIdx.y, blk = blockIdx.x;
    if (g.info_player[info] != p.walker) return;
    const uint32_t A = g.A, nact = g.info_actions[info], W2 = 2 * A;
    const uint32_t T = compose_block(A);  // touches per LDS tile
    const uint32_t n = so.counts[(size_t)info * so.n_chunks + blk];
    const uint32_t TP = T + TILE_PAD;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const size_t base = seg_base(so, info) + so.offs[(size_t)info * so.n_chunks + blk];
    const bool isreg = lane < A;
    const uint32_t a = lane % A;
    const bool chain = lane < W2 && a < nact;
    const float tf = (float)p.epoch;
    const ChainParams cp = chain_params(p, isreg, tf);
    const float fl = cp.fl, d = cp.d;
    Map mp{1.0f, 0.0f, rp_u2f(0xff800000u), 0u};
    float psum = 0.0f;
    for (uint32_t t0 = 0; t0 < n; t0 += T) {  // the chain runs through the block tile by tile
        const uint32_t m = min(T, n - t0);
        if (wave == 0) {
            const size_t e0 = (base + t0) * W2;
            const uint32_t nfl = m * W2;
            float lr[TILE_FLOATS / 64];
#pragma unroll
            for (uint32_t q = 0; q < TILE_FLOATS / 64; ++q) {
                const uint32_t k = lane + 64 * q;
                lr[q] = k < nfl ? so.rw[e0 + k] : 0.0f;
            }
#pragma unroll
            for (uint32_t q = 0; q < TILE_FLOATS / 64; ++q) {
                const uint32_t k = lane + 64 * q;
                if (k < nfl) tile[(k % W2) * TP + k / W2] = lr[q];
            }
            if (PRUNED)
                for (uint32_t k = lane; k < m; k += 64) mtile[k] = so.mask[base + t0 + k];
        } else {
            for (uint32_t k = lane; k < m; k += 64) ptile[k] = so.payoff[base + t0 + k];
        }
        __syncthreads();
        if (wave == 0 && chain) {
            const float* row = tile + lane * TP;
            for (uint32_t i = 0; i < m; ++i) {
                const float delta = row[i];
                const bool skip = PRUNED && isreg && !((mtile[i] >> a) & 1u);
                // map_touch_unless(mp, skip, d, delta, fl), spelled out: behind a call the compiler schedules this loop differently
                const float na = mp.n ? mp.a * d : d;
                const float nb = mp.n ? mp.b * d + delta : delta;
                const float nm = mp.n ? rp_maxf(mp.m * d + delta, fl) : fl;
                mp.a = skip ? mp.a : na;
                mp.b = skip ? mp.b : nb;
                mp.m = skip ? mp.m : nm;
                mp.n += skip ? 0u : 1u;
            }
        }
        if (wave == 1 && lane == 0)
            for (uint32_t i = 0; i < m; ++i) psum += ptile[i];
        __syncthreads();
    }
    const size_t out = bmap_index(blk, g.info_rank[info], 0u, g.rank_max, W2);
    if (wave == 0 && lane < W2) bmaps[out + lane] = Map{mp.a, mp.b, mp.m, chain ? mp.n : 0u};
    if (wave == 1 && lane == 0) bmaps[out + W2] = map_sum_slot(psum, n);
}

// Small games: block maps straight from the lane-interleaved Decisions of one chunk — no sorted copy in HBM at all.
// One thread per tree.  The chunk's Decisions get their place in per-infoset, tree-ordered lists (LDS bitmap + prefix
// popcount, as k_compact_small); then, cell by cell, every thread drops its trees' values at those places in an LDS
// array (global reads coalesced over trees) and one thread per infoset composes its list sequentially out of LDS.
template <bool PRUNED, uint32_t PASSES>
__global__ __launch_bounds__(CH_THREADS) void k_chunk_maps(DevGame g, DevDecisions dc, StepParams p, Map* bmaps) {
    extern __shared__ __attribute__((aligned(16))) uint32_t cm_lds[];
    __shared__ uint32_t wave_tot[CH_THREADS / 64];
    const uint32_t NI = g.n_infos, A = g.A, W2 = 2 * A, chunk = blockIdx.x, tid = threadIdx.x, MD = dc.maxdec;
    uint32_t* bits = cm_lds;                                              // [NI][SM_WORDS]
    uint32_t* lcount = bits + NI * SM_WORDS;                              // [NI]
    uint32_t* lbase = lcount + NI;                                        // [NI]
    float* vals = reinterpret_cast<float*>(lbase + NI);                   // [MD * CH_TREES] one cell's values, list order
    uint16_t* pre = reinterpret_cast<uint16_t*>(vals + MD * CH_TREES);    // [NI][SM_WORDS]
    uint16_t* posl = pre + NI * SM_WORDS;                                 // [MD][CH_TREES] list position of (slot, tree)
    uint16_t* lmask = posl + MD * CH_TREES;                               // [MD * CH_TREES] expanded-edge masks (PRUNED)
    chunk_bitmap(dc, NI, chunk, p.batch, bits);
    for (uint32_t info = tid; info < NI; info += CH_THREADS) lcount[info] = list_prefix(bits, pre, info);
    __syncthreads();
    lds_exscan(lcount, lbase, NI, wave_tot);
    const uint32_t lt = tid, tree = chunk * CH_TREES + lt;  // CH_TREES == CH_THREADS: one tree per thread
    const uint32_t nd = tree < p.batch ? dc.ndec[tree] : 0u;
    for (uint32_t slot = 0; slot < nd; ++slot) {
        const uint32_t info = dc.info[slot * dc.stride + tree];
        const uint32_t pos = lbase[info] + list_rank(bits, pre, info, lt);
        posl[slot * CH_TREES + lt] = (uint16_t)pos;
        if (PRUNED) lmask[pos] = (uint16_t)dc.mask[slot * dc.stride + tree];
    }
    const float tf = (float)p.epoch;
    // chain phase: thread t owns infosets t, t + 256, ... (PASSES = 1 when the game has at most 256 infosets)
    uint32_t my_nact[PASSES], my_n[PASSES], my_base[PASSES];
#pragma unroll
    for (uint32_t q = 0; q < PASSES; ++q) {
        const uint32_t info = tid + q * CH_THREADS;
        const bool mine = info < NI && g.info_player[info < NI ? info : 0u] == p.walker;
        my_nact[q] = mine ? g.info_actions[info] : 0u;  // 0: not this walker's infoset
        my_n[q] = mine ? lcount[info] : 0u;
        my_base[q] = mine ? lbase[info] : 0u;
    }
    for (uint32_t c = 0; c <= W2; ++c) {  // regret cells, weight cells, then the payoff sum
        const bool isreg = c < A, ispay = c == W2;
        const uint32_t a = c % A;
        __syncthreads();  // the previous cell's chains are done with `vals`
        for (uint32_t slot = 0; slot < nd; ++slot) {
            float v;
            if (ispay) v = dc.payoff[slot * dc.stride + tree];
            else if (isreg) v = dc.regret[(slot * A + a) * dc.stride + tree];
            else v = weight_delta(p.W, dc.policy[(slot * A + a) * dc.stride + tree], tf);
            vals[posl[slot * CH_TREES + lt]] = v;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t q = 0; q < PASSES; ++q) {
            const uint32_t info = tid + q * CH_THREADS;
            if (!my_nact[q]) continue;
            const uint32_t n = my_n[q], base = my_base[q];
            const size_t out = bmap_index(chunk, g.info_rank[info], c, g.rank_max, W2);
            if (ispay) {  // payoff sum of the block, left fold from 0.0f
                float sum = 0.0f;
                for (uint32_t e = 0; e < n; ++e) sum += vals[base + e];
                bmaps[out] = map_sum_slot(sum, n);
                continue;
            }
            const bool chain = a < my_nact[q];
            const ChainParams cp = chain_params(p, isreg, tf);
            Map mp = map_identity();
            if (chain)
                for (uint32_t e = 0; e < n; ++e)
                    map_touch_unless(mp, PRUNED && isreg && !((lmask[base + e] >> a) & 1u), cp.d, vals[base + e], cp.fl);
            bmaps[out] = mp;
        }
    }
}

// The two-level fold of the block maps (include/rp_mi355x.h RP_FOLD_GROUP: the block maps of a cell composed sequentially
// inside groups of RP_FOLD_GROUP consecutive blocks, the group maps then in group order), spread over (group, infoset tile)
// workgroups, and — APPLY — the rest of the step with it.  The block maps are chunk-major (bmap_index), so nothing is transposed:
//   tiles    the walker's infosets in rank order, cut into the fewest runs of at most 256 / (2A + 1) whole infosets, balanced
//            (Leduc: 2 tiles of 30); lane = (infoset of the tile, slot), slot 2A the payoff sum and count;
//   stage 1  a lane walks the blocks of its group in block order: one 16-byte load per step, a wavefront's loads one contiguous
//            run; the loads do not depend on the chain and stay CB2_DEPTH ahead of it.  The group maps go to HBM with
//            agent-scope stores, laid out as the block maps are;
//   stage 2  the LAST group of a tile to finish (arrival counter; which one is timing, what it computes is not) folds the
//            tile's group maps in group order, same lanes, into the summary cell maps, payoff sum and count;
//   APPLY    single-GPU step: that workgroup also applies the summary to its infosets' table rows (k_fold with world = 1)
//            and refreshes their rows of the per-infoset tables the next traversal reads (k_prepare_infos): one launch
//            instead of three.  Otherwise it writes the summary blob (rp_mccfr_step_local).
// Cross-workgroup data is a few KB per group: agent-scope (sc1) stores + s_waitcnt before the arrival, agent-scope
// loads after it.  (A release FENCE at agent scope writes back a whole XCD's L2: tried on the block maps, 4x slower.)
// This hand-over is written against the gfx942 / gfx950 memory system, not against the portable memory model: relaxed agent-scope
// stores are sc1 write-through stores that `s_waitcnt vmcnt(0)` waits for (no separate store counter), relaxed agent-scope loads
// bypass the XCD's non-coherent lines.  On any other target the arrival counter would need release / acquire semantics:
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "k_combine2's cross-workgroup hand-over relies on gfx942/gfx950 store counting and sc1 semantics: use an acq_rel arrival counter on other targets"
#endif
__device__ __forceinline__ void st_agent(uint32_t* q, uint32_t v) { __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_map(Map* m, const Map& v) {
    uint32_t* w = reinterpret_cast<uint32_t*>(m);
    st_agent(w, rp_f2u(v.a));
    st_agent(w + 1, rp_f2u(v.b));
    st_agent(w + 2, rp_f2u(v.m));
    st_agent(w + 3, v.n);
}
#ifndef CB2_DEPTH
#define CB2_DEPTH 8u   // block maps per batch of a stage-1 chain: one batch composes while the loads of the next are in flight
#endif
#ifndef CB2_DEPTH2
#define CB2_DEPTH2 8u   // the same for the group maps of stage 2, two 8-byte agent-scope loads each: its one workgroup per tile is the
                       // serial tail of the launch, but deeper batches cost the registers that keep four workgroups on a CU
#endif
#define CB2_THREADS 256u
static_assert(2u * RP_MAX_ACTIONS + 1u <= CB2_THREADS, "a tile of k_combine2 holds at least one whole infoset");
// infosets per tile at most, and the number of tiles of a player with nr infosets
__host__ __device__ inline uint32_t cb2_tile_infos(uint32_t W2) { return CB2_THREADS / (W2 + 1u); }
__host__ __device__ inline uint32_t cb2_tiles(uint32_t nr, uint32_t W2) { return nr ? (nr + cb2_tile_infos(W2) - 1u) / cb2_tile_infos(W2) : 1u; }
struct FoldScratch {
    Map* gmaps;      // [group][rank][2A + 1]: bmap_index
    uint32_t* done;  // [tile] groups finished
};
// one lane's left fold, continued from m (the identity, or the fold of the slots before these), of the n >= 1 slots load(0), load(1),
// ... : cell maps composed, or — sum — payoff sums and counts added (from 0.0f / 0: the identity's b and n).  The loads do not depend
// on the chain: two batches of D, the loads of one in flight while the other is folded; the clamp keeps the loads of a ragged last
// batch inside the run.
template <uint32_t D, class Load>
__device__ __forceinline__ Map fold_slots(Map m, uint32_t n, bool sum, Load load) {
    uint4 va[D], vb[D];
    auto issue = [&](uint4* v, uint32_t k0) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t q = 0; q < D; ++q) v[q] = load(min(k0 + q, n - 1u));
    };
    auto fold = [&](const uint4* v, uint32_t k0) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t q = 0; q < D; ++q) {
            const Map s{rp_u2f(v[q].x), rp_u2f(v[q].y), rp_u2f(v[q].z), v[q].w};
            // the payoff lane runs the compose too and keeps nothing of it but the lock step: its a and m are never read
            const Map c = map_compose_select(m, s);
            const bool on = k0 + q < n;
            m.a = on ? c.a : m.a;
            m.b = on ? (sum ? m.b + s.b : c.b) : m.b;
            m.m = on ? c.m : m.m;
            m.n = on ? m.n + s.n : m.n;
        }
    };
    // every load below is issued unconditionally on its path and consumed on the same path: no loaded value is merged with an
    // older one at a join, where the copy would wait for the loads just issued
    uint32_t k0 = 0;
    issue(va, 0u);
    // (sched_barrier: the scheduler otherwise sinks a batch's loads below the fold they are meant to overlap)
    for (; k0 + 2u * D < n; k0 += 2u * D) {
        issue(vb, k0 + D);
        __builtin_amdgcn_sched_barrier(0);
        fold(va, k0);
        __builtin_amdgcn_sched_barrier(0);
        issue(va, k0 + 2u * D);
        __builtin_amdgcn_sched_barrier(0);
        fold(vb, k0 + D);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (k0 + D < n) {
        issue(vb, k0 + D);
        __builtin_amdgcn_sched_barrier(0);
        fold(va, k0);
        fold(vb, k0 + D);
    } else {
        fold(va, k0);
    }
    return m;
}
// the summary blob's entries of the other player's infosets, by one workgroup of CB2_THREADS: nothing happened to them
__device__ __forceinline__ void blob_idle_entries(const DevGame& g, const StepParams& p, Cell* cells, InfoSum* sums) {
    const uint32_t A = g.A, W2 = 2 * A, SL = W2 + 1u;
    const Map ident = map_identity();
    for (uint32_t e = threadIdx.x; e < g.n_infos * SL; e += CB2_THREADS) {
        const uint32_t info = e / SL, slot = e - info * SL;
        if (g.info_player[info] == p.walker) continue;
        if (slot == W2) {
            sums[info] = InfoSum{0u, 0.0f};
        } else {
            Cell& cl = cells[(size_t)info * A + slot % A];
            if (slot < A) cell_set_regret(cl, ident);
            else cell_set_weight(cl, ident);
        }
    }
}
// What follows the fold of the group maps, by every thread of the workgroup: lane (li, slot) of an `active` lane holds `tot`, the summary
// of its cell of infoset `info` (slot 2A: the payoff sum and count).  !APPLY: the lane's entry of the summary blob.  APPLY: k_fold with
// world = 1 for the rows of the workgroup's infosets, then their rows of the per-infoset tables (prepare_one).  sh_ps / sh_len: one
// entry per infoset of the workgroup.
template <bool APPLY>
__device__ __forceinline__ void fold_finish(const DevGame& g, const DevTables& t, const DevInfoTab& it, const StepParams& p, bool active, uint32_t li,
                                            uint32_t slot, uint32_t info, const Map& tot, Cell* cells, InfoSum* sums, float* sh_ps, uint32_t* sh_len) {
    const uint32_t A = g.A, W2 = 2 * A;
    const bool sum = slot == W2;
    if (!APPLY) {
        if (active) {
            if (sum) {
                sums[info] = InfoSum{tot.n, tot.b};
            } else {
                Cell& cl = cells[(size_t)info * A + slot % A];
                if (slot < A) cell_set_regret(cl, tot);
                else cell_set_weight(cl, tot);
            }
        }
        return;
    }
    if (active && sum) {
        sh_ps[li] = tot.b;
        sh_len[li] = tot.n;
    }
    __syncthreads();
    if (active && !sum && slot % A < g.info_actions[info]) {
        const uint32_t cell = info * A + slot % A;
        if (slot < A) {
            t.regret[cell] = map_apply(tot, t.regret[cell]);
            float ev = t.payoff[cell];
            uint32_t visits = t.visits[cell];
            fold_payoff(ev, visits, sh_ps[li], sh_len[li]);
            t.payoff[cell] = ev;
            t.visits[cell] = visits;
        } else {
            t.weight[cell] = map_apply(tot, t.weight[cell]);
        }
    }
    __syncthreads();  // workgroup scope: the rows just written are what prepare_one reads
    if (active && slot == 0) prepare_one(g, t, p, it, info);
}
// TAIL: stages 1 and 2 and what follows, in one launch, as described above.  !TAIL (then !APPLY): stage 1 alone, the group maps stored
// plainly, no arrival counter; k_fold_groups<APPLY>, the next launch on the stream, is stage 2 and what follows.
template <bool APPLY, bool TAIL = true>
__global__ __launch_bounds__(CB2_THREADS) void k_combine2(DevGame g, DevTables t, DevInfoTab it, StepParams p, const Map* bmaps, uint32_t nr,
                                                          FoldScratch fs, Cell* cells, InfoSum* sums) {
    static_assert(TAIL || !APPLY, "stage 1 alone applies nothing");
    __shared__ uint32_t role;
    __shared__ float sh_ps[CB2_THREADS / 3u];
    __shared__ uint32_t sh_len[CB2_THREADS / 3u];
    const uint32_t grp = blockIdx.x, tile = blockIdx.y, tid = threadIdx.x;
    const uint32_t A = g.A, W2 = 2 * A, SL = W2 + 1u;
    if (TAIL && !APPLY && grp == 0 && tile == 0) blob_idle_entries(g, p, cells, sums);
    const uint32_t nb = (p.batch + RP_COMPOSE_CHUNK - 1) / RP_COMPOSE_CHUNK;  // one block per chunk of trees
    const uint32_t ngrp = (nb + RP_FOLD_GROUP - 1) / RP_FOLD_GROUP;
    if (grp >= ngrp) return;
    const uint32_t ntiles = cb2_tiles(nr, W2);
    const uint32_t r_lo = (uint32_t)((uint64_t)tile * nr / ntiles), r_hi = (uint32_t)((uint64_t)(tile + 1u) * nr / ntiles);
    const uint32_t li = tid / SL, slot = tid - li * SL, rank = r_lo + li;
    const bool active = rank < r_hi, sum = slot == W2;
    const size_t row = (size_t)g.rank_max * SL;  // 16-byte words from a block's (group's) row to the next
    if (active) {
        const uint32_t b_lo = grp * RP_FOLD_GROUP, n = min(nb, b_lo + RP_FOLD_GROUP) - b_lo;
        const uint4* src = reinterpret_cast<const uint4*>(bmaps) + bmap_index(b_lo, rank, slot, g.rank_max, W2);
        const Map m = fold_slots<CB2_DEPTH>(map_identity(), n, sum, [&](uint32_t k) { return src[(size_t)k * row]; });
        if (TAIL) st_map(&fs.gmaps[bmap_index(grp, rank, slot, g.rank_max, W2)], m);
        else fs.gmaps[bmap_index(grp, rank, slot, g.rank_max, W2)] = m;
    }
    if (!TAIL) return;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the group maps are in memory before this group counts itself in
    __syncthreads();
    if (tid == 0) role = atomicAdd(&fs.done[tile], 1u) == ngrp - 1u ? 1u : 0u;
    __syncthreads();
    if (!role) return;
    if (tid == 0) fs.done[tile] = 0;  // for the next launch
    // the tile's group maps, folded in group order
    Map tot = map_identity();
    uint32_t info = 0;
    if (active) {
        const uint64_t* gm = reinterpret_cast<const uint64_t*>(fs.gmaps + bmap_index(0u, rank, slot, g.rank_max, W2));
        tot = fold_slots<CB2_DEPTH2>(tot, ngrp, sum, [&](uint32_t k) {
            const uint64_t* w = gm + (size_t)k * row * 2u;
            const uint64_t lo = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t hi = __hip_atomic_load(w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
        });
        info = g.rank_info[(size_t)p.walker * g.rank_max + rank];
    }
    fold_finish<APPLY>(g, t, it, p, active, li, slot, info, tot, cells, sums, sh_ps, sh_len);
}

// Stage 2 and what follows as a launch of its own, after k_combine2<false, false> on the same stream (the kernel boundary orders the
// group maps: plain loads, no counter, no hand-over): one workgroup per infoset of the walker, in rank order.
//   load    the infoset's group maps — ngrp x (2A + 1) slots, 2A + 1 contiguous per group — by all lanes, FG_LOADS 16-byte loads per
//           lane, every one issued before the first is waited for: one memory round trip, where the tail of k_combine2 pulls a whole
//           tile's maps through one CU eight at a time;
//   stage   into LDS in group order: FG_SLOTS slots = FG_SLOTS * 16 B = 40 KB of static LDS, 60.3 KB with the 20 KB of compacted
//           operands of a unit slab, below (two workgroups fit a CU's 160 KB; the grid needs one per CU).  A slab is the
//           FG_SLOTS / (2A + 1) whole groups that fit (Leduc: 512, i.e. 2^23 trees); more groups take further slabs in group order,
//           the running maps carried across;
//   fold    lanes 0 .. 2A continue their slot's left fold through the slab in group order out of LDS: a unit slab (below) compacted
//           and by fold_unit_ops, any other by fold_slots (the association and the payoff-lane rule of k_combine2's stage 2); the
//           reads FG_DEPTH ahead of the dependent chain in both;
//   finish  fold_finish, as the last workgroup of a tile does in k_combine2.
// Unit slabs.  With unit discounts (Summed / Floored regret, Constant / Linear / Quadratic weight: chain_params) every map has
// a == 1.0f, and a step of the fold needs two dependent operations where map_compose_select spends six.  A slab is `unit` when every
// non-empty map (n != 0) of its cell slots, and every non-empty running map carried into it, has a == 1.0f bitwise, a finite b and an m
// that is not NaN.  The workgroup decides that once per slab, from the data, for all its cells together (a wavefront with lanes of both
// kinds would run both loops one after the other); a slab that is not unit is folded by fold_slots as before.  For a unit slab
//   compact  wavefront w packs the (b, m) of the non-empty maps of cell slots w, w + 4, ... in group order into LDS (ballot + popcount
//            per 64 groups) and sums their counts: the chain meets no empty map, and the counts are off it;
//   chain    lane `slot` folds its operands with fold_unit_ops, the reads FG_DEPTH ahead;
//   payoff   a lane of the last wavefront adds the b and n of EVERY group's payoff slot in group order, from the carried sum:
//            fold_slots' payoff-lane rule, beside the cell chains instead of in lock step with them.
// The bits are those of fold_slots (map_compose_select) on the same slots:
//   - an empty map is skipped and an empty running map becomes the first non-empty one: map_compose's first two lines;
//   - x * 1.0f == x for every float, so with a == 1.0f on both sides map_compose_touched gives a' = 1.0f, b' = first.b + second.b
//     and t = first.m + second.b: fold_unit_ops' operations on the same operands in the same order;
//   - the one other difference is map_compose_touched's test for first.m == -inf, and with second.b finite -inf + second.b is -inf,
//     the bits of first.m;
//   - every b is finite and no m is NaN, so the running m never becomes NaN (+-inf + finite == +-inf; an overflowing running b is
//     +-inf on both paths): rp_maxf never has a NaN to drop.
// So the two differ only on operands that the test sends to fold_slots.
typedef float __attribute__((ext_vector_type(2))) FgOp;  // (b, m) of a compacted operand (a plain vector, as Word4 below)
__device__ __forceinline__ bool unit_operand(uint32_t a, uint32_t b, uint32_t m) {
    return a == 0x3f800000u && (b & 0x7f800000u) != 0x7f800000u && (m & 0x7fffffffu) <= 0x7f800000u;
}
// one lane's left fold, continued from `tot`, of the cnt compacted operands (b, m) at op[0 .. cnt) of a unit slab; nsum: the sum of
// their counts.  Two batches of D as in fold_slots, but whole batches only: the ragged rest has a loop of its own.
template <uint32_t D>
__device__ __forceinline__ void fold_unit_ops(Map& tot, const FgOp* op, uint32_t cnt, uint32_t nsum) {
    float B = tot.b, M = tot.m;
    uint32_t k = 0;
    if (tot.n == 0 && cnt) {  // map_compose: first.n == 0
        B = op[0].x;
        M = op[0].y;
        k = 1;
    }
    FgOp va[D], vb[D];
    auto issue = [&](FgOp* v, uint32_t k0) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t q = 0; q < D; ++q) v[q] = op[k0 + q];
    };
    auto fold = [&](const FgOp* v) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t q = 0; q < D; ++q) {
            B = B + v[q].x;
            M = rp_maxf(M + v[q].x, v[q].y);
        }
    };
    if (k + D <= cnt) {
        issue(va, k);
        for (; k + 3u * D <= cnt; k += 2u * D) {
            issue(vb, k + D);
            __builtin_amdgcn_sched_barrier(0);
            fold(va);
            __builtin_amdgcn_sched_barrier(0);
            issue(va, k + 2u * D);
            __builtin_amdgcn_sched_barrier(0);
            fold(vb);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (k + 2u * D <= cnt) {
            issue(vb, k + D);
            __builtin_amdgcn_sched_barrier(0);
            fold(va);
            fold(vb);
            k += 2u * D;
        } else {
            fold(va);
            k += D;
        }
    }
    for (; k < cnt; ++k) {
        const FgOp v = op[k];
        B = B + v.x;
        M = rp_maxf(M + v.x, v.y);
    }
    tot.b = B;
    tot.m = M;
    tot.n += nsum;
}
#define FG_LOADS 10u
#define FG_SLOTS (FG_LOADS * CB2_THREADS)
#define FG_DEPTH 8u
#define FG_WAVES (CB2_THREADS / 64u)
#define FG_PAY_LANE (CB2_THREADS - 64u)  // the payoff lane of a unit slab: a wavefront of its own beside the cell lanes 0 .. 2A - 1
static_assert(2u * RP_MAX_ACTIONS + 1u <= FG_SLOTS, "a slab of k_fold_groups holds at least one group");
static_assert(2u * RP_MAX_ACTIONS <= FG_PAY_LANE, "the cell lanes of k_fold_groups end before its payoff lane's wavefront");
__host__ __device__ inline uint32_t fg_slab_groups(uint32_t W2) { return FG_SLOTS / (W2 + 1u); }
template <bool APPLY>
__global__ __launch_bounds__(CB2_THREADS) void k_fold_groups(DevGame g, DevTables t, DevInfoTab it, StepParams p, const Map* gmaps, uint32_t nr,
                                                             Cell* cells, InfoSum* sums) {
    typedef uint32_t __attribute__((ext_vector_type(4))) Word4;  // (a plain vector: an array of uint4 in flight ends up in scratch)
    __shared__ __attribute__((aligned(16))) Word4 slab[FG_SLOTS];
    __shared__ __attribute__((aligned(8))) FgOp ops[FG_SLOTS];  // unit slab: [cell slot][operand], n per slot (n * 2A < FG_SLOTS)
    __shared__ uint32_t op_cnt[2u * RP_MAX_ACTIONS], op_n[2u * RP_MAX_ACTIONS];  // operands of a cell slot, and the sum of their counts
    __shared__ uint32_t sh_general[FG_WAVES];
    __shared__ float pay_b;
    __shared__ uint32_t pay_n;
    __shared__ float sh_ps[1];
    __shared__ uint32_t sh_len[1];
    const uint32_t rank = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t A = g.A, W2 = 2 * A, SL = W2 + 1u;
    if (!APPLY && rank == 0) blob_idle_entries(g, p, cells, sums);
    if (rank >= nr) return;
    const uint32_t nb = (p.batch + RP_COMPOSE_CHUNK - 1) / RP_COMPOSE_CHUNK;
    const uint32_t ngrp = (nb + RP_FOLD_GROUP - 1) / RP_FOLD_GROUP, per = fg_slab_groups(W2);
    const size_t row = (size_t)g.rank_max * SL;
    const Word4* src = reinterpret_cast<const Word4*>(gmaps) + bmap_index(0u, rank, 0u, g.rank_max, W2);
    const bool active = tid < SL;
    Map tot = map_identity();
    for (uint32_t g0 = 0; g0 < ngrp; g0 += per) {
        const uint32_t n = min(per, ngrp - g0), nel = n * SL;  // 1 <= nel <= FG_SLOTS
        Word4 v[FG_LOADS];
        uint32_t vslot[FG_LOADS];
#pragma unroll
        for (uint32_t q = 0; q < FG_LOADS; ++q) {  // the clamp keeps the loads of a ragged slab inside it: no branch between the loads
            const uint32_t e = min(tid + q * CB2_THREADS, nel - 1u), k = e / SL;
            vslot[q] = e - k * SL;
            v[q] = src[(size_t)(g0 + k) * row + vslot[q]];
        }
        if (g0) __syncthreads();  // the fold of the slab before is done with the LDS
        // is the slab unit?  A lane tests the maps it stages (a clamped load repeats the slab's last map: tested twice) and its running map
        bool general = tid < W2 && tot.n != 0u && !unit_operand(rp_f2u(tot.a), rp_f2u(tot.b), rp_f2u(tot.m));
#pragma unroll
        for (uint32_t q = 0; q < FG_LOADS; ++q) {
            const uint32_t e = tid + q * CB2_THREADS;
            if (e < nel) slab[e] = v[q];
            general |= vslot[q] != W2 && v[q].w != 0u && !unit_operand(v[q].x, v[q].y, v[q].z);
        }
        const bool wave_general = __ballot(general) != 0ull;
        if (lane == 0) sh_general[wave] = wave_general ? 1u : 0u;
        __syncthreads();
        uint32_t any_general = 0;
#pragma unroll
        for (uint32_t w = 0; w < FG_WAVES; ++w) any_general |= sh_general[w];
        if (__builtin_amdgcn_readfirstlane(any_general)) {  // the same for the whole workgroup
            if (active) tot = fold_slots<FG_DEPTH>(tot, n, tid == W2, [&](uint32_t k) {
                const Word4 w = slab[k * SL + tid];
                return make_uint4(w.x, w.y, w.z, w.w);
            });
            continue;
        }
        for (uint32_t s = wave; s < W2; s += FG_WAVES) {  // compact
            uint32_t base = 0, nsum = 0;
            for (uint32_t k0 = 0; k0 < n; k0 += 64u) {
                const uint32_t k = k0 + lane;
                const Word4 w = slab[min(k, n - 1u) * SL + s];
                const bool on = k < n && w.w != 0u;
                const uint64_t mask = __ballot(on);
                if (on) {
                    const uint32_t at = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                    ops[s * n + at] = FgOp{rp_u2f(w.y), rp_u2f(w.z)};
                    nsum += w.w;
                }
                base += (uint32_t)__popcll(mask);
            }
            for (int d = 32; d > 0; d >>= 1) nsum += __shfl_xor(nsum, d, 64);
            if (lane == 0) {
                op_cnt[s] = base;
                op_n[s] = nsum;
            }
        }
        if (tid == W2) {  // the carried payoff sum and count, handed to the payoff lane
            pay_b = tot.b;
            pay_n = tot.n;
        }
        __syncthreads();
        if (tid < W2) fold_unit_ops<FG_DEPTH>(tot, ops + tid * n, op_cnt[tid], op_n[tid]);
        if (tid == FG_PAY_LANE) {
            float b = pay_b;
            uint32_t cn = pay_n;
#pragma unroll 8
            for (uint32_t k = 0; k < n; ++k) {
                const Word4 w = slab[k * SL + W2];
                b += rp_u2f(w.y);
                cn += w.w;
            }
            pay_b = b;
            pay_n = cn;
        }
        __syncthreads();
        if (tid == W2) {
            tot.b = pay_b;
            tot.n = pay_n;
        }
    }
    const uint32_t info = g.rank_info[(size_t)p.walker * g.rank_max + rank];
    fold_finish<APPLY>(g, t, it, p, active, 0u, tid, info, tot, cells, sums, sh_ps, sh_len);
}

// ------------------------------------------------------------------------------------------------
// k_fold: the receiving side of the multi-GPU exchange (oracle: ora_mccfr_step_apply)
// ------------------------------------------------------------------------------------------------
// one thread per table cell; `blob` holds `world` summaries back to back: [cells][sums]
__global__ void k_fold(DevGame g, DevTables t, const unsigned char* blob, size_t blob_stride, uint32_t world) {
    const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t ncell = g.n_infos * g.A;
    if (cell >= ncell) return;
    const uint32_t info = cell / g.A, a = cell % g.A;
    if (a >= g.info_actions[info]) return;
    float r = t.regret[cell], w = t.weight[cell], ev = t.payoff[cell];
    uint32_t visits = t.visits[cell];
    for (uint32_t rk = 0; rk < world; ++rk) {
        const unsigned char* b = blob + (size_t)rk * blob_stride;
        const Cell c = reinterpret_cast<const Cell*>(b)[cell];
        const InfoSum s = reinterpret_cast<const InfoSum*>(b + (size_t)ncell * sizeof(Cell))[info];
        if (c.rn) r = map_eval(cell_regret(c), r);  // map_apply, its test here: the Cell's fields are then loaded only when used
        if (c.wn) w = map_eval(cell_weight(c), w);
        fold_payoff(ev, visits, s.psum, s.count);
    }
    t.regret[cell] = r;
    t.weight[cell] = w;
    t.payoff[cell] = ev;
    t.visits[cell] = visits;
}

// the exchange window (rp_mccfr_window_local): acc <- step o acc per table cell — the maps of consecutive local
// steps composed in step order, touch counts, payoff sums and visit counts added (oracle: ora_mccfr_window_accumulate)
__global__ void k_accumulate(DevGame g, unsigned char* acc, const unsigned char* step, uint32_t first) {
    const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t ncell = g.n_infos * g.A;
    if (cell >= ncell) return;
    const Cell s = reinterpret_cast<const Cell*>(step)[cell];
    Cell* ac = reinterpret_cast<Cell*>(acc) + cell;
    if (first) {
        *ac = s;
    } else {
        const Cell a = *ac;
        const Map r = map_compose(cell_regret(a), cell_regret(s));
        const Map w = map_compose(cell_weight(a), cell_weight(s));
        *ac = Cell{r.a, r.b, r.m, w.a, w.b, w.m, r.n, w.n};
    }
    if (cell % g.A == 0) {
        const uint32_t info = cell / g.A;
        const InfoSum si = reinterpret_cast<const InfoSum*>(step + (size_t)ncell * sizeof(Cell))[info];
        InfoSum* ai = reinterpret_cast<InfoSum*>(acc + (size_t)ncell * sizeof(Cell)) + info;
        if (first) *ai = si;
        else *ai = InfoSum{ai->count + si.count, ai->psum + si.psum};
    }
}

}  // namespace rp

#endif
