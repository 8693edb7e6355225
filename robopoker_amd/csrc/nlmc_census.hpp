// nlmc_census.hpp — the blueprint census: one read-only scan of the device-resident NLHE table into an rp_census record
// (rp_nlhe_table_census; the contract is the header's THE BLUEPRINT CENSUS).
//
// Reference: TrainingAPI::stats / street_stats / cold / hot / saturation (portal/src/training/api.rs:74-286) and
// StrategyAPI::grid_usage (portal/src/strategy/api.rs:196-245): full scans of the blueprint table with a GROUP BY.
//
// The contract fixes the float order — a left fold in slot order inside a segment of 65 536 slots, then a left fold of the segment
// sums — so that the kernel below is the natural one:
//   k_nl_census_scan  one workgroup of THREE WAVEFRONTS per segment.  64 slots at a time: wavefront 0 loads the 32-byte slots (one
//                     coalesced load), ballots the ready ones and stages their keys in LDS; all 192 lanes then stage the ready slots'
//                     rows in 16-byte pieces, consecutive lanes consecutive pieces (an empty slot's row is never touched).  Every
//                     wavefront walks the ready slots in ascending order with LANES OWNING CELLS: cell (street, code) belongs to
//                     wavefront street >> 1, lane (street & 1) * 32 + code, so every sum is a register-resident sequential fold —
//                     no atomics, no shuffles in the sum path, and two actions with one edge code are two turns of one lane.  A
//                     wavefront passes over the infosets of the other wavefronts' streets after reading their key.  Wavefront 2 —
//                     its cells are street 4's, which a table of real abstractions leaves empty — also counts the infosets and
//                     keeps the ranked lists, one entry per lane in rank order: a candidate's place is a ballot of the lanes that
//                     rank behind it, its insertion a shuffle-up.  The workgroup stores one partial: its cells, counts and lists.
//                     (One wavefront with three accumulator sets per lane, the first version, took 256 VGPRs and 47 AGPRs.)
//   k_nl_census_fold  folds the partials in ascending segment order, one lane per cell, and merges the lists (one wavefront each);
//                     writes every byte of the record.
#ifndef RP_NLMC_CENSUS_HPP
#define RP_NLMC_CENSUS_HPP

#include "nlmc_query.hpp"

namespace rp {

#define NC_CELLS (RP_NLHE_CENSUS_STREETS * RP_NLHE_CENSUS_CODES)  // 160
#define NC_TOP RP_NLHE_CENSUS_TOP
#define NC_SCAN_BLOCK 192u  // k_nl_census_scan: three wavefronts, one per pair of streets
static_assert(NC_TOP == 64u, "a ranked list is one entry per lane of a wavefront");
static_assert(RP_NLHE_CENSUS_SEGMENT % 64u == 0, "a segment is walked 64 slots at a time");

// the scratch of a scan over nseg segments: cells cell-major (the fold's lane reads its cell's partials contiguously), the rest
// segment-major.  A list entry of a partial keeps its rank key in `visits`; a hot entry its value, MAX(regret), in `regret` (a cold
// entry's value is its key).
struct NcPartials {
    rp_census_cell* cells;     // [NC_CELLS][nseg]
    uint64_t* infosets;        // [nseg][5]
    rp_census_entry* lists;    // [nseg][2][NC_TOP]: cold, hot
    uint32_t* counts;          // [nseg][2]
};
inline size_t nc_partial_bytes(uint32_t nseg) {
    return (size_t)nseg * (NC_CELLS * sizeof(rp_census_cell) + 5 * 8 + 2 * NC_TOP * sizeof(rp_census_entry) + 2 * 4);
}
inline NcPartials nc_partials(void* base, uint32_t nseg) {
    NcPartials p;
    unsigned char* b = reinterpret_cast<unsigned char*>(base);
    p.cells = reinterpret_cast<rp_census_cell*>(b);
    b += (size_t)nseg * NC_CELLS * sizeof(rp_census_cell);
    p.infosets = reinterpret_cast<uint64_t*>(b);
    b += (size_t)nseg * 5 * 8;
    p.lists = reinterpret_cast<rp_census_entry*>(b);
    b += (size_t)nseg * 2 * NC_TOP * sizeof(rp_census_entry);
    p.counts = reinterpret_cast<uint32_t*>(b);
    return p;
}

__device__ __forceinline__ uint32_t nc_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// one cell's accumulators, in the registers of the lane that owns the cell
struct NcAcc {
    uint64_t rows, rated, dominant, visits;
    double ratio, weight, total, regret, payoff;
    float max_regret, min_regret, max_weight, max_payoff, min_payoff;
    uint32_t max_visits, min_visits;
};
__device__ __forceinline__ void nc_clear(NcAcc& c) {
    c.rows = c.rated = c.dominant = c.visits = 0;
    c.ratio = c.weight = c.total = c.regret = c.payoff = 0.0;
    c.max_regret = c.min_regret = c.max_weight = c.max_payoff = c.min_payoff = 0.0f;
    c.max_visits = c.min_visits = 0;
}
// one row of the SQL table into its cell
__device__ __forceinline__ void nc_add(NcAcc& c, float w, float r, float p, uint32_t v, float dec_total, bool rated, float ratio) {
    if (c.rows == 0) {
        c.max_regret = c.min_regret = r;
        c.max_weight = w;
        c.max_payoff = c.min_payoff = p;
        c.max_visits = c.min_visits = v;
    } else {
        c.max_regret = r > c.max_regret ? r : c.max_regret;
        c.min_regret = r < c.min_regret ? r : c.min_regret;
        c.max_weight = w > c.max_weight ? w : c.max_weight;
        c.max_payoff = p > c.max_payoff ? p : c.max_payoff;
        c.min_payoff = p < c.min_payoff ? p : c.min_payoff;
        c.max_visits = v > c.max_visits ? v : c.max_visits;
        c.min_visits = v < c.min_visits ? v : c.min_visits;
    }
    c.rows += 1;
    if (rated) {
        c.rated += 1;
        c.dominant += ratio > 0.5f ? 1u : 0u;
        c.ratio = c.ratio + (double)ratio;
    }
    c.visits += v;
    c.weight = c.weight + (double)w;
    c.total = c.total + (double)dec_total;
    c.regret = c.regret + (double)r;
    c.payoff = c.payoff + (double)p;
}
__device__ __forceinline__ void nc_store(rp_census_cell* o, const NcAcc& c) {
    o->rows = c.rows; o->rated = c.rated; o->dominant = c.dominant; o->visits = c.visits;
    o->ratio = c.ratio; o->weight = c.weight; o->total = c.total; o->regret = c.regret; o->payoff = c.payoff;
    o->max_regret = c.max_regret; o->min_regret = c.min_regret; o->max_weight = c.max_weight;
    o->max_payoff = c.max_payoff; o->min_payoff = c.min_payoff;
    o->max_visits = c.max_visits; o->min_visits = c.min_visits;
    o->reserved = 0;
}

// A ranked list: lane l holds the entry of rank l, `n` of them (wave-uniform).  Entries rank by (key, past, present, choices)
// ascending, all unsigned: cold key = MIN(visits); hot key = ~bits(MAX(ABS(regret))) — the bits of a non-negative float order as
// its values do.  Keys of a table are distinct, so the order is total and the merged list does not depend on the order of insertion.
struct NcList {
    uint64_t past, choices;
    uint32_t present, edges, key, val;
    uint32_t n;
};
__device__ __forceinline__ void nc_list_clear(NcList& l) {
    l.past = l.choices = 0;
    l.present = l.edges = l.key = l.val = 0;
    l.n = 0;
}
// the candidate (wave-uniform arguments) goes in front of the first entry that ranks behind it; the last entry of a full list drops
// out.  Called by the whole wavefront.  Returns whether the candidate went in.
__device__ __forceinline__ bool nc_list_insert(NcList& l, uint32_t lane, uint64_t past, uint64_t choices, uint32_t present, uint32_t edges,
                                               uint32_t key, uint32_t val) {
    const bool behind = lane >= l.n || l.key > key ||
                        (l.key == key && (l.past > past || (l.past == past && (l.present > present || (l.present == present && l.choices > choices)))));
    const uint64_t m = __ballot(behind);
    if (m == 0) return false;
    const uint32_t pos = (uint32_t)__ffsll((long long)m) - 1u;
    const uint64_t up_past = __shfl_up(l.past, 1), up_choices = __shfl_up(l.choices, 1);
    const uint32_t up_present = __shfl_up(l.present, 1), up_edges = __shfl_up(l.edges, 1), up_key = __shfl_up(l.key, 1), up_val = __shfl_up(l.val, 1);
    if (lane > pos) {
        l.past = up_past; l.choices = up_choices; l.present = up_present; l.edges = up_edges; l.key = up_key; l.val = up_val;
    } else if (lane == pos) {
        l.past = past; l.choices = choices; l.present = present; l.edges = edges; l.key = key; l.val = val;
    }
    l.n = l.n < NC_TOP ? l.n + 1u : NC_TOP;
    return true;
}

__global__ __launch_bounds__(NC_SCAN_BLOCK) void k_nl_census_scan(NlTable t, uint32_t nseg, NcPartials part) {
    __shared__ uint4 s_key[64][2];   // the ready slots of the 64 in hand
    __shared__ float4 s_row[64][9];  // and their rows: regret[9] weight[9] payoff[9] visits[9]
    __shared__ uint32_t s_mask[2][2];  // the ballot of the ready ones, two words, of the even and of the odd 64
    const uint32_t lane = threadIdx.x & 63u, wave = nc_uniform(threadIdx.x >> 6);
    const bool lists = wave == 2u;
    const uint64_t slots = (uint64_t)t.mask + 1u;
    for (uint32_t seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        const uint64_t seg_lo = (uint64_t)seg * RP_NLHE_CENSUS_SEGMENT;
        const uint32_t seg_n = (uint32_t)(slots - seg_lo < RP_NLHE_CENSUS_SEGMENT ? slots - seg_lo : RP_NLHE_CENSUS_SEGMENT);  // a multiple of 64: slots >= 256
        NcAcc acc;
        nc_clear(acc);
        NcList cold, hot;
        nc_list_clear(cold); nc_list_clear(hot);
        uint64_t infosets = 0;  // of street `lane`, lanes 0..4 of wavefront 2
        for (uint32_t base = 0; base < seg_n; base += 64u) {
            const uint32_t par = (base >> 6) & 1u;
            if (wave == 0u) {
                const uint4* sl = reinterpret_cast<const uint4*>(t.slots + (seg_lo + base + lane));
                const uint4 lo = sl[0], hi = sl[1];
                const bool ready = hi.z == 2u;
                const uint64_t b = __ballot(ready);
                if (ready) {
                    s_key[lane][0] = lo;
                    s_key[lane][1] = hi;
                }
                if (lane == 0) {
                    s_mask[par][0] = (uint32_t)b;
                    s_mask[par][1] = (uint32_t)(b >> 32);
                }
            }
            __syncthreads();
            const uint64_t mask = (uint64_t)nc_uniform(s_mask[par][0]) | ((uint64_t)nc_uniform(s_mask[par][1]) << 32);
            // 64 empty slots: on to the next 64 without the two barriers below.  Wavefront 0 then writes the OTHER pair of mask words
            // while the others may still be reading this one, and this one again only behind the next barrier above.
            if (mask == 0) continue;  // the same in every lane of the workgroup
            const float4* rw = reinterpret_cast<const float4*>(t.rows + (size_t)(seg_lo + base) * 4u * NLMC_A);
#pragma unroll
            for (uint32_t k = 0; k < 3u; ++k) {  // 64 rows of 9 pieces over 192 lanes
                const uint32_t piece = k * NC_SCAN_BLOCK + threadIdx.x, j = piece / 9u;
                if ((mask >> j) & 1ull) s_row[j][piece - j * 9u] = rw[piece];
            }
            __syncthreads();
            for (uint64_t m = mask; m != 0; m &= m - 1) {
                const uint32_t j = (uint32_t)__ffsll((long long)m) - 1u;
                const uint32_t present = nc_uniform(s_key[j][1].x);
                const uint32_t street = (present >> 8) < 4u ? (present >> 8) : 4u;
                if ((street >> 1) != wave && !lists) continue;
                const uint4 klo = s_key[j][0];
                const uint32_t c0 = nc_uniform(klo.z), c1 = nc_uniform(klo.w);
                const uint64_t past = (uint64_t)klo.x | ((uint64_t)klo.y << 32), choices = (uint64_t)c0 | ((uint64_t)c1 << 32);
                const uint32_t nch = nlq_nch(choices);
                if (nch == 0) continue;  // no row of the SQL table
                const float* rf = reinterpret_cast<const float*>(&s_row[j][0]);
                const uint32_t* ru = reinterpret_cast<const uint32_t*>(&s_row[j][0]);
                if ((street >> 1) == wave) {
                    float dec_total = 0.0f;
                    for (uint32_t a = 0; a < nch; ++a) dec_total = dec_total + rf[NLMC_A + a];
                    const bool rated = dec_total != 0.0f;
                    // the actions whose cell this lane owns, as a bit mask: every lane takes its own action in the same turn, so an
                    // infoset is ONE turn of nc_add unless it holds an edge code twice — then the code's lane takes its actions in
                    // ascending order, one per turn
                    const uint32_t mine = lane - (street & 1u) * 32u;  // this lane's edge code in the street; 32 or more: none
                    uint32_t todo = 0;
                    for (uint32_t a = 0; a < nch; ++a) todo |= (((uint32_t)(choices >> (5u * a)) & 31u) == mine ? 1u : 0u) << a;
                    while (__any(todo != 0)) {
                        if (todo != 0) {
                            const uint32_t a = (uint32_t)__ffs((int)todo) - 1u;
                            const float w = rf[NLMC_A + a];
                            nc_add(acc, w, rf[a], rf[2u * NLMC_A + a], ru[3u * NLMC_A + a], dec_total, rated, rated ? w / dec_total : 0.0f);
                            todo &= todo - 1u;
                        }
                    }
                }
                if (lists) {
                    uint32_t min_v = 0xffffffffu;
                    float max_r = rf[0], max_abs = 0.0f;
                    for (uint32_t a = 0; a < nch; ++a) {
                        const float r = rf[a], ar = fabsf(r);
                        const uint32_t v = ru[3u * NLMC_A + a];
                        min_v = v < min_v ? v : min_v;
                        max_r = r > max_r ? r : max_r;
                        max_abs = ar > max_abs ? ar : max_abs;
                    }
                    if (lane == street) infosets += 1;
                    (void)nc_list_insert(cold, lane, past, choices, present, nch, min_v, min_v);
                    (void)nc_list_insert(hot, lane, past, choices, present, nch, ~__float_as_uint(max_abs), __float_as_uint(max_r));
                }
            }
            __syncthreads();  // wavefront 0 overwrites the keys next
        }
        // the partial of this segment
        {
            const uint32_t cell = wave * 64u + lane;
            if (cell < NC_CELLS) nc_store(part.cells + (size_t)cell * nseg + seg, acc);
        }
        if (!lists) continue;
        if (lane < 5u) part.infosets[(size_t)seg * 5u + lane] = infosets;
        rp_census_entry ec, eh;
        const bool lc = lane < cold.n, lh = lane < hot.n;
        ec.past = lc ? cold.past : 0; ec.choices = lc ? cold.choices : 0; ec.present = lc ? cold.present : 0; ec.edges = lc ? cold.edges : 0;
        ec.visits = lc ? cold.key : 0; ec.regret = 0.0f;  // the cold list's value is its key: no integer travels through a float
        eh.past = lh ? hot.past : 0; eh.choices = lh ? hot.choices : 0; eh.present = lh ? hot.present : 0; eh.edges = lh ? hot.edges : 0;
        eh.visits = lh ? hot.key : 0; eh.regret = __uint_as_float(lh ? hot.val : 0u);
        part.lists[((size_t)seg * 2u + 0u) * NC_TOP + lane] = ec;
        part.lists[((size_t)seg * 2u + 1u) * NC_TOP + lane] = eh;
        if (lane == 0) {
            part.counts[(size_t)seg * 2u + 0u] = cold.n;
            part.counts[(size_t)seg * 2u + 1u] = hot.n;
        }
    }
}

// workgroups 0..2: one lane per cell, the partials in ascending segment order; 3: the cold list, the infoset counts, epoch and slots;
// 4: the hot list.  64 lanes each.
__global__ __launch_bounds__(64) void k_nl_census_fold(NcPartials part, uint32_t nseg, uint64_t epoch, uint64_t slots, rp_census* out) {
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x < 3u) {
        const uint32_t cell = blockIdx.x * 64u + lane;
        if (cell >= NC_CELLS) return;
        NcAcc c;
        nc_clear(c);
        const rp_census_cell* p = part.cells + (size_t)cell * nseg;
        for (uint32_t s = 0; s < nseg; ++s) {
            const rp_census_cell q = p[s];
            c.ratio = c.ratio + q.ratio;
            c.weight = c.weight + q.weight;
            c.total = c.total + q.total;
            c.regret = c.regret + q.regret;
            c.payoff = c.payoff + q.payoff;
            if (q.rows == 0) continue;
            if (c.rows == 0) {
                c.max_regret = q.max_regret; c.min_regret = q.min_regret; c.max_weight = q.max_weight;
                c.max_payoff = q.max_payoff; c.min_payoff = q.min_payoff;
                c.max_visits = q.max_visits; c.min_visits = q.min_visits;
            } else {
                c.max_regret = q.max_regret > c.max_regret ? q.max_regret : c.max_regret;
                c.min_regret = q.min_regret < c.min_regret ? q.min_regret : c.min_regret;
                c.max_weight = q.max_weight > c.max_weight ? q.max_weight : c.max_weight;
                c.max_payoff = q.max_payoff > c.max_payoff ? q.max_payoff : c.max_payoff;
                c.min_payoff = q.min_payoff < c.min_payoff ? q.min_payoff : c.min_payoff;
                c.max_visits = q.max_visits > c.max_visits ? q.max_visits : c.max_visits;
                c.min_visits = q.min_visits < c.min_visits ? q.min_visits : c.min_visits;
            }
            c.rows += q.rows; c.rated += q.rated; c.dominant += q.dominant; c.visits += q.visits;
        }
        nc_store(&out->cell[cell / RP_NLHE_CENSUS_CODES][cell % RP_NLHE_CENSUS_CODES], c);
        return;
    }
    if (blockIdx.x > 4u) return;
    const uint32_t which = blockIdx.x - 3u;
    NcList l;
    nc_list_clear(l);
    for (uint32_t s = 0; s < nseg; ++s) {
        const uint32_t n = part.counts[(size_t)s * 2u + which];
        const rp_census_entry* e = part.lists + ((size_t)s * 2u + which) * NC_TOP;
        for (uint32_t i = 0; i < n; ++i)  // a partial list is in rank order: behind the first entry that stays out, all stay out
            if (!nc_list_insert(l, lane, e[i].past, e[i].choices, e[i].present, e[i].edges, e[i].visits, __float_as_uint(e[i].regret))) break;
    }
    const bool live = lane < l.n;
    rp_census_entry o;
    o.past = live ? l.past : 0; o.choices = live ? l.choices : 0; o.present = live ? l.present : 0; o.edges = live ? l.edges : 0;
    o.visits = (live && which == 0u) ? l.key : 0u;
    o.regret = __uint_as_float((live && which == 1u) ? l.val : 0u);
    if (which == 0u) {
        out->cold[lane] = o;
        if (lane < 5u) {
            uint64_t k = 0;
            for (uint32_t s = 0; s < nseg; ++s) k += part.infosets[(size_t)s * 5u + lane];
            out->infosets[lane] = k;
        }
        if (lane == 0) {
            out->epoch = epoch;
            out->slots = slots;
            out->n_cold = l.n;
        }
    } else {
        out->hot[lane] = o;
        if (lane == 0) out->n_hot = l.n;
    }
}

}  // namespace rp

#endif
