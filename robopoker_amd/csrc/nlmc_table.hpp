// nlmc_table.hpp — moving the NLHE infoset table itself on the device: compact it (rp_nlhe_export_device), insert into it in bulk
// (rp_nlhe_import_device) and rehash it into a table of another size (rp_nlhe_resize, and the growth in front of a step).
//
// Reference: the profile is a HashMap that grows by itself (mccfr/src/strategy/macros.rs:13-16); NlheProfile::rows streams it out
// and Hydrate loads it (nlhe/src/profile.rs:90-163).  Here the table is NlTable (nlmc_common.hpp): 32-byte key slots beside 144-byte
// rows, slot index = row, open addressing with linear probing from nl_key_hash.
//
// None of the three is bound by occupancy: a slot is 32 B and a row 144 B, read or written at hashed places, so what counts is how many
// bytes one lane keeps in flight.  ONE LANE MOVES ONE ROW, as nine 16-byte pieces issued back to back: the nine pieces of a row share
// two or three 128-byte lines, so the pieces after the first of a line find it on its way, and at the fills a table is kept at (up to
// a half) neighbouring lanes hold neighbouring slots only every other time — spreading a row over nine lanes would coalesce the
// 144 B and idle the lanes of empty slots.  The Encounter <-> row transposition (rp_encounter is {weight, regret, payoff, visits} per
// action, a row is regret[9] weight[9] payoff[9] visits[9]) then happens in the lane's registers.
//   k_nl_table_count    a wavefront per SEGMENT of NT_SEGMENT slots: the ready slots of the segment (a ballot per 64 slots)
//   k_nl_table_compact  the same walk behind an exclusive scan of the segment counts: rank in the segment = the ready slots before it
//                       (running count + the ballot's prefix), so the output is in slot order — rp_nlhe_export's
//   k_nl_table_find     find or insert every key of a batch (nl_row_of with no actions to initialise, born = 0) and claim its slot for
//                       the LAST index that names it: atomicMax of i + 1 into the slot's `pad` word, which is zero between launches
//   k_nl_table_write    the owner of a slot writes the whole row from its Encounters and clears the claim
//   k_nl_table_rehash   old slots read coalesced; a ready one claims a slot of the new table by compare-and-swap from its new home
//                       (keys of a table are distinct: nobody waits for anybody, state goes 0 -> 2 at once) and copies its row
#ifndef RP_NLMC_TABLE_HPP
#define RP_NLMC_TABLE_HPP

#include "nlmc_common.hpp"

namespace rp {

#define NT_SEGMENT 1024u  // slots one wavefront compacts in order (a table has at least 256 slots: a short table is one short segment)
#define NT_BLOCK 256u     // four wavefronts, a segment each
#define NT_NO_ROW 0xffffffffu
static_assert(NT_SEGMENT % 64u == 0, "a segment is walked 64 slots at a time");
static_assert(sizeof(rp_encounter) == 16 && sizeof(NlSlot) == 32, "16-byte pieces");

__device__ __forceinline__ uint32_t nt_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t nt_segment_slots(uint64_t slots, uint32_t seg) {  // a multiple of 64: slots is a power of two >= 256
    const uint64_t left = slots - (uint64_t)seg * NT_SEGMENT;
    return (uint32_t)(left < NT_SEGMENT ? left : NT_SEGMENT);
}

// a row <-> its nine Encounters, in registers (every index is a constant once the loops are unrolled)
__device__ __forceinline__ void nt_load9(const float4* src, float* f) {
#pragma unroll
    for (uint32_t k = 0; k < 9u; ++k) {
        const float4 q = src[k];
        f[4u * k] = q.x; f[4u * k + 1u] = q.y; f[4u * k + 2u] = q.z; f[4u * k + 3u] = q.w;
    }
}
__device__ __forceinline__ void nt_row_to_encounters(const float* rows, uint32_t row, rp_encounter* out) {
    float f[4u * NLMC_A];
    nt_load9(reinterpret_cast<const float4*>(rows + (size_t)row * 4u * NLMC_A), f);
    float4* o = reinterpret_cast<float4*>(out);
#pragma unroll
    for (uint32_t a = 0; a < NLMC_A; ++a) o[a] = make_float4(f[NLMC_A + a], f[a], f[2u * NLMC_A + a], f[3u * NLMC_A + a]);
}
__device__ __forceinline__ void nt_encounters_to_row(const rp_encounter* in, float* rows, uint32_t row) {
    float e[4u * NLMC_A], f[4u * NLMC_A];
    nt_load9(reinterpret_cast<const float4*>(in), e);
#pragma unroll
    for (uint32_t a = 0; a < NLMC_A; ++a) {
        f[NLMC_A + a] = e[4u * a];
        f[a] = e[4u * a + 1u];
        f[2u * NLMC_A + a] = e[4u * a + 2u];
        f[3u * NLMC_A + a] = e[4u * a + 3u];  // the visits' bits
    }
    float4* o = reinterpret_cast<float4*>(rows + (size_t)row * 4u * NLMC_A);
#pragma unroll
    for (uint32_t k = 0; k < 9u; ++k) o[k] = make_float4(f[4u * k], f[4u * k + 1u], f[4u * k + 2u], f[4u * k + 3u]);
}

__global__ __launch_bounds__(NT_BLOCK) void k_nl_table_count(NlTable t, uint32_t nseg, uint32_t* seg_count) {
    const uint32_t lane = threadIdx.x & 63u, wave = nt_uniform(threadIdx.x >> 6);
    const uint64_t slots = (uint64_t)t.mask + 1u;
    for (uint32_t seg = blockIdx.x * (NT_BLOCK / 64u) + wave; seg < nseg; seg += gridDim.x * (NT_BLOCK / 64u)) {
        const uint32_t seg_n = nt_segment_slots(slots, seg);
        const uint4* sl = reinterpret_cast<const uint4*>(t.slots + (uint64_t)seg * NT_SEGMENT);
        uint32_t ready = 0;
        for (uint32_t base = 0; base < seg_n; base += 64u) ready += (uint32_t)__popcll(__ballot(sl[2u * (base + lane) + 1u].z == 2u));
        if (lane == 0) seg_count[seg] = ready;
    }
}

// the first `cap` ready slots in slot order: keys, and the row of each as nine Encounters.  seg_off = the exclusive scan of seg_count.
__global__ __launch_bounds__(NT_BLOCK) void k_nl_table_compact(NlTable t, uint32_t nseg, const uint32_t* seg_off, uint64_t cap, uint64_t* past,
                                                               uint32_t* present, uint64_t* choices, rp_encounter* enc) {
    const uint32_t lane = threadIdx.x & 63u, wave = nt_uniform(threadIdx.x >> 6);
    const uint64_t slots = (uint64_t)t.mask + 1u;
    for (uint32_t seg = blockIdx.x * (NT_BLOCK / 64u) + wave; seg < nseg; seg += gridDim.x * (NT_BLOCK / 64u)) {
        const uint32_t seg_n = nt_segment_slots(slots, seg);
        const uint64_t seg_lo = (uint64_t)seg * NT_SEGMENT;
        uint64_t at = seg_off[seg];  // wave-uniform: ready slots in front of the 64 in hand
        if (at >= cap) continue;
        for (uint32_t base = 0; base < seg_n; base += 64u) {
            const uint32_t s = (uint32_t)(seg_lo + base + lane);
            const uint4* sl = reinterpret_cast<const uint4*>(t.slots + s);
            const uint4 lo = sl[0], hi = sl[1];
            const bool ready = hi.z == 2u;
            const uint64_t b = __ballot(ready);
            const uint64_t i = at + (uint64_t)__popcll(b & ((1ull << lane) - 1ull));
            if (ready && i < cap) {
                past[i] = (uint64_t)lo.x | ((uint64_t)lo.y << 32);
                choices[i] = (uint64_t)lo.z | ((uint64_t)lo.w << 32);
                present[i] = hi.x;
                nt_row_to_encounters(t.rows, s, enc + i * NLMC_A);
            }
            at += (uint64_t)__popcll(b);
        }
    }
}

// rows[i] = the slot of key i, inserted (born 0, the row's bytes left for k_nl_table_write) where the table did not hold it; NT_NO_ROW
// and NERR_TABLE_FULL in *err where the probe ran through the whole table.  A launch is one chunk of the call's items and the chunks
// run one behind the other, so a later chunk's Encounters land on an earlier chunk's: last wins across any chunking.
__global__ __launch_bounds__(NT_BLOCK) void k_nl_table_find(NlTable t, uint32_t n, const uint64_t* past, const uint32_t* present, const uint64_t* choices,
                                                            uint32_t* rows, uint32_t* err) {
    for (uint32_t i = blockIdx.x * NT_BLOCK + threadIdx.x; i < n; i += gridDim.x * NT_BLOCK) {
        const uint64_t p = past[i], c = choices[i];
        const uint32_t b = present[i];
        uint32_t e = 0;
        bool inserted = false;
        const uint32_t row = nl_row_of(t, p, c, b, nl_key_hash(p, c, b), 0u, 0u, &e, nullptr, &inserted);
        const uint64_t fresh = __ballot(inserted);  // the lanes still in the loop; the first of them counts for all
        if (fresh != 0 && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)__ballot(true)) - 1u) atomicAdd(t.n_keys, (unsigned int)__popcll(fresh));
        if (e) {
            rows[i] = NT_NO_ROW;
            atomicOr(err, e);
        } else {
            rows[i] = row;
            atomicMax(&t.slots[row].pad, i + 1u);
        }
    }
}
__global__ __launch_bounds__(NT_BLOCK) void k_nl_table_write(NlTable t, uint32_t n, const uint32_t* rows, const rp_encounter* enc) {
    for (uint32_t i = blockIdx.x * NT_BLOCK + threadIdx.x; i < n; i += gridDim.x * NT_BLOCK) {
        const uint32_t row = rows[i];
        if (row == NT_NO_ROW || t.slots[row].pad != i + 1u) continue;  // a later item names the key again: its Encounters stay
        nt_encounters_to_row(enc + (size_t)i * NLMC_A, t.rows, row);
        t.slots[row].pad = 0u;
    }
}

// every ready slot of `from` into `to` (all slots empty, rows zero, *to.n_keys 0 before the launch): the key at the new table's probe
// position, state and born as they were, the row's 144 bytes verbatim.  The probe is bounded by the table; the host has checked
// that the keys fit, so *err stays 0.
__global__ __launch_bounds__(NT_BLOCK) void k_nl_table_rehash(NlTable from, NlTable to, uint32_t* err) {
    const uint64_t slots = (uint64_t)from.mask + 1u;
    for (uint64_t s = (uint64_t)blockIdx.x * NT_BLOCK + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * NT_BLOCK) {  // whole wavefronts: slots % 64 == 0
        const uint4* sl = reinterpret_cast<const uint4*>(from.slots + s);
        const uint4 lo = sl[0], hi = sl[1];
        const bool ready = hi.z == 2u;
        const uint64_t b = __ballot(ready);
        if ((threadIdx.x & 63u) == 0 && b != 0) atomicAdd(to.n_keys, (unsigned int)__popcll(b));
        if (!ready) continue;
        const uint64_t past = (uint64_t)lo.x | ((uint64_t)lo.y << 32), choices = (uint64_t)lo.z | ((uint64_t)lo.w << 32);
        uint32_t d = (uint32_t)nl_key_hash(past, choices, hi.x) & to.mask, probes = 0;
        bool placed = false;
        while (!placed && probes <= to.mask) {
            if (atomicCAS(&to.slots[d].state, 0u, 2u) == 0u) {  // the winner finishes the slot inside the loop body
                NlSlot* o = to.slots + d;
                o->past = past;
                o->choices = choices;
                o->present = hi.x;
                o->pad = 0u;
                o->born = hi.w;
                placed = true;
            } else {
                d = (d + 1u) & to.mask;
                probes += 1u;
            }
        }
        if (placed) {  // the row: nine loads in flight, then nine stores
            float f[4u * NLMC_A];
            nt_load9(reinterpret_cast<const float4*>(from.rows + (size_t)s * 4u * NLMC_A), f);
            float4* dst = reinterpret_cast<float4*>(to.rows + (size_t)d * 4u * NLMC_A);
#pragma unroll
            for (uint32_t k = 0; k < 9u; ++k) dst[k] = make_float4(f[4u * k], f[4u * k + 1u], f[4u * k + 2u], f[4u * k + 3u]);
        } else {
            atomicOr(err, (uint32_t)NERR_TABLE_FULL);
        }
    }
}

}  // namespace rp

#endif
