// atlas.hip — host entry points of rp_atlas (include/rp_mi355x.h "abstraction atlas"); the kernels are in atlas.hpp.
// Argument checks that need no device come first; the table's own check is rp_lookup_create's, whose search keys the queries use.
#include <hip/hip_runtime.h>

#include <vector>

#include "atlas.hpp"
#include "host_util.hpp"

using namespace rp;
using atlas::View;

struct rp_atlas {
    int device = 0, street = 0;
    uint64_t n = 0;
    uint32_t K = 0, bins = 0;
    rp_lookup* lookup = nullptr;
    int64_t* obs = nullptr;
    uint32_t *population = nullptr, *offset = nullptr, *members = nullptr, *position = nullptr, *rows = nullptr, *future = nullptr;
    float *equity = nullptr, *fold = nullptr, *tri = nullptr, *row_equity = nullptr;
    uint64_t* weight = nullptr;
    double sort_ms = 0.0, rest_ms = 0.0;
    View view{};
};

namespace {

const uint32_t N_CARDS[4] = {2, 5, 6, 7};                                           // street.rs:59-66
const double N_OBSERVATIONS[4] = {1326.0, 25989600.0, 305377800.0, 2809475760.0};   // street.rs:138-145
const double N_ISOMORPHISMS[4] = {169.0, 1286792.0, 13960050.0, 123156254.0};       // street.rs:129-136
const double N_CHILDREN[4] = {19600.0, 47.0, 46.0, 0.0};                            // street.rs:120-127

// sort_rows' temporaries: device allocations that free themselves
struct Arena {
    std::vector<void*> ptrs;
    ~Arena() {
        for (void* p : ptrs) (void)hipFree(p);
    }
    template <class T>
    hipError_t alloc(T** out, size_t count) {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, count * sizeof(T) ? count * sizeof(T) : 1);
        if (e == hipSuccess) ptrs.push_back(p);
        *out = static_cast<T*>(p);
        return e;
    }
};
struct Events {
    hipEvent_t a = nullptr, b = nullptr, c = nullptr;
    Events() {
        (void)hipEventCreate(&a);
        (void)hipEventCreate(&b);
        (void)hipEventCreate(&c);
    }
    ~Events() {
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
        (void)hipEventDestroy(c);
    }
};

int pick_device(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return rp::fail(RP_ERR_NO_DEVICE, "no HIP device: the library has no CPU path");
    if (device < 0 || device >= count) return rp::fail(RP_ERR_INVALID, "device %d out of range (%d devices)", device, count);
    HIP_TRY(hipSetDevice(device));
    return RP_OK;
}
unsigned blocks_of(uint64_t n, uint32_t per) { return (unsigned)((n + per - 1) / per); }

void release(rp_atlas* h) {
    (void)rp_lookup_destroy(h->lookup);
    for (void* p : {(void*)h->obs, (void*)h->population, (void*)h->offset, (void*)h->members, (void*)h->position, (void*)h->rows, (void*)h->future,
                    (void*)h->equity, (void*)h->fold, (void*)h->tri, (void*)h->row_equity, (void*)h->weight})
        if (p) (void)hipFree(p);
    delete h;
}

// members <- the rows by (abs, obs): one or two rounds of at most 27 key bits, low bits first, each a stable sort of the digits
int sort_rows(rp_atlas* h, const uint8_t* abs_) {
    const uint32_t n = (uint32_t)h->n, nc = N_CARDS[h->street], total = 6u * nc + 8u, low = total < 27u ? total : 27u, high = total - low;
    Arena tmp;
    uint32_t *ka, *kb, *va, *perm = nullptr;
    unsigned char* scratch;
    HIP_TRY(tmp.alloc(&ka, n));
    HIP_TRY(tmp.alloc(&kb, n));
    HIP_TRY(tmp.alloc(&va, n));
    if (high) HIP_TRY(tmp.alloc(&perm, n));
    HIP_TRY(tmp.alloc(&scratch, ss::sort_scratch_bytes(n)));
    const dim3 grid(blocks_of(n, 256)), block(256);
    hipLaunchKernelGGL(atlas::k_atlas_digits, grid, block, 0, nullptr, h->obs, abs_, (const uint32_t*)nullptr, n, nc, 0u, low, ka, va);
    HIP_TRY(ss::sort_pairs(ka, va, kb, high ? perm : h->members, n, low, scratch, nullptr));
    if (high) {
        hipLaunchKernelGGL(atlas::k_atlas_digits, grid, block, 0, nullptr, h->obs, abs_, (const uint32_t*)perm, n, nc, low, high, ka, (uint32_t*)nullptr);
        HIP_TRY(ss::sort_pairs(ka, perm, kb, h->members, n, high, scratch, nullptr));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());  // the temporaries are freed on return
    return RP_OK;
}

int derive(rp_atlas* h, const float* next_equity) {
    const uint32_t n = (uint32_t)h->n;
    const uint64_t* keys;
    const uint8_t* abs_;
    uint64_t rows;
    int street;
    if (int rc = rp::lookup_view(h->lookup, &keys, &abs_, &rows, &street)) return rc;
    HIP_TRY(hipMalloc((void**)&h->population, (h->K + 1) * 4));  // the last word counts the rows with abs >= K
    HIP_TRY(hipMalloc((void**)&h->offset, (h->K + 1) * 4));
    HIP_TRY(hipMalloc((void**)&h->members, (size_t)n * 4));
    HIP_TRY(hipMalloc((void**)&h->position, (size_t)n * 4));
    HIP_TRY(hipMalloc((void**)&h->equity, h->K * 4));
    HIP_TRY(hipMemset(h->population, 0, (h->K + 1) * 4));
    Events ev;
    const unsigned per_wg = 256u * 64u;
    const unsigned hist_grid = blocks_of(n, per_wg) < 2048u ? blocks_of(n, per_wg) : 2048u;
    hipLaunchKernelGGL(atlas::k_atlas_population, dim3(hist_grid), dim3(256), 0, nullptr, abs_, n, h->K, h->population, h->population + h->K);
    HIP_TRY(hipGetLastError());
    uint32_t bad = 0;
    HIP_TRY(hipMemcpy(&bad, h->population + h->K, 4, hipMemcpyDeviceToHost));
    if (bad) return rp::fail(RP_ERR_INVALID, "rp_atlas_create: %u rows have an abstraction index >= K = %u", bad, h->K);
    HIP_TRY(hipEventRecord(ev.a, nullptr));
    if (int rc = sort_rows(h, abs_)) return rc;
    HIP_TRY(hipEventRecord(ev.b, nullptr));
    hipLaunchKernelGGL(atlas::k_atlas_offsets, dim3(1), dim3(256), 0, nullptr, h->population, h->K, h->offset);
    hipLaunchKernelGGL(atlas::k_atlas_position, dim3(blocks_of(n, 256)), dim3(256), 0, nullptr, h->members, abs_, h->offset, n, h->position);
    if (h->street == RP_STREET_RIVE) {
        hipLaunchKernelGGL(atlas::k_atlas_river_equity, dim3(1), dim3(256), 0, nullptr, h->K, h->equity);
    } else {
        HIP_TRY(hipMalloc((void**)&h->fold, h->K * 4));
        HIP_TRY(hipMalloc((void**)&h->rows, h->K * 4));
        hipLaunchKernelGGL(atlas::k_atlas_equity, dim3(h->K), dim3(64), 0, nullptr, h->future, h->weight, h->bins, next_equity, h->equity, h->fold,
                           h->rows);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.c, nullptr));
    HIP_TRY(hipEventSynchronize(ev.c));
    float sort_ms = 0.0f, rest_ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&sort_ms, ev.a, ev.b));
    HIP_TRY(hipEventElapsedTime(&rest_ms, ev.b, ev.c));
    h->sort_ms = sort_ms, h->rest_ms = rest_ms;
    View& v = h->view;
    v.keys = keys, v.abs_ = abs_, v.obs = h->obs, v.population = h->population, v.offset = h->offset, v.members = h->members;
    v.position = h->position, v.equity = h->equity, v.fold = h->fold, v.rows = h->rows, v.tri = h->tri, v.row_equity = h->row_equity;
    v.future = h->future, v.weight = h->weight, v.n = h->n, v.K = h->K, v.bins = h->bins, v.street = (uint32_t)h->street;
    v.n_cards = N_CARDS[h->street];
    v.n_observations = (float)N_OBSERVATIONS[h->street], v.n_isomorphisms = (float)N_ISOMORPHISMS[h->street];
    v.n_children = (float)N_CHILDREN[h->street];
    return RP_OK;
}

// ---- the queries: pairs by the rule of host_util.hpp ("entry points in pairs"), on the null stream.  begin and need_* are what the
// pairs' checks share; the _device forms return after the device finished (finish)
int begin(const rp_atlas* h, const char* who, uint64_t n, bool nulls) {
    if (!h) return rp::fail(RP_ERR_INVALID, "%s: NULL handle", who);
    if (n && nulls) return rp::fail(RP_ERR_INVALID, "%s: null argument", who);
    if (n > (1ull << 32)) return rp::fail(RP_ERR_INVALID, "%s: at most 2^32 queries per call", who);
    return RP_OK;
}
int finish() {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return RP_OK;
}
int need_tri(const rp_atlas* h, const char* who) {
    return h->tri ? RP_OK : rp::fail(RP_ERR_UNSUPPORTED, "%s: this atlas was created without a metric (tri)", who);
}
int need_future(const rp_atlas* h, const char* who) {
    return h->future ? RP_OK : rp::fail(RP_ERR_UNSUPPORTED, "%s: a river atlas has no transitions", who);
}
int check_describe(const rp_atlas* h, uint64_t n, const void* obs, const void* wrt, const void* out, const void* status) {
    if (int rc = begin(h, "rp_atlas_describe", n, !obs || !out || !status)) return rc;
    return wrt ? need_tri(h, "rp_atlas_describe") : RP_OK;
}
int check_obs_equity(const rp_atlas* h, uint64_t n, const void* obs, const void* out, const void* status) {
    if (int rc = begin(h, "rp_atlas_obs_equity", n, !obs || !out || !status)) return rc;
    if (h->street == RP_STREET_RIVE && !h->row_equity)
        return rp::fail(RP_ERR_UNSUPPORTED, "rp_atlas_obs_equity: this river atlas was created without row_equity");
    return RP_OK;
}
int check_pick(const rp_atlas* h, uint64_t n, const void* abs, const void* draw, const void* out, const void* status) {
    return begin(h, "rp_atlas_pick", n, !abs || !draw || !out || !status);
}
int check_neighbors(const rp_atlas* h, uint64_t n, const void* wrt, uint32_t k, const void* out, const void* status) {
    if (int rc = begin(h, "rp_atlas_neighbors", n, !wrt || !out || !status)) return rc;
    if (int rc = need_tri(h, "rp_atlas_neighbors")) return rc;
    const uint32_t most = h->K - 1u < atlas::MAX_NEIGHBORS ? h->K - 1u : atlas::MAX_NEIGHBORS;
    if (k == 0 || k > most) return rp::fail(RP_ERR_INVALID, "rp_atlas_neighbors: k = %u, must be in 1..min(K - 1, 16) = %u", k, most);
    return RP_OK;
}
int check_distance(const rp_atlas* h, uint64_t n, const void* a, const void* b, const void* out) {
    if (int rc = begin(h, "rp_atlas_distance", n, !a || !b || !out)) return rc;
    return need_tri(h, "rp_atlas_distance");
}
int check_histograms(const rp_atlas* h, uint64_t n, int kind, const void* ids, const void* counts, const void* status) {
    if (int rc = begin(h, "rp_atlas_histograms", n, !ids || !counts || !status)) return rc;
    if (int rc = need_future(h, "rp_atlas_histograms")) return rc;
    if (kind != RP_ATLAS_HIST_ABS && kind != RP_ATLAS_HIST_OBS) return rp::fail(RP_ERR_INVALID, "rp_atlas_histograms: kind %d (0 ABS, 1 OBS)", kind);
    return RP_OK;
}
int check_members(const rp_atlas* h, uint64_t n, const void* abs, const void* start, uint32_t count, const void* out, const void* got) {
    if (int rc = begin(h, "rp_atlas_members", n, !abs || !start || !out || !got)) return rc;
    if (count == 0 || count > atlas::MAX_WINDOW) return rp::fail(RP_ERR_INVALID, "rp_atlas_members: count = %u, must be in 1..16", count);
    return RP_OK;
}

}  // namespace

extern "C" {

int rp_atlas_create(int device, int street, uint64_t n, const int64_t* obs_dev, const uint8_t* abs_dev, uint32_t K, const uint32_t* future_counts,
                    const uint64_t* future_weight, uint32_t bins, const float* tri, const float* row_equity_dev, const rp_atlas* next, rp_atlas** out) {
    if (!out || !obs_dev || !abs_dev || !n) return rp::fail(RP_ERR_INVALID, "rp_atlas_create: null or empty argument");
    if (street < 0 || street > 3) return rp::fail(RP_ERR_INVALID, "rp_atlas_create: street %d: preflop (0), flop (1), turn (2) or river (3)", street);
    if (K == 0 || K > atlas::MAX_K) return rp::fail(RP_ERR_INVALID, "rp_atlas_create: K = %u, must be in 1..256", K);
    if (n > RP_ATLAS_MAX_ROWS) return rp::fail(RP_ERR_UNSUPPORTED, "rp_atlas_create: %llu rows; row indices are 27 bits", (unsigned long long)n);
    if (street == RP_STREET_RIVE) {
        if (future_counts || future_weight || tri || next || bins)
            return rp::fail(RP_ERR_INVALID, "rp_atlas_create: a river atlas takes no future, no tri, no next and bins = 0");
    } else {
        if (!future_counts || !future_weight || !next) return rp::fail(RP_ERR_INVALID, "rp_atlas_create: future_counts, future_weight and next are required");
        if (row_equity_dev) return rp::fail(RP_ERR_INVALID, "rp_atlas_create: row_equity is the river's column");
        if (next->street != street + 1) return rp::fail(RP_ERR_INVALID, "rp_atlas_create: next is the atlas of street %d, not %d", next->street, street + 1);
        if (next->device != device) return rp::fail(RP_ERR_INVALID, "rp_atlas_create: next lives on device %d, not %d", next->device, device);
        if (bins != next->K) return rp::fail(RP_ERR_INVALID, "rp_atlas_create: bins = %u, next has K = %u", bins, next->K);
    }
    if (int rc = pick_device(device)) return rc;
    rp_atlas* h = new rp_atlas;
    h->device = device, h->street = street, h->n = n, h->K = K, h->bins = bins;
    auto build = [&]() -> int {
        if (int rc = rp_lookup_create(device, street, n, obs_dev, abs_dev, &h->lookup)) return rc;
        HIP_TRY(hipMalloc((void**)&h->obs, n * 8));
        HIP_TRY(hipMemcpy(h->obs, obs_dev, n * 8, hipMemcpyDeviceToDevice));
        if (row_equity_dev) {
            HIP_TRY(hipMalloc((void**)&h->row_equity, n * 4));
            HIP_TRY(hipMemcpy(h->row_equity, row_equity_dev, n * 4, hipMemcpyDeviceToDevice));
        }
        if (future_counts) {
            HIP_TRY(hipMalloc((void**)&h->future, (size_t)K * bins * 4));
            HIP_TRY(hipMalloc((void**)&h->weight, (size_t)K * 8));
            HIP_TRY(hipMemcpy(h->future, future_counts, (size_t)K * bins * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(h->weight, future_weight, (size_t)K * 8, hipMemcpyHostToDevice));
        }
        if (tri && K > 1) {
            const size_t pairs = (size_t)K * (K - 1) / 2;
            HIP_TRY(hipMalloc((void**)&h->tri, pairs * 4));
            HIP_TRY(hipMemcpy(h->tri, tri, pairs * 4, hipMemcpyHostToDevice));
        }
        return derive(h, next ? next->equity : nullptr);
    };
    if (int rc = build()) {
        release(h);
        return rc;
    }
    *out = h;
    return RP_OK;
}

int rp_atlas_destroy(rp_atlas* h) {
    if (!h) return RP_OK;
    (void)hipSetDevice(h->device);
    release(h);
    return RP_OK;
}

int rp_atlas_shape(const rp_atlas* h, uint64_t* n, uint32_t* K, uint32_t* bins, int* street) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_atlas_shape: NULL handle");
    if (n) *n = h->n;
    if (K) *K = h->K;
    if (bins) *bins = h->bins;
    if (street) *street = h->street;
    return RP_OK;
}

int rp_atlas_tables(rp_atlas* h, uint32_t* population, uint32_t* offset, float* equity, uint32_t* position, uint32_t* members) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_atlas_tables: NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    if (population) HIP_TRY(hipMemcpy(population, h->population, h->K * 4, hipMemcpyDefault));
    if (offset) HIP_TRY(hipMemcpy(offset, h->offset, (h->K + 1) * 4, hipMemcpyDefault));
    if (equity) HIP_TRY(hipMemcpy(equity, h->equity, h->K * 4, hipMemcpyDefault));
    if (position) HIP_TRY(hipMemcpy(position, h->position, h->n * 4, hipMemcpyDefault));
    if (members) HIP_TRY(hipMemcpy(members, h->members, h->n * 4, hipMemcpyDefault));
    return RP_OK;
}

int rp_atlas_create_ms(const rp_atlas* h, double* sort_ms, double* rest_ms) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_atlas_create_ms: NULL handle");
    if (sort_ms) *sort_ms = h->sort_ms;
    if (rest_ms) *rest_ms = h->rest_ms;
    return RP_OK;
}

int rp_atlas_describe_device(rp_atlas* h, uint64_t n, const int64_t* obs, const uint8_t* wrt, rp_atlas_sample* out, uint8_t* status) {
    int rc = check_describe(h, n, obs, wrt, out, status);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(atlas::k_atlas_describe, dim3(blocks_of(n, 256)), dim3(256), 0, nullptr, h->view, n, obs, wrt, out, status);
    return finish();
}
int rp_atlas_describe(rp_atlas* h, uint64_t n, const int64_t* obs, const uint8_t* wrt, rp_atlas_sample* out, uint8_t* status) {
    int rc = check_describe(h, n, obs, wrt, out, status);
    if (rc || n == 0) return rc;
    Stage s(h->device, nullptr);
    s.in(obs, n).in(wrt, n).out(out, n).out(status, n);
    if ((rc = s.up()) || (rc = rp_atlas_describe_device(h, n, obs, wrt, out, status))) return rc;
    return s.down();
}

int rp_atlas_obs_equity_device(rp_atlas* h, uint64_t n, const int64_t* obs, float* out, uint8_t* status) {
    int rc = check_obs_equity(h, n, obs, out, status);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(atlas::k_atlas_obs_equity, dim3(blocks_of(n, 256)), dim3(256), 0, nullptr, h->view, n, obs, out, status);
    return finish();
}
int rp_atlas_obs_equity(rp_atlas* h, uint64_t n, const int64_t* obs, float* out, uint8_t* status) {
    int rc = check_obs_equity(h, n, obs, out, status);
    if (rc || n == 0) return rc;
    Stage s(h->device, nullptr);
    s.in(obs, n).out(out, n).out(status, n);
    if ((rc = s.up()) || (rc = rp_atlas_obs_equity_device(h, n, obs, out, status))) return rc;
    return s.down();
}

int rp_atlas_pick_device(rp_atlas* h, uint64_t n, const uint8_t* abs, const uint64_t* draw, rp_atlas_sample* out, uint8_t* status) {
    int rc = check_pick(h, n, abs, draw, out, status);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(atlas::k_atlas_pick, dim3(blocks_of(n, 256)), dim3(256), 0, nullptr, h->view, n, abs, draw, out, status);
    return finish();
}
int rp_atlas_pick(rp_atlas* h, uint64_t n, const uint8_t* abs, const uint64_t* draw, rp_atlas_sample* out, uint8_t* status) {
    int rc = check_pick(h, n, abs, draw, out, status);
    if (rc || n == 0) return rc;
    Stage s(h->device, nullptr);
    s.in(abs, n).in(draw, n).out(out, n).out(status, n);
    if ((rc = s.up()) || (rc = rp_atlas_pick_device(h, n, abs, draw, out, status))) return rc;
    return s.down();
}

int rp_atlas_neighbors_device(rp_atlas* h, uint64_t n, const uint8_t* wrt, uint32_t k, int farthest, const uint64_t* draws, rp_atlas_sample* out,
                              uint8_t* status) {
    int rc = check_neighbors(h, n, wrt, k, out, status);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(atlas::k_atlas_neighbors, dim3(blocks_of(n, 4)), dim3(256), 0, nullptr, h->view, n, wrt, k, farthest, draws, out, status);
    return finish();
}
int rp_atlas_neighbors(rp_atlas* h, uint64_t n, const uint8_t* wrt, uint32_t k, int farthest, const uint64_t* draws, rp_atlas_sample* out,
                       uint8_t* status) {
    int rc = check_neighbors(h, n, wrt, k, out, status);
    if (rc || n == 0) return rc;
    Stage s(h->device, nullptr);
    s.in(wrt, n).in(draws, n * k).out(out, n * k).out(status, n * k);
    if ((rc = s.up()) || (rc = rp_atlas_neighbors_device(h, n, wrt, k, farthest, draws, out, status))) return rc;
    return s.down();
}

int rp_atlas_distance_device(rp_atlas* h, uint64_t n, const uint8_t* a, const uint8_t* b, float* out) {
    int rc = check_distance(h, n, a, b, out);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(atlas::k_atlas_distance, dim3(blocks_of(n, 256)), dim3(256), 0, nullptr, h->view, n, a, b, out);
    return finish();
}
int rp_atlas_distance(rp_atlas* h, uint64_t n, const uint8_t* a, const uint8_t* b, float* out) {
    int rc = check_distance(h, n, a, b, out);
    if (rc || n == 0) return rc;
    Stage s(h->device, nullptr);
    s.in(a, n).in(b, n).out(out, n);
    if ((rc = s.up()) || (rc = rp_atlas_distance_device(h, n, a, b, out))) return rc;
    return s.down();
}

int rp_atlas_histograms_device(rp_atlas* h, uint64_t n, int kind, const void* ids, uint32_t* counts, uint8_t* status) {
    int rc = check_histograms(h, n, kind, ids, counts, status);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(atlas::k_atlas_histograms, dim3(blocks_of(n, 4)), dim3(256), 0, nullptr, h->view, n, kind, ids, counts, status);
    return finish();
}
int rp_atlas_histograms(rp_atlas* h, uint64_t n, int kind, const void* ids, uint32_t* counts, uint8_t* status) {
    int rc = check_histograms(h, n, kind, ids, counts, status);
    if (rc || n == 0) return rc;
    const uint8_t* id_bytes = static_cast<const uint8_t*>(ids);  // 1 byte an abstraction, 8 an observation
    Stage s(h->device, nullptr);
    s.in(id_bytes, n * (kind == RP_ATLAS_HIST_OBS ? 8u : 1u)).out(counts, n * h->bins).out(status, n);
    if ((rc = s.up()) || (rc = rp_atlas_histograms_device(h, n, kind, id_bytes, counts, status))) return rc;
    return s.down();
}

int rp_atlas_members_device(rp_atlas* h, uint64_t n, const uint8_t* abs, const uint32_t* start, uint32_t count, int64_t* out, uint8_t* got) {
    int rc = check_members(h, n, abs, start, count, out, got);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(atlas::k_atlas_members, dim3(blocks_of(n, 256)), dim3(256), 0, nullptr, h->view, n, abs, start, count, out, got);
    return finish();
}
int rp_atlas_members(rp_atlas* h, uint64_t n, const uint8_t* abs, const uint32_t* start, uint32_t count, int64_t* out, uint8_t* got) {
    int rc = check_members(h, n, abs, start, count, out, got);
    if (rc || n == 0) return rc;
    Stage s(h->device, nullptr);
    s.in(abs, n).in(start, n).out(out, n * count).out(got, n);
    if ((rc = s.up()) || (rc = rp_atlas_members_device(h, n, abs, start, count, out, got))) return rc;
    return s.down();
}

}  // extern "C"
