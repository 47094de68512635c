// svx_mine.hip -- candidate scoring of margin-based mining (gfx950 only): what follows two svx_knn_search calls when
// the rows of one side are mined against the other (Artetxe & Schwenk, P19-1309 sec. 3; LASER mine_bitexts.py:
// score_candidates + argmax).
//
// Two streaming kernels over the lists [n][k] a search left, one thread per list.  k_list_means adds a list's k
// similarities one by one; k_margin_candidates re-scores every neighbour with the margin -- the mean of the other side
// is gathered through the neighbour's id, n * k floats that stay in L2 / Infinity Cache -- and keeps the first best one.
// The operation order is the contract of include/svx.h (tests compare bits), so a lane walks its list from j = 0 up
// and nothing is reduced across lanes.  A list is read in 16-byte pieces when k is a multiple of 4 (every list then
// starts on a 16-byte boundary); no LDS, no scratch: the walk keeps one accumulator or one (score, id) pair.
#include <math.h>

#include "svx_common.h"

#define MINE_NT 256      // threads per workgroup
#define MINE_KMAX 64
#define MINE_MAXGRID 65536

typedef long long mine_i64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ mine_i64x2 gld_ids2(const long long* p) { return *(const SVX_GLOBAL(mine_i64x2)*)p; }

// mean[i] = (((s[i][0] + s[i][1]) + ...) + s[i][k-1]) / (float)k
template <bool VEC>
__global__ __launch_bounds__(MINE_NT) void k_list_means(const float* __restrict__ sims, long n, int k, float* __restrict__ mean) {
    const long step = (long)gridDim.x * MINE_NT;
    for (long i = (long)blockIdx.x * MINE_NT + threadIdx.x; i < n; i += step) {
        const float* s = sims + i * (long)k;
        float acc;
        if (VEC) {
            float4 v = gldf4(s);
            acc = ((v.x + v.y) + v.z) + v.w;
            for (int j = 4; j < k; j += 4) {
                v = gldf4(s + j);
                acc = (((acc + v.x) + v.y) + v.z) + v.w;
            }
        } else {
            acc = gld(s);
            for (int j = 1; j < k; j++) acc += gld(s + j);
        }
        gst(mean + i, acc / (float)k);
    }
}

// The state of one list's walk: candidate j replaces the best so far when its score is strictly greater.
struct MineBest {
    float score;
    long long id;
};

template <int MARGIN>
__device__ __forceinline__ float mine_score(float sim, long long id, float mq, const float* __restrict__ mean_db, long n_db,
                                            long long id_base, MineBest& best) {
#pragma clang fp contract(off)
    // (unsigned: one comparison covers ids below id_base and ids at or past id_base + n_db)
    const unsigned long long r = (unsigned long long)id - (unsigned long long)id_base;
    float sc = -INFINITY;
    if (id != -1 && r < (unsigned long long)n_db) {
        if (MARGIN == SVX_MARGIN_ABSOLUTE) {
            sc = sim;
        } else {
            const float b = (mq + gld(mean_db + r)) * 0.5f;
            sc = MARGIN == SVX_MARGIN_RATIO ? sim / b : sim - b;
        }
    }
    if (sc > best.score) {
        best.score = sc;
        best.id = id;
    }
    return sc;
}

template <int MARGIN, bool VEC>
__global__ __launch_bounds__(MINE_NT) void k_margin_candidates(const float* __restrict__ sims, const long long* __restrict__ ids, long n,
                                                               int k, const float* __restrict__ mean_q,
                                                               const float* __restrict__ mean_db, long n_db, long long id_base,
                                                               float* __restrict__ scores, long long* __restrict__ best_id,
                                                               float* __restrict__ best_score) {
    const long step = (long)gridDim.x * MINE_NT;
    for (long i = (long)blockIdx.x * MINE_NT + threadIdx.x; i < n; i += step) {
        const float* s = sims + i * (long)k;
        const long long* id = ids + i * (long)k;
        float* out = scores ? scores + i * (long)k : nullptr;
        const float mq = MARGIN == SVX_MARGIN_ABSOLUTE ? 0.f : gld(mean_q + i);
        MineBest best = {-INFINITY, -1};
        if (VEC) {
            for (int j = 0; j < k; j += 4) {
                const float4 v = gldf4(s + j);
                const mine_i64x2 a = gld_ids2(id + j), b = gld_ids2(id + j + 2);
                const float s0 = mine_score<MARGIN>(v.x, a.x, mq, mean_db, n_db, id_base, best);
                const float s1 = mine_score<MARGIN>(v.y, a.y, mq, mean_db, n_db, id_base, best);
                const float s2 = mine_score<MARGIN>(v.z, b.x, mq, mean_db, n_db, id_base, best);
                const float s3 = mine_score<MARGIN>(v.w, b.y, mq, mean_db, n_db, id_base, best);
                if (out) gstf4(out + j, s0, s1, s2, s3);
            }
        } else {
            for (int j = 0; j < k; j++) {
                const float sc = mine_score<MARGIN>(gld(s + j), gld(id + j), mq, mean_db, n_db, id_base, best);
                if (out) gst(out + j, sc);
            }
        }
        gst(best_id + i, best.id);
        gst(best_score + i, best.score);
    }
}

// ------------------------------------------------------------------------------------ launchers
static unsigned mine_grid(int64_t n) {
    const int64_t g = (n + MINE_NT - 1) / MINE_NT;
    return (unsigned)(g < MINE_MAXGRID ? g : MINE_MAXGRID);
}

template <int MARGIN>
static void launch_candidates(svx_ctx* ctx, const float* sims, const long long* ids, long n, int k, const float* mean_q,
                              const float* mean_db, long n_db, long long id_base, float* scores, long long* best_id, float* best_score) {
    const dim3 grid(mine_grid(n)), block(MINE_NT);
    if (k % 4 == 0 && aligned16(sims) && aligned16(ids) && aligned16(scores))
        k_margin_candidates<MARGIN, true><<<grid, block, 0, ctx->stream>>>(sims, ids, n, k, mean_q, mean_db, n_db, id_base, scores, best_id, best_score);
    else
        k_margin_candidates<MARGIN, false><<<grid, block, 0, ctx->stream>>>(sims, ids, n, k, mean_q, mean_db, n_db, id_base, scores, best_id, best_score);
}

extern "C" {

int svx_knn_list_means(svx_ctx* ctx, const float* sims, int64_t n, int k, float* mean) {
    NEED(ctx, ctx && (n == 0 || (sims && mean)), "svx_knn_list_means: null argument");
    NEED(ctx, n >= 0, "svx_knn_list_means: negative row count");
    NEED(ctx, k >= 1 && k <= MINE_KMAX, "svx_knn_list_means: k = %d, supported 1..%d", k, MINE_KMAX);
    if (n == 0) return SVX_OK;
    const dim3 grid(mine_grid(n)), block(MINE_NT);
    if (k % 4 == 0 && aligned16(sims))
        k_list_means<true><<<grid, block, 0, ctx->stream>>>(sims, n, k, mean);
    else
        k_list_means<false><<<grid, block, 0, ctx->stream>>>(sims, n, k, mean);
    SVX_LAUNCH_CHECK(ctx, "k_list_means");
    return SVX_OK;
}

int svx_margin_candidates(svx_ctx* ctx, const float* sims, const int64_t* ids, int64_t n, int k, const float* mean_q,
                          const float* mean_db, int64_t n_db, int64_t id_base, int margin, float* scores, int64_t* best_id,
                          float* best_score) {
    NEED(ctx, margin == SVX_MARGIN_RATIO || margin == SVX_MARGIN_DISTANCE || margin == SVX_MARGIN_ABSOLUTE, "Wrong margin type: %d", margin);
    const bool means = margin != SVX_MARGIN_ABSOLUTE;   // the absolute score reads neither mean
    NEED(ctx, ctx && (n == 0 || (sims && ids && best_id && best_score && (!means || (mean_q && (mean_db || n_db == 0))))),
         "svx_margin_candidates: null argument");
    NEED(ctx, n >= 0 && n_db >= 0, "svx_margin_candidates: negative row count");
    NEED(ctx, k >= 1 && k <= MINE_KMAX, "svx_margin_candidates: k = %d, supported 1..%d", k, MINE_KMAX);
    if (n == 0) return SVX_OK;
    const long long* gi = reinterpret_cast<const long long*>(ids);
    long long* bi = reinterpret_cast<long long*>(best_id);
    switch (margin) {
    case SVX_MARGIN_RATIO: launch_candidates<SVX_MARGIN_RATIO>(ctx, sims, gi, n, k, mean_q, mean_db, n_db, id_base, scores, bi, best_score); break;
    case SVX_MARGIN_DISTANCE: launch_candidates<SVX_MARGIN_DISTANCE>(ctx, sims, gi, n, k, mean_q, mean_db, n_db, id_base, scores, bi, best_score); break;
    default: launch_candidates<SVX_MARGIN_ABSOLUTE>(ctx, sims, gi, n, k, mean_q, mean_db, n_db, id_base, scores, bi, best_score); break;
    }
    SVX_LAUNCH_CHECK(ctx, "k_margin_candidates");
    return SVX_OK;
}

}  // extern "C"
