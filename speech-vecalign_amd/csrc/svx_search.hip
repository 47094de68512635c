// svx_search.hip -- exact k-NN search with row ids over a Flat database (gfx950 only): faiss' index.search(x, k)
// (score_align.py:139-141) for the unit-norm fp16 / bf16 rows of svx_margin.hip.
//
// k_knn_search is k_knn_mean's sweep (16 x d query blocks in registers as MFMA A-fragments, database tiles through LDS
// by LDS-DMA, double-buffered; the similarity matrix never exists in memory) with a per-row top-k of (value, id) PAIRS.
// The kept values of a query live in LDS as in k_knn_mean's LDS lists.  The kept ids live in the output buffer
// ids [n][k] in global memory, slot for slot beside the values: the one lane that owns a query row writes a slot's id
// when it replaces that slot's value (rare after the first tiles), and reads ids back only to break a tie.  At the end
// every wave sorts the k pairs of each of its rows by (similarity descending, id ascending) and writes both outputs.
//
// The kept set is the first k of that total order over all rows seen: the entry that leaves is the worst one (smallest
// value, of those the largest id), and a row replaces it when it comes before it in the order.  While the ids of one
// sweep ascend and the lists started empty, a row that ties with the k-th value never comes before it, so the tile
// test is "strictly greater"; lists continued from an earlier call (shards in any order) may hold larger ids, and the
// tile test becomes "greater or equal" with the ids compared by the owner lane.
#include <math.h>

#include "svx_knn.h"

#define KS_NW 4   // waves per workgroup

// One database tile: 16 x 32 similarities per wave (the k-step loop of k_knn_mean's knn_tile), then the update of
// the kept pairs.  `cur` holds tile t; the pieces of tile t + 1 are issued between the k-steps.
template <bool BF>
__device__ __forceinline__ void search_tile(const char* cur, char* nxt, const uint16_t* __restrict__ db, long t, long N, int d, int k,
                                            int k4, int hs, const uint4 (&qf)[KNN_KSTEPS], float* Sw, float* heap, float* thr,
                                            long long* ids, long n, long long id_base, bool cont, int w, int lane) {
    constexpr int rs = KNN_RS;
    constexpr int PIECES = 2 * KNN_DT / KS_NW, SPP = KNN_KSTEPS / PIECES;  // pieces per wave, k-steps per piece
    const int lr = lane & 15, lg = lane >> 4;
    f32x4_t acc[2];
    acc[0] = acc[1] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const char* bp = cur + lr * rs + 16 * lg;
    // B-fragments are read two k-steps ahead of the MFMAs that use them
    uint4 bq[3][2];
#pragma unroll
    for (int s = 0; s < 2; s++) {
        bq[s][0] = *reinterpret_cast<const uint4*>(bp + 64 * s);
        bq[s][1] = *reinterpret_cast<const uint4*>(bp + 16 * rs + 64 * s);
    }
#pragma unroll
    for (int s = 0; s < KNN_KSTEPS; s++) {
        if (s + 2 < KNN_KSTEPS) {
            bq[(s + 2) % 3][0] = *reinterpret_cast<const uint4*>(bp + 64 * (s + 2));
            bq[(s + 2) % 3][1] = *reinterpret_cast<const uint4*>(bp + 16 * rs + 64 * (s + 2));
        }
        if (s % SPP == 0) knn_fetch_piece<KS_NW>(db, t + 1, N, d, nxt, w, lane, s / SPP);
        __builtin_amdgcn_sched_barrier(0);  // keep the reads ahead of this k-step's MFMAs
        mma16<BF>(acc[0], qf[s], bq[s % 3][0]);
        mma16<BF>(acc[1], qf[s], bq[s % 3][1]);
    }
    // ---- acc[j][r] = <query 16 w + 4 lg + r, database row 32 t + 16 j + lr>
    const bool c0 = t * KNN_DT + lr < N, c1 = t * KNN_DT + 16 + lr < N;
    // bal[j][r]: lanes whose value may enter the list of its row (thr is +INF for query rows past n)
    unsigned long long bal[2][4];
    unsigned long long any = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const float tv = thr[w * 16 + 4 * lg + r];
        bal[0][r] = __ballot(c0 && (cont ? acc[0][r] >= tv : acc[0][r] > tv));
        bal[1][r] = __ballot(c1 && (cont ? acc[1][r] >= tv : acc[1][r] > tv));
        any |= bal[0][r] | bal[1][r];
    }
    if (any == 0) return;  // wave-uniform
#pragma unroll
    for (int r = 0; r < 4; r++) {
        float* row = Sw + (4 * lg + r) * KNN_SPAD;
        row[lr] = acc[0][r];
        row[16 + lr] = acc[1][r];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < 16) {
        // the owner lane of a row walks that row's flagged columns in ascending order (= ascending id)
        const int orr = lane & 3, sh = 16 * (lane >> 2);
        unsigned long long m0 = 0, m1 = 0;
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (orr == r) { m0 = bal[0][r]; m1 = bal[1][r]; }
        unsigned cols = (unsigned)((m0 >> sh) & 0xffffu) | ((unsigned)((m1 >> sh) & 0xffffu) << 16);
        const int qi = w * 16 + lane;
        const long qrow = (long)blockIdx.x * (16 * KS_NW) + qi;
        if (cols && qrow < n) {
            float* h = heap + qi * hs;
            long long* gi = ids + qrow * k;
            float tr = thr[qi];
            const float* row = Sw + lane * KNN_SPAD;
            while (cols) {
                const int c = __builtin_ctz(cols);
                cols &= cols - 1;
                const float v = row[c];
                if (v > tr || (cont && v == tr)) {
                    // the smallest kept value `lo` (first slot `at`) and the runner-up, duplicates counted
                    int at = 0;
                    float lo = INFINITY, lo2 = INFINITY;
#pragma unroll 4
                    for (int j = 0; j < k4; j += 4) {
                        const f32x4_t e = *reinterpret_cast<const f32x4_t*>(h + j);
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            if (e[u] < lo) { lo2 = lo; lo = e[u]; at = j + u; }
                            else if (e[u] < lo2) lo2 = e[u];
                        }
                    }
                    const long long id = id_base + t * KNN_DT + c;
                    bool rep = true;
                    // several slots hold `lo`, or the new row ties with it: the largest id among them is the worst pair
                    // (empty slots, -INF, are all alike)
                    if (v == lo || (lo2 == lo && lo != -INFINITY)) {
                        long long worst = gi[at];
                        for (int j = at + 1; j < k; j++)
                            if (h[j] == lo) {
                                const long long o = gi[j];
                                if (o > worst) { worst = o; at = j; }
                            }
                        if (v == lo) rep = id < worst;
                    }
                    if (rep) {
                        h[at] = v;
                        gi[at] = id;
                        tr = fminf(v, lo2);
                    }
                }
            }
            thr[qi] = tr;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One workgroup = 4 waves x 16 query rows = 64 queries; its kept values fit beside the tiles for every k <= 64.  LDS: two database tiles [KNN_DT][2064 B], per-wave
// similarity scratch, per-row kept values (unsorted, their minimum cached in thr[]).  sims / ids [n][k] are read when
// `cont` (the lists an earlier call left) and written sorted at the end.
template <bool BF, typename QE>
__global__ __launch_bounds__(64 * KS_NW, 1) void k_knn_search(const typename QE::storage* __restrict__ q, long n,
                                                              const uint16_t* __restrict__ db, long N, int d, int k,
                                                              long long id_base, float* sims, long long* ids, int cont_) {
    // (two tile buffers as two LDS objects, see k_knn_mean)
    __shared__ __attribute__((aligned(16))) char tile0[KNN_DT * KNN_RS];
    __shared__ __attribute__((aligned(16))) char tile1[KNN_DT * KNN_RS];
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NW = KS_NW, QT = 16 * NW, NT = 64 * NW;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const bool cont = cont_ != 0;
    float* S = reinterpret_cast<float*>(smem);                   // [NW][16][KNN_SPAD]
    const int k4 = (k + 3) & ~3, hs = k4 + 4;                    // list stride: 16-byte groups + one group of padding
    float* heap = S + NW * 16 * KNN_SPAD;                  // [QT][hs]: k kept values, +INF in the slots past k
    float* thr = heap + QT * hs;                                 // [QT]

    // ---- query rows -> unit norm -> MFMA A-fragments (as k_knn_mean: the similarities are defined there)
    uint4 qf[KNN_KSTEPS];
    {
        const long qrow = (long)blockIdx.x * QT + w * 16 + lr;
        const bool ok = qrow < n;
        const typename QE::storage* rowp = q + (ok ? qrow : 0) * (long)d;
        float ss = 0.f;
#pragma unroll
        for (int s = 0; s < KNN_KSTEPS; s++) {
            const int kel = 32 * s + 8 * lg;
            if (ok && kel < d) {
                float f[8];
                load8<QE>(rowp + kel, f);
#pragma unroll
                for (int j = 0; j < 8; j++) ss += f[j] * f[j];
            }
        }
        ss += __shfl_xor(ss, 16, SVX_WAVE);
        ss += __shfl_xor(ss, 32, SVX_WAVE);
        const float inv = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
#pragma unroll
        for (int s = 0; s < KNN_KSTEPS; s++) {
            const int kel = 32 * s + 8 * lg;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (ok && kel < d) {
                float f[8];
                load8<QE>(rowp + kel, f);
                v.x = pack_pair(f[0] * inv, f[1] * inv, BF);
                v.y = pack_pair(f[2] * inv, f[3] * inv, BF);
                v.z = pack_pair(f[4] * inv, f[5] * inv, BF);
                v.w = pack_pair(f[6] * inv, f[7] * inv, BF);
            }
            qf[s] = v;
        }
    }
    // ---- kept values: empty (-INF) or what the earlier call left; their ids are already in `ids`
    for (int i = tid; i < QT * hs; i += NT) {
        const int qi = i / hs, j = i % hs;
        const long qrow = (long)blockIdx.x * QT + qi;
        heap[i] = j < k ? ((cont && qrow < n) ? sims[qrow * k + j] : -INFINITY) : INFINITY;
    }
    __syncthreads();
    for (int qi = tid; qi < QT; qi += NT) {
        float m = -INFINITY;
        if (cont) {
            m = INFINITY;
            for (int j = 0; j < k; j++) m = fminf(m, heap[qi * hs + j]);
        }
        if ((long)blockIdx.x * QT + qi >= n) m = INFINITY;  // a row past n takes part in the MFMAs only
        thr[qi] = m;
    }

    const long ntiles = (N + KNN_DT - 1) / KNN_DT;
    constexpr int PIECES = 2 * KNN_DT / NW;
    if (ntiles > 0) {
#pragma unroll
        for (int i = 0; i < PIECES; i++) knn_fetch_piece<NW>(db, 0, N, d, tile0, w, lane, i);
    }
    __syncthreads();

    float* Sw = S + w * 16 * KNN_SPAD;
    // (the last tile's step fetches "tile ntiles": clamped to the last row, never computed)
    for (long t = 0; t < ntiles; t += 2) {
        search_tile<BF>(tile0, tile1, db, t, N, d, k, k4, hs, qf, Sw, heap, thr, ids, n, id_base, cont, w, lane);
        __syncthreads();
        if (t + 1 >= ntiles) break;
        search_tile<BF>(tile1, tile0, db, t + 1, N, d, k, k4, hs, qf, Sw, heap, thr, ids, n, id_base, cont, w, lane);
        __syncthreads();
    }

    // ---- sort: lane j holds pair j of a row and counts the pairs that come before it.  The ids the owner lanes wrote
    // are made visible to the other lanes of the wave first; all k ids of a row are in registers (the ranks depend on
    // every one of them) before the first of them is overwritten.
    __threadfence();
    __syncthreads();
    for (int rr = 0; rr < 16; rr++) {
        const int qi = w * 16 + rr;
        const long qrow = (long)blockIdx.x * QT + qi;
        if (qrow >= n) break;  // wave-uniform
        const float* h = heap + qi * hs;
        const bool mine = lane < k;
        const float v = mine ? h[lane] : -INFINITY;
        long long id = -1;   // an empty slot is (-INF, -1)
        if (mine && v != -INFINITY) id = ids[qrow * k + lane];
        const int ilo = (int)(id & 0xffffffffll), ihi = (int)(id >> 32);
        int rank = 0;
        for (int i = 0; i < k; i++) {
            const float vi = h[i];
            const unsigned olo = (unsigned)__builtin_amdgcn_readlane(ilo, i);
            const long long oi = ((long long)__builtin_amdgcn_readlane(ihi, i) << 32) | (long long)olo;
            rank += (vi > v || (vi == v && (oi < id || (oi == id && i < lane)))) ? 1 : 0;
        }
        if (mine) {
            sims[qrow * k + rank] = v;
            ids[qrow * k + rank] = id;
        }
    }
}

// ------------------------------------------------------------------------------------ launchers
static size_t search_smem(int k) {
    return (size_t)KS_NW * 16 * KNN_SPAD * 4 + (size_t)16 * KS_NW * (((k + 3) & ~3) + 5) * 4;
}

template <bool BF, typename QE>
static int launch_search(svx_ctx* ctx, const void* q, long n, const void* db, long N, int d, int k, long long id_base, float* sims,
                         long long* ids, int cont) {
    const size_t smem = search_smem(k);
    static size_t attr_set = 0;
    if (smem > attr_set) {
        SVX_HIP(ctx, hipFuncSetAttribute((const void*)k_knn_search<BF, QE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        attr_set = smem;
    }
    const long qt = 16 * KS_NW;
    k_knn_search<BF, QE><<<dim3((unsigned)((n + qt - 1) / qt)), dim3(64 * KS_NW), smem, ctx->stream>>>(
        reinterpret_cast<const typename QE::storage*>(q), n, reinterpret_cast<const uint16_t*>(db), N, d, k, id_base, sims, ids, cont);
    SVX_LAUNCH_CHECK(ctx, "k_knn_search");
    return SVX_OK;
}

extern "C" int svx_knn_search(svx_ctx* ctx, const void* queries, int q_dtype, int64_t n, const void* db, int db_dtype, int64_t n_db,
                              int d, int k, int64_t id_base, float* sims, int64_t* ids, int first) {
    NEED(ctx, ctx && (n == 0 || (queries && sims && ids)) && (n_db == 0 || db), "svx_knn_search: null argument");
    NEED(ctx, db_dtype == SVX_F16 || db_dtype == SVX_BF16, "svx_knn_search: the database is kept in fp16 or bf16 (got dtype %d)", db_dtype);
    NEED(ctx, n >= 0 && n_db >= 0, "svx_knn_search: negative row count");
    NEED(ctx, k >= 1 && k <= KNN_KMAX, "svx_knn_search: k = %d, supported 1..%d", k, KNN_KMAX);
    NEED(ctx, d > 0 && d % 32 == 0 && d <= 32 * KNN_KSTEPS, "embedding dimension %d: must be a positive multiple of 32, at most %d", d,
         32 * KNN_KSTEPS);
    if (n == 0) return SVX_OK;
    const bool bf = db_dtype == SVX_BF16;
    const int cont = first ? 0 : 1;
    long long* gi = reinterpret_cast<long long*>(ids);
    switch (q_dtype) {
    case SVX_F32:
        return bf ? launch_search<true, ElemF32>(ctx, queries, n, db, n_db, d, k, id_base, sims, gi, cont)
                  : launch_search<false, ElemF32>(ctx, queries, n, db, n_db, d, k, id_base, sims, gi, cont);
    case SVX_F16:
        return bf ? launch_search<true, ElemF16>(ctx, queries, n, db, n_db, d, k, id_base, sims, gi, cont)
                  : launch_search<false, ElemF16>(ctx, queries, n, db, n_db, d, k, id_base, sims, gi, cont);
    case SVX_BF16:
        return bf ? launch_search<true, ElemBF16>(ctx, queries, n, db, n_db, d, k, id_base, sims, gi, cont)
                  : launch_search<false, ElemBF16>(ctx, queries, n, db, n_db, d, k, id_base, sims, gi, cont);
    default: return svx_fail(ctx, SVX_ERR_ARG, "svx_knn_search: unknown query dtype %d", q_dtype);
    }
}
