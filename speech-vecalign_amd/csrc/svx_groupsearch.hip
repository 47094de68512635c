// svx_groupsearch.hip -- svx_knn_search_groups: exact k-NN search with row ids in which every block of queries sees
// only its own range of database rows (gfx950 only).  One launch searches many (query rows, database rows) pairs -- the
// two documents of every parallel pair of a corpus, for the Local Mining baseline -- where a loop of svx_knn_search calls
// would pay a launch, two output allocations and an index object per pair.
//
// k_knn_search_groups is k_knn_search's sweep (svx_search.hip) with the workgroup's view cut to one group: 64 queries per
// workgroup, database tiles by LDS-DMA, the kept values in LDS, the kept ids in the output buffer, one sort per row at
// the end.  A workgroup never spans two groups; a group of n_g queries takes ceil(n_g / 64) workgroups; a host-built table
// maps a workgroup to (group, workgroup inside the group).  The query pointer and bound, the database pointer, N and the
// id base are the group's, so tile t of a workgroup holds the group's rows 32 t .. 32 t + 31 wherever the group starts in
// the database: the k-step order and the MFMA sequence of a query against a row are those of svx_knn_search called on
// the group's slices, and the results are equal bit for bit.  There is no continuation mode: the lists start empty, the
// ids of one sweep ascend, and the tile test is "strictly greater".
#include <math.h>
#include <string.h>

#include "svx_knn.h"

#define GS_NW 4   // waves per workgroup

namespace {

struct GroupBlock {
    int group, blk;   // the group of this workgroup, and its number inside the group (first query row = 64 blk)
};

// search_tile of svx_search.hip without the continuation branches; `first` is the workgroup's first query row inside
// its group (there: blockIdx.x * 64), n / N / db / ids / id_base are the group's.
template <bool BF>
__device__ __forceinline__ void group_search_tile(long first, const char* cur, char* nxt, const uint16_t* __restrict__ db, long t, long N,
                                                  int d, int k, int k4, int hs, const uint4 (&qf)[KNN_KSTEPS], float* Sw, float* heap,
                                                  float* thr, long long* ids, long n, long long id_base, int w, int lane) {
    constexpr int rs = KNN_RS;
    constexpr int PIECES = 2 * KNN_DT / GS_NW, SPP = KNN_KSTEPS / PIECES;  // pieces per wave, k-steps per piece
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
        if (s % SPP == 0) knn_fetch_piece<GS_NW>(db, t + 1, N, d, nxt, w, lane, s / SPP);
        __builtin_amdgcn_sched_barrier(0);  // keep the reads ahead of this k-step's MFMAs
        mma16<BF>(acc[0], qf[s], bq[s % 3][0]);
        mma16<BF>(acc[1], qf[s], bq[s % 3][1]);
    }
    // ---- acc[j][r] = <query first + 16 w + 4 lg + r, group row 32 t + 16 j + lr>
    const bool c0 = t * KNN_DT + lr < N, c1 = t * KNN_DT + 16 + lr < N;
    // bal[j][r]: lanes whose value may enter the list of its row (thr is +INF for query rows past n)
    unsigned long long bal[2][4];
    unsigned long long any = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const float tv = thr[w * 16 + 4 * lg + r];
        bal[0][r] = __ballot(c0 && acc[0][r] > tv);
        bal[1][r] = __ballot(c1 && acc[1][r] > tv);
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
        const long qrow = first + qi;
        if (cols && qrow < n) {
            float* h = heap + qi * hs;
            long long* gi = ids + qrow * k;
            float tr = thr[qi];
            const float* row = Sw + lane * KNN_SPAD;
            while (cols) {
                const int c = __builtin_ctz(cols);
                cols &= cols - 1;
                const float v = row[c];
                if (v > tr) {
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
                    // several slots hold `lo`: the largest id among them is the worst pair (empty slots, -INF, are all alike)
                    if (lo2 == lo && lo != -INFINITY) {
                        long long worst = gi[at];
                        for (int j = at + 1; j < k; j++)
                            if (h[j] == lo) {
                                const long long o = gi[j];
                                if (o > worst) { worst = o; at = j; }
                            }
                    }
                    h[at] = v;
                    gi[at] = id_base + t * KNN_DT + c;
                    tr = fminf(v, lo2);
                }
            }
            thr[qi] = tr;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One workgroup = 4 waves x 16 query rows = 64 queries of ONE group.  LDS as k_knn_search: two database tiles
// [KNN_DT][2064 B], per-wave similarity scratch, per-row kept values (unsorted, their minimum cached in thr[]).
// q_off / db_off [n_groups + 1], tab [gridDim.x]; q [q_off[n_groups]][d], sims / ids [q_off[n_groups]][k].
template <bool BF, typename QE>
__global__ __launch_bounds__(64 * GS_NW, 1) void k_knn_search_groups(const typename QE::storage* __restrict__ q_all,
                                                                     const uint16_t* __restrict__ db_all, int d, int k,
                                                                     const long long* __restrict__ q_off,
                                                                     const long long* __restrict__ db_off,
                                                                     const GroupBlock* __restrict__ tab, float* sims_all,
                                                                     long long* ids_all) {
    // (two tile buffers as two LDS objects, see k_knn_mean)
    __shared__ __attribute__((aligned(16))) char tile0[KNN_DT * KNN_RS];
    __shared__ __attribute__((aligned(16))) char tile1[KNN_DT * KNN_RS];
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NW = GS_NW, QT = 16 * NW, NT = 64 * NW;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    // ---- the group's view (workgroup-uniform)
    const GroupBlock gb = tab[blockIdx.x];
    const long long q0 = q_off[gb.group], db0 = db_off[gb.group];
    const long n = (long)(q_off[gb.group + 1] - q0), N = (long)(db_off[gb.group + 1] - db0);
    const long first = (long)gb.blk * QT;
    const typename QE::storage* q = q_all + q0 * (long long)d;
    const uint16_t* db = db_all + db0 * (long long)d;
    float* sims = sims_all + q0 * (long long)k;
    long long* ids = ids_all + q0 * (long long)k;
    const long long id_base = db0;

    float* S = reinterpret_cast<float*>(smem);                   // [NW][16][KNN_SPAD]
    const int k4 = (k + 3) & ~3, hs = k4 + 4;                    // list stride: 16-byte groups + one group of padding
    float* heap = S + NW * 16 * KNN_SPAD;                        // [QT][hs]: k kept values, +INF in the slots past k
    float* thr = heap + QT * hs;                                 // [QT]

    // ---- query rows -> unit norm -> MFMA A-fragments (as k_knn_search: the similarities are defined there)
    uint4 qf[KNN_KSTEPS];
    {
        const long qrow = first + w * 16 + lr;
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
    // ---- kept values: empty (-INF)
    for (int i = tid; i < QT * hs; i += NT) heap[i] = i % hs < k ? -INFINITY : INFINITY;
    for (int qi = tid; qi < QT; qi += NT) thr[qi] = first + qi < n ? -INFINITY : INFINITY;  // a row past n takes part in the MFMAs only

    const long ntiles = (N + KNN_DT - 1) / KNN_DT;
    constexpr int PIECES = 2 * KNN_DT / NW;
    if (ntiles > 0) {
#pragma unroll
        for (int i = 0; i < PIECES; i++) knn_fetch_piece<NW>(db, 0, N, d, tile0, w, lane, i);
    }
    __syncthreads();

    float* Sw = S + w * 16 * KNN_SPAD;
    // (the last tile's step fetches "tile ntiles": clamped to the group's last row, never computed)
    for (long t = 0; t < ntiles; t += 2) {
        group_search_tile<BF>(first, tile0, tile1, db, t, N, d, k, k4, hs, qf, Sw, heap, thr, ids, n, id_base, w, lane);
        __syncthreads();
        if (t + 1 >= ntiles) break;
        group_search_tile<BF>(first, tile1, tile0, db, t + 1, N, d, k, k4, hs, qf, Sw, heap, thr, ids, n, id_base, w, lane);
        __syncthreads();
    }

    // ---- sort: lane j holds pair j of a row and counts the pairs that come before it (as k_knn_search)
    __threadfence();
    __syncthreads();
    for (int rr = 0; rr < 16; rr++) {
        const int qi = w * 16 + rr;
        const long qrow = first + qi;
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

size_t group_search_smem(int k) {
    return (size_t)GS_NW * 16 * KNN_SPAD * 4 + (size_t)16 * GS_NW * (((k + 3) & ~3) + 5) * 4;
}

template <bool BF, typename QE>
int launch_group_search(svx_ctx* ctx, const void* q, const void* db, int d, int k, const long long* q_off, const long long* db_off,
                        const GroupBlock* tab, long long n_blocks, float* sims, long long* ids) {
    const size_t smem = group_search_smem(k);
    static size_t attr_set = 0;
    if (smem > attr_set) {
        SVX_HIP(ctx, hipFuncSetAttribute((const void*)k_knn_search_groups<BF, QE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        attr_set = smem;
    }
    k_knn_search_groups<BF, QE><<<dim3((unsigned)n_blocks), dim3(64 * GS_NW), smem, ctx->stream>>>(
        reinterpret_cast<const typename QE::storage*>(q), reinterpret_cast<const uint16_t*>(db), d, k, q_off, db_off, tab, sims, ids);
    SVX_LAUNCH_CHECK(ctx, "k_knn_search_groups");
    return SVX_OK;
}

}  // namespace

extern "C" int svx_knn_search_groups(svx_ctx* ctx, const void* queries, int q_dtype, const void* db, int db_dtype, int d, int k,
                                     const int64_t* q_off, const int64_t* db_off, int n_groups, float* sims, int64_t* ids) {
    if (!ctx) return svx_fail(nullptr, SVX_ERR_ARG, "svx_knn_search_groups: ctx is NULL");
    NEED(ctx, n_groups >= 0, "svx_knn_search_groups: negative n_groups (%d)", n_groups);
    NEED(ctx, q_off && db_off, "svx_knn_search_groups: null offset array");
    NEED(ctx, db_dtype == SVX_F16 || db_dtype == SVX_BF16, "svx_knn_search_groups: the database is kept in fp16 or bf16 (got dtype %d)", db_dtype);
    NEED(ctx, q_dtype == SVX_F32 || q_dtype == SVX_F16 || q_dtype == SVX_BF16, "svx_knn_search_groups: unknown query dtype %d", q_dtype);
    NEED(ctx, k >= 1 && k <= KNN_KMAX, "svx_knn_search_groups: k = %d, supported 1..%d", k, KNN_KMAX);
    NEED(ctx, d > 0 && d % 32 == 0 && d <= 32 * KNN_KSTEPS, "embedding dimension %d: must be a positive multiple of 32, at most %d", d,
         32 * KNN_KSTEPS);
    NEED(ctx, q_off[0] == 0 && db_off[0] == 0, "svx_knn_search_groups: the offsets start at %lld and %lld, not at 0", (long long)q_off[0],
         (long long)db_off[0]);
    const long long QT = 16 * GS_NW;
    long long n_blocks = 0;
    for (int g = 0; g < n_groups; g++) {
        NEED(ctx, q_off[g + 1] >= q_off[g] && db_off[g + 1] >= db_off[g], "svx_knn_search_groups: the offsets decrease at group %d", g);
        n_blocks += ((long long)(q_off[g + 1] - q_off[g]) + QT - 1) / QT;
        NEED(ctx, n_blocks <= 0x7fffffffLL, "svx_knn_search_groups: the groups need 2^31 or more workgroups");
    }
    const long long n = q_off[n_groups], n_db = db_off[n_groups];
    NEED(ctx, (n == 0 || (queries && sims && ids)) && (n_db == 0 || db), "svx_knn_search_groups: null argument");
    if (n_blocks == 0) return SVX_OK;
    // ---- post-processing scratch: [q_off][db_off][workgroup table], all of it uploaded
    const size_t b_off = up256((size_t)(n_groups + 1) * sizeof(long long)), b_tab = up256((size_t)n_blocks * sizeof(GroupBlock));
    const size_t b_up = 2 * b_off + b_tab;
    char *pin, *dev;
    int rc = svxl_scratch_begin(ctx, "svx_knn_search_groups", b_up, b_up, &pin, &dev);
    if (rc) return rc;
    memcpy(pin, q_off, (size_t)(n_groups + 1) * sizeof(long long));
    memcpy(pin + b_off, db_off, (size_t)(n_groups + 1) * sizeof(long long));
    GroupBlock* ht = reinterpret_cast<GroupBlock*>(pin + 2 * b_off);
    long long at = 0;
    for (int g = 0; g < n_groups; g++) {
        const long long nb = ((long long)(q_off[g + 1] - q_off[g]) + QT - 1) / QT;
        for (long long b = 0; b < nb; b++) {
            ht[at].group = g;
            ht[at].blk = (int)b;
            at++;
        }
    }
    rc = svxl_scratch_upload(ctx, b_up);
    if (rc) return rc;
    const long long* dq = reinterpret_cast<const long long*>(dev);
    const long long* dd = reinterpret_cast<const long long*>(dev + b_off);
    const GroupBlock* dt = reinterpret_cast<const GroupBlock*>(dev + 2 * b_off);
    const bool bf = db_dtype == SVX_BF16;
    long long* gi = reinterpret_cast<long long*>(ids);
    switch (q_dtype) {
    case SVX_F32:
        return bf ? launch_group_search<true, ElemF32>(ctx, queries, db, d, k, dq, dd, dt, n_blocks, sims, gi)
                  : launch_group_search<false, ElemF32>(ctx, queries, db, d, k, dq, dd, dt, n_blocks, sims, gi);
    case SVX_F16:
        return bf ? launch_group_search<true, ElemF16>(ctx, queries, db, d, k, dq, dd, dt, n_blocks, sims, gi)
                  : launch_group_search<false, ElemF16>(ctx, queries, db, d, k, dq, dd, dt, n_blocks, sims, gi);
    default:
        return bf ? launch_group_search<true, ElemBF16>(ctx, queries, db, d, k, dq, dd, dt, n_blocks, sims, gi)
                  : launch_group_search<false, ElemBF16>(ctx, queries, db, d, k, dq, dd, dt, n_blocks, sims, gi);
    }
}
