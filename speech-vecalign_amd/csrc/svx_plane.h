// svx_plane.h -- what svx_slack.hip and svx_alt.hip share: the per-pair descriptor of their kernels and the device helpers
// that read the two band planes of a pair, F (the stored forward csum) and Bk (the backward plane); DESIGN.md 6d, 6e.
// Device helpers and the descriptor only: the kernels stay in their .hip files.  gfx950 only.
#pragma once
#include "svx_common.h"

constexpr int MAXSTEP = 200;   // make_types: type sizes are at most 100 a side (the per-wave band-offset table has 2 * MAXSTEP entries)

// One pair, for every kernel of both files (each takes `const PlanePair* pairs, PlanePair one, int use_one`: the batch
// entries pass an array in the post-processing scratch, the per-op entries the one record by value).
struct PlanePair {
    const float* costs;
    const int* boff_in;         // [A]
    const int* path_len;        // device A (the pipeline), or null: A below
    const double* pen_dev;      // device penalty (the pipeline), or null: pen below
    const int* status;          // the aligner's info[1] of the pair, or null
    const double* csum;         // [A+2][B] forward plane
    double* bsum;               // [A+2][B] backward plane (written by the sweep only); null: the sweep skips the pair
    const int* xp;              // int32 back-pointers, or null when bpk is given
    const int* yp;
    const unsigned char* bpk;   // packed back-pointers xp << 4 | yp, 0xFF = none
    const int* rows;            // [cap][4]
    const int* n_rows;          // [1]
    int* table;                 // [A+2][2] scratch: (cell, node number) of the path node on each diagonal
    double* slack;              // [cap] or null; null: k_path_slack skips the pair
    int* edge;                  // [cap][4]; null: k_row_alt and k_given_regret skip the pair
    int* span;                  // [cap][4]
    int* detour;                // [cap][K][4] or null: edges only
    double* dscores;            // [cap][K] or null
    const int* given;           // [given_cap][4] or null
    const int* given_info;      // [2]
    double* regret;             // [given_cap]
    int* summary;               // [4] or null (per-op entry)
    double pen;
    int A, xs, ys, cap, given_cap, pad;
};

struct PlaneGeo {
    const float* costs;
    const int* boff_in;
    const double* csum;
    double* bsum;
    int A, B, T, atb, xs, ys;
    double pen;
};

// false: the aligner failed the pair, or it has no diagonals
__device__ __forceinline__ bool plane_geo(const PlanePair& P, const SvxTypes& ty, int B, int atb, PlaneGeo* g) {
    if (P.status && gld(P.status) != 0) return false;
    g->A = P.path_len ? gld(P.path_len) : P.A;
    if (g->A <= 0) return false;
    g->costs = P.costs;
    g->boff_in = P.boff_in;
    g->csum = P.csum;
    g->bsum = P.bsum;
    g->B = B;
    g->T = ty.n;
    g->atb = atb;
    g->xs = P.xs;
    g->ys = P.ys;
    g->pen = P.pen_dev ? gld(P.pen_dev) : P.pen;
    return true;
}

// both cost layouts: [A][T][B] (atb, the fused pipeline) and [T][A][B] (per-op)
__device__ __forceinline__ size_t plane_cost_index(const PlaneGeo& g, int t, int a, int b) {
    return g.atb ? ((size_t)a * g.T + t) * g.B + b : ((size_t)t * g.A + a) * g.B + b;
}
// b_offset_out[a], 0 <= a < A + 2
__device__ __forceinline__ int plane_bout(const int* boff_in, int a) { return a < 2 ? gld(boff_in) : gld(boff_in + (a - 2)) + 1; }

// total = F(end); +inf when the end node is no band cell
__device__ __forceinline__ double plane_total(const PlaneGeo& g) {
    const long long xs = g.xs, ys = g.ys, Aout = (long long)g.A + 2;
    if (xs >= 0 && ys >= 0 && xs + ys < Aout) {
        const long long be = ys - plane_bout(g.boff_in, (int)(xs + ys));
        if (be >= 0 && be < g.B) return gld(g.csum + ((size_t)(xs + ys) * g.B + be));
    }
    return __builtin_inf();
}

// Is the row an edge of the search space?  Range checks, the move is in the list (-> *t, its first index), both nodes are
// band cells (-> *bu, *bv).  No address is formed before the ranges are known to hold.
__device__ __forceinline__ bool plane_is_edge(const PlaneGeo& g, const SvxTypes& ty, uint4 rv, int* t, int* bu, int* bv) {
    const long long x0 = (int)rv.x, xl = (int)rv.y, y0 = (int)rv.z, yl = (int)rv.w;
    const long long Aout = (long long)g.A + 2, c = x0 + y0;
    if (!(x0 >= 0 && xl >= 0 && y0 >= 0 && yl >= 0 && x0 + xl <= g.xs && y0 + yl <= g.ys && xl + yl >= 1 && c + xl + yl < Aout)) return false;
    int tt = -1;
    for (int k = ty.n + 1; k >= 0; k--)
        if (ty.x[k] == xl && ty.y[k] == yl) tt = k;
    if (tt < 0) return false;
    const long long b0 = y0 - plane_bout(g.boff_in, (int)c);
    const long long b1 = y0 + yl - plane_bout(g.boff_in, (int)(c + xl + yl));
    if (!(b0 >= 0 && b0 < g.B && b1 >= 0 && b1 < g.B)) return false;
    *t = tt; *bu = (int)b0; *bv = (int)b1;
    return true;
}

// a wave's LDS writes become visible to its own lanes
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The rows a row kernel walks (uniform over the workgroup).  With a summary (the batch entries) a failed pair, or a count
// outside [0, cap], gets four -1 words and no rows; without (per-op) a failed pair writes nothing and the count is clamped.
__device__ __forceinline__ bool plane_row_count(const PlanePair& P, bool ok_pair, int* count) {
    int cnt = ok_pair ? gld(P.n_rows) : -1;
    if (P.summary) {
        if (cnt < 0 || cnt > P.cap) {
            if (threadIdx.x == 0) gst16(P.summary, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
            return false;
        }
    } else {
        if (!ok_pair) return false;
        cnt = cnt < 0 ? 0 : (cnt > P.cap ? P.cap : cnt);
    }
    *count = cnt;
    return true;
}

// The summary of a pair: lane 0 of every wave hands in its N counts, thread 0 writes (cnt, their sums, 0 ...).
template <int N, int WAVES>
__device__ __forceinline__ void plane_summary(int (&scnt)[WAVES][N], int* summary, int cnt, int c0, int c1, int c2) {
    const int tid = threadIdx.x, c[3] = {c0, c1, c2};
    if ((tid & 63) == 0)
        for (int k = 0; k < N; k++) scnt[tid >> 6][k] = c[k];
    __syncthreads();
    if (tid != 0) return;
    int s[3] = {0, 0, 0};
    for (int u = 0; u < WAVES; u++)
        for (int k = 0; k < N; k++) s[k] += scnt[u][k];
    gst16(summary, (uint32_t)cnt, (uint32_t)s[0], (uint32_t)s[1], (uint32_t)s[2]);
}

// The cut scan of one row, by one wave (every argument wave-uniform).  The row is an edge (plane_is_edge) that starts on
// diagonal ci in cell bui with move (xli, yli).  The cut behind ci is crossed by the edges into diagonals ci + 1 .. ci + maxstep:
// lanes take (diagonal, cell) targets v in ascending order and loop over the moves in list order that reach back to ci or
// further, and price (F(u) + w) + Bk(v) from three resident reads; the row's own edge is left out.  -> the minimum, in every
// lane.  KEYED: also the order key  item * (T + 2) + move  of the first candidate in that order to attain it (a lane's first
// strictly smaller candidate is its smallest key; the wave arg-min is on (cand, key)).  `bo`, the wave's table of 2 * MAXSTEP
// ints, is left holding b_offset_out of diagonals ci - maxstep + 1 .. ci + maxstep (0 outside the plane).
template <bool KEYED>
__device__ __forceinline__ double cut_scan(const PlaneGeo& g, const SvxTypes& ty, int* bo, int ci, int bui, int xli, int yli,
                                           unsigned long long* key_out) {
    const int lane = threadIdx.x & 63;
    const int B = g.B, T = ty.n, NTt = ty.n + 2, Aout = g.A + 2;
    const int ms = ty.maxstep, dbase = ci - ms + 1;
    __builtin_amdgcn_wave_barrier();   // (the row before may still be reading the table)
    for (int k = lane; k < 2 * ms; k += SVX_WAVE) {
        const long long a = (long long)dbase + k;
        bo[k] = (a >= 0 && a < Aout) ? plane_bout(g.boff_in, (int)a) : 0;
    }
    wave_lds_sync();
    double alt = __builtin_inf();
    unsigned long long key = ~0ull;
    const int items = ms * B;
    for (int it = lane; it < items; it += SVX_WAVE) {
        const int dv = it / B + 1, bv = it - (dv - 1) * B;
        const long long avl = (long long)ci + dv;
        if (avl >= Aout) continue;
        const int av = (int)avl;
        const int vy = bv + bo[av - dbase], vx = av - vy;
        if (vx < 0 || vx > g.xs || vy < 0 || vy > g.ys) continue;
        const double bk = gld(g.bsum + ((size_t)av * B + bv));
        for (int t = 0; t < NTt; t++) {
            const int xo = ty.x[t], yo = ty.y[t], st = xo + yo;
            if (st < dv) continue;             // the edge starts behind the cut
            const int au = av - st, ux = vx - xo, uy = vy - yo;
            if (au < 0 || ux < 0 || uy < 0) continue;
            const int bp = uy - bo[au - dbase];
            if (bp < 0 || bp >= B) continue;
            if (au == ci && bp == bui && xo == xli && yo == yli) continue;   // the row's own edge
            const double wgt = t < T ? (double)gld(g.costs + plane_cost_index(g, t, av - 2, bv)) : g.pen;
            const double cand = (gld(g.csum + ((size_t)au * B + bp)) + wgt) + bk;
            if (cand < alt) {   // (a lane meets its keys in ascending order)
                alt = cand;
                if (KEYED) key = (unsigned long long)it * (unsigned)NTt + (unsigned)t;
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double oa = __shfl_xor(alt, o, SVX_WAVE);
        if (KEYED) {
            const unsigned long long ok = __shfl_xor(key, o, SVX_WAVE);
            if (oa < alt || (oa == alt && ok < key)) { alt = oa; key = ok; }
        } else {
            alt = oa < alt ? oa : alt;
        }
    }
    if (KEYED) *key_out = key;
    return alt;
}
