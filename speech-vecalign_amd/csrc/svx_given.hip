// svx_given.hip -- svx_score_alignments: price alignments the caller GIVES with the normalisers, the deletion penalty, the
// band and the type set of the last svx_align_batch / svx_align_around call (include/svx.h; gfx950 only).
//
// The grid is flat over chunks of SVX_GV_CHUNK rows of ONE pair, a host-built table maps chunk -> (pair, first row) and the
// chunks of a pair are consecutive workgroups: the rows of a path are neighbours in memory, so are the candidate rows they
// name.  The row COUNT of a pair is only known on the device, so the table covers the pair's `cap` rows and a chunk past
// the count returns at once.
//   k_given_rows   one workgroup per chunk.  Every thread classifies one row (include/svx.h: PRICED, DELETION, WIDE,
//                  INVALID, OFF_TYPE), checks that it starts where its predecessor ended -- the rows of the chunk go
//                  through LDS, the predecessor of the chunk's first row is one more 16-byte load -- and tests the node
//                  at its end against the band.  Then every wave prices the PRICED rows among its 64, one row at a time:
//                  16 bytes per lane per load, the pieces of both candidate rows in flight before the first FMA, the lane's
//                  elements added in index order, the wave reduction of svx_common.h, and the double expression of the
//                  level-0 band-cost kernel (raw dot x the two inverse norms lev[0].inv, which the call's arena still
//                  holds).  The workgroup writes the rows' scores, and per chunk the sum of its costs in row order and
//                  seven counts.
//   k_given_pairs  one workgroup per pair: the chunk sums in chunk order, the counts, node 0, then total and report.
// A row that is not PRICED is never used to form an address.  Vector stores only; nothing here waits for the host.
// (The chunk table is this file's own: svx_alignrows.hip sizes its table by n + m + 2 rows of an svx_pair, and its
// ranking helpers compact rows, which nothing here needs -- a wave walks the set bits of its ballot instead.)
#include <vector>

#include "svx_common.h"
#include "svx_slab.h"   // cost_formula: the level-0 band-cost kernel's expression

#define SVX_GV_CHUNK 256
#define SVX_GV_STEP 4   // 16-byte pieces per lane and side in flight

namespace {

struct GivenPair {
    const void* v[2];       // [k][n][d] candidate tensors of the call
    const float* nrm[2];    // [k][n] n0 / n1
    const float* inv[2];    // [k][n] 1/(||row|| + 1e-5)
    const double* pen;      // the level-0 deletion penalty
    const int* boff_out;    // [path_len + 2]
    const int* path_len;
    const int* status;      // the aligner's info[1] of the pair
    const int* rows;        // [cap][4] the given rows; null: the pair is skipped
    const int* info;        // [2]
    double* scores;         // [cap] or null
    double* total;          // [2]
    int* report;            // [8]
    int n, m, k0, k1;
    int cap;
    int first_chunk;        // the pair's first entry of the chunk table
};

struct GivenChunk {
    int pair, first;
};

struct GivenPart {          // what one chunk adds to its pair
    double sum;             // the costs of its PRICED rows, added in row order
    int priced, dels, wide, invalid, off_type, outside, breaks, pad;
};

enum { GV_PRICED = 0, GV_DEL = 1, GV_WIDE = 2, GV_INVALID = 3 };

// the given rows are usable: the aligner's call and the giver both report success, and the count fits the buffer
__device__ __forceinline__ bool given_ok(const GivenPair& P, int& cnt) {
    cnt = gld(P.info);
    return gld(P.status) == 0 && gld(P.info + 1) == 0 && cnt >= 0 && cnt <= P.cap;
}

// include/svx.h: node (x, y) is OUTSIDE
__device__ __forceinline__ bool node_outside(const GivenPair& P, long long x, long long y, int a_out, int B) {
    if (x < 0 || x > P.n || y < 0 || y > P.m) return true;
    const long long a = x + y;
    if (a >= a_out) return true;
    const long long b = y - (long long)gld(P.boff_out + a);
    return b < 0 || b >= B;
}

// <x, y> of two candidate rows of `pieces` 16-byte pieces each, by one wave: lane l holds pieces l, l + 64, ...
template <typename E>
__device__ __forceinline__ float wave_dot(const typename E::storage* xr, const typename E::storage* yr, int pieces, int lane) {
    float acc = 0.f;
    for (int p0 = 0; p0 < pieces; p0 += SVX_GV_STEP * SVX_WAVE) {
        uint4 vx[SVX_GV_STEP], vy[SVX_GV_STEP];
#pragma unroll
        for (int u = 0; u < SVX_GV_STEP; u++) {
            const int p = p0 + u * SVX_WAVE + lane;
            vx[u] = vy[u] = make_uint4(0, 0, 0, 0);
            if (p < pieces) {
                vx[u] = gld16(xr + (size_t)p * E::VEC);
                vy[u] = gld16(yr + (size_t)p * E::VEC);
            }
        }
#pragma unroll
        for (int u = 0; u < SVX_GV_STEP; u++) {
            float a[E::VEC], b[E::VEC];
            decode_piece<E>(vx[u], a);
            decode_piece<E>(vy[u], b);
#pragma unroll
            for (int e = 0; e < E::VEC; e++) acc = fmaf(a[e], b[e], acc);
        }
    }
    return wave_sum(acc);
}

template <typename E>
__global__ __launch_bounds__(SVX_GV_CHUNK) void k_given_rows(const GivenPair* __restrict__ pairs, const GivenChunk* __restrict__ chunks,
                                                             SvxTypes types, int B, int d, GivenPart* __restrict__ parts) {
    using S = typename E::storage;
    __shared__ int4 srow[SVX_GV_CHUNK + 1];       // [0]: the predecessor of the chunk's first row
    __shared__ double scost[SVX_GV_CHUNK];
    __shared__ int scnt[SVX_GV_CHUNK / SVX_WAVE][8];
    const GivenChunk c = chunks[blockIdx.x];
    const GivenPair P = pairs[c.pair];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int cnt;
    if (!given_ok(P, cnt) || c.first >= cnt) return;   // (uniform) k_given_pairs reads no part of such a chunk
    const int a_out = gld(P.path_len) + 2;
    const int r = c.first + tid;
    const bool have = r < cnt;
    int4 me = make_int4(0, 0, 0, 0);
    if (have) {
        const uint4 v = gld16(P.rows + 4 * (size_t)r);
        me = make_int4((int)v.x, (int)v.y, (int)v.z, (int)v.w);
    }
    srow[tid + 1] = me;
    if (tid == 0) {
        int4 pr = make_int4(0, 0, 0, 0);           // row 0 follows the node (0, 0)
        if (c.first > 0) {
            const uint4 v = gld16(P.rows + 4 * (size_t)(c.first - 1));
            pr = make_int4((int)v.x, (int)v.y, (int)v.z, (int)v.w);
        }
        srow[0] = pr;
    }
    __syncthreads();
    // ---- the row's class, its chain link and its node
    int cls = GV_INVALID;
    bool off_type = false, outside = false, brk = false;
    if (have) {
        const long long xs = me.x, xl = me.y, ys = me.z, yl = me.w;
        const bool in_range = xs >= 0 && xl >= 0 && ys >= 0 && yl >= 0 && xs + xl <= P.n && ys + yl <= P.m;
        if (in_range) {
            if (xl >= 1 && yl >= 1) cls = (xl > P.k0 || yl > P.k1) ? GV_WIDE : GV_PRICED;
            else if (xl + yl == 1) cls = GV_DEL;
        }
        if (cls == GV_PRICED) {
            off_type = true;
            for (int t = 0; t < types.n; t++)
                if (types.x[t] == me.y && types.y[t] == me.w) off_type = false;
        }
        const int4 pr = srow[tid];
        brk = xs != (long long)pr.x + pr.y || ys != (long long)pr.z + pr.w;
        if (r == cnt - 1 && (xs + xl != P.n || ys + yl != P.m)) brk = true;
        outside = node_outside(P, xs + xl, ys + yl, a_out, B);
    }
    // ---- the wave prices the PRICED rows among its 64, in row order
    float cost = 0.f;
    unsigned long long todo = __ballot(have && cls == GV_PRICED);
    const int pieces = d / E::VEC;
    while (todo) {
        const int j = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int4 a = srow[w * SVX_WAVE + j + 1];
        const size_t xrow = (size_t)(a.y - 1) * P.n + a.x + a.y - 1, yrow = (size_t)(a.w - 1) * P.m + a.z + a.w - 1;
        const float dot = wave_dot<E>(reinterpret_cast<const S*>(P.v[0]) + xrow * d, reinterpret_cast<const S*>(P.v[1]) + yrow * d, pieces, lane);
        const float sumx = dot * gld(P.inv[0] + xrow) * gld(P.inv[1] + yrow);
        const float cj = cost_formula(sumx, a.y, a.w, gld(P.nrm[0] + xrow), gld(P.nrm[1] + yrow));
        if (lane == j) cost = cj;
    }
    if (have && P.scores) {
        double s = __builtin_nan("");
        if (cls == GV_DEL) s = 0.0;
        else if (cls == GV_PRICED) s = (double)fmaxf(cost, 0.f) / (double)(me.y * me.w);
        gst(P.scores + r, s);
    }
    scost[tid] = cls == GV_PRICED && have ? (double)cost : 0.0;
    const bool flags[7] = {have && cls == GV_PRICED, have && cls == GV_DEL, have && cls == GV_WIDE, have && cls == GV_INVALID,
                           off_type, outside, brk};
#pragma unroll
    for (int f = 0; f < 7; f++) {
        const int k = __popcll(__ballot(flags[f]));
        if (lane == 0) scnt[w][f] = k;
    }
    __syncthreads();
    if (tid == 0) {
        GivenPart* out = parts + blockIdx.x;
        const int rows = cnt - c.first < SVX_GV_CHUNK ? cnt - c.first : SVX_GV_CHUNK;
        double sum = 0.0;
        for (int i = 0; i < rows; i++) sum += scost[i];
        int k[8];
#pragma unroll
        for (int f = 0; f < 7; f++) k[f] = scnt[0][f] + scnt[1][f] + scnt[2][f] + scnt[3][f];
        gst(&out->sum, sum);
        gst(&out->priced, k[0]); gst(&out->dels, k[1]); gst(&out->wide, k[2]); gst(&out->invalid, k[3]);
        gst(&out->off_type, k[4]); gst(&out->outside, k[5]); gst(&out->breaks, k[6]);
    }
}

__global__ __launch_bounds__(256) void k_given_pairs(const GivenPair* __restrict__ pairs, const GivenPart* __restrict__ parts, int B) {
#pragma clang fp contract(off)
    __shared__ double ssum[256];
    __shared__ int scnt[4][8];
    const GivenPair P = pairs[blockIdx.x];
    if (!P.rows) return;   // (uniform) a skipped pair: nothing of it is written
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int cnt;
    if (!given_ok(P, cnt)) {
        if (tid == 0) {
            gst16(P.report, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
            gst16(P.report + 4, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
            gst(P.total, __builtin_nan(""));
            gst(P.total + 1, __builtin_nan(""));
        }
        return;
    }
    const int n_chunks = (cnt + SVX_GV_CHUNK - 1) / SVX_GV_CHUNK;
    double sum = 0.0;   // thread 0's
    int k[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int base = 0; base < n_chunks; base += 256) {
        const int i = base + tid;
        double s = 0.0;
        if (i < n_chunks) {
            const GivenPart* q = parts + P.first_chunk + i;
            s = gld(&q->sum);
            k[0] += gld(&q->priced); k[1] += gld(&q->dels); k[2] += gld(&q->wide); k[3] += gld(&q->invalid);
            k[4] += gld(&q->off_type); k[5] += gld(&q->outside); k[6] += gld(&q->breaks);
        }
        __syncthreads();   // (ssum may still be read from the stretch before)
        ssum[tid] = s;
        __syncthreads();
        if (tid == 0) {
            const int have = n_chunks - base < 256 ? n_chunks - base : 256;
            for (int j = 0; j < have; j++) sum += ssum[j];
        }
    }
#pragma unroll
    for (int f = 0; f < 7; f++) {
        int v = k[f];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) scnt[w][f] = v;
    }
    __syncthreads();
    if (tid == 0) {
        int t[7];
#pragma unroll
        for (int f = 0; f < 7; f++) t[f] = scnt[0][f] + scnt[1][f] + scnt[2][f] + scnt[3][f];
        if (node_outside(P, 0, 0, gld(P.path_len) + 2, B)) t[5]++;
        const int complete = cnt > 0 && t[6] == 0 && t[3] == 0 ? 1 : 0;
        const double pen = gld(P.pen);
        gst16(P.report, (uint32_t)cnt, (uint32_t)t[0], (uint32_t)t[1], (uint32_t)t[2]);
        gst16(P.report + 4, (uint32_t)t[3], (uint32_t)t[4], (uint32_t)t[5], (uint32_t)complete);
        gst(P.total, sum + pen * (double)t[1]);
        gst(P.total + 1, pen);
    }
}

}  // namespace

extern "C" int svx_score_alignments(svx_ctx* ctx, const svx_given* given, int n_pairs) {
    if (!ctx) return svx_fail(nullptr, SVX_ERR_ARG, "svx_score_alignments: ctx is NULL");
    NEED(ctx, given, "svx_score_alignments: given is NULL");
    NEED(ctx, n_pairs >= 0, "svx_score_alignments: negative n_pairs");
    long long n_chunks = 0;
    for (int p = 0; p < n_pairs; p++) {
        const svx_given& g = given[p];
        if (!g.rows) continue;
        NEED(ctx, g.info && g.total && g.report, "svx_score_alignments: pair %d: null info / total / report", p);
        NEED(ctx, g.cap >= 0, "svx_score_alignments: pair %d: cap %d", p, g.cap);
        NEED(ctx, aligned16(g.report), "svx_score_alignments: pair %d: report must be 16-byte aligned", p);
        NEED(ctx, aligned16(g.rows), "svx_score_alignments: pair %d: rows must be 16-byte aligned", p);
        n_chunks += ((long long)g.cap + SVX_GV_CHUNK - 1) / SVX_GV_CHUNK;
    }
    NEED(ctx, n_chunks <= 0x7fffffffLL, "svx_score_alignments: %lld chunks of rows", n_chunks);
    SvxLastCall lc;
    int rc = svxl_last_call(ctx, "svx_score_alignments", n_pairs, nullptr, &lc);
    if (rc) return rc;
    // ---- scratch: [descriptors][chunk table] uploaded, then [chunk parts]
    const size_t b_desc = up256((size_t)n_pairs * sizeof(GivenPair)), b_tab = up256((size_t)n_chunks * sizeof(GivenChunk));
    const size_t b_part = up256((size_t)n_chunks * sizeof(GivenPart));
    const size_t b_up = b_desc + b_tab;
    char *pin, *dev;
    rc = svxl_scratch_begin(ctx, "svx_score_alignments", b_up, b_up + b_part, &pin, &dev);
    if (rc) return rc;
    GivenPair* hp = reinterpret_cast<GivenPair*>(pin);
    GivenChunk* hc = reinterpret_cast<GivenChunk*>(pin + b_desc);
    long long at = 0;
    for (int p = 0; p < n_pairs; p++) {
        const SvxPairDev& P = lc.pair(p);
        const SvxLevel& Lv = P.lev[0];
        const svx_given& g = given[p];
        GivenPair& r = hp[p];
        for (int s = 0; s < 2; s++) { r.v[s] = P.v[s]; r.nrm[s] = Lv.nrm[s]; r.inv[s] = Lv.inv[s]; }
        r.pen = Lv.pen;
        r.boff_out = Lv.boff_out;
        r.path_len = Lv.path_len;
        r.status = P.status;
        r.rows = g.rows; r.info = g.info; r.scores = g.scores; r.total = g.total; r.report = g.report;
        r.n = Lv.n[0]; r.m = Lv.n[1]; r.k0 = P.K[0]; r.k1 = P.K[1];
        r.cap = g.rows ? g.cap : 0;
        r.first_chunk = (int)at;
        for (int first = 0; first < r.cap; first += SVX_GV_CHUNK) {
            hc[at].pair = p;
            hc[at].first = first;
            at++;
        }
    }
    rc = svxl_scratch_upload(ctx, b_up);
    if (rc) return rc;
    const GivenPair* dp = reinterpret_cast<const GivenPair*>(dev);
    const GivenChunk* dc = reinterpret_cast<const GivenChunk*>(dev + b_desc);
    GivenPart* dparts = reinterpret_cast<GivenPart*>(dev + b_up);
    hipStream_t st = ctx->stream;
    if (n_chunks > 0) {
        const dim3 grid((unsigned)n_chunks), block(SVX_GV_CHUNK);
        if (lc.dtype == SVX_F32) k_given_rows<ElemF32><<<grid, block, 0, st>>>(dp, dc, *lc.types, lc.band, lc.d, dparts);
        else if (lc.dtype == SVX_F16) k_given_rows<ElemF16><<<grid, block, 0, st>>>(dp, dc, *lc.types, lc.band, lc.d, dparts);
        else k_given_rows<ElemBF16><<<grid, block, 0, st>>>(dp, dc, *lc.types, lc.band, lc.d, dparts);
        SVX_LAUNCH_CHECK(ctx, "k_given_rows");
    }
    k_given_pairs<<<dim3((unsigned)n_pairs), dim3(256), 0, st>>>(dp, dparts, lc.band);
    SVX_LAUNCH_CHECK(ctx, "k_given_pairs");
    return SVX_OK;
}
