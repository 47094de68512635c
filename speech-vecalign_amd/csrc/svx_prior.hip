// svx_prior.hip -- band search around a prior alignment (include/svx.h: svx_align_around, svx_time_prior; gfx950 only).
//
//   k_prior_ingest  one workgroup per pair of a svx_align_around batch: validates the caller's rows (block reduction of
//                   the two length sums and of the "bad row" flag), appends the remainder row and copies the lengths into
//                   lev[0].align / n_align -- where k_init_batch seeds the covering block of the straight search, so the
//                   search-path, band-cost, DP and traceback kernels run unchanged.
//   k_prior_width   one workgroup per pair: the same validation, then the width_over2 at which the band around the
//                   prior's search path covers every block of the prior (svx_prior_width).
//   k_time_prior    one workgroup per pair: a prior from the segments' timestamps.  A segment is the HEAD of a run when its
//                   window differs from its predecessor's.  A window present on the source side gives the row of its
//                   source head; a window present on the target side only gives the row of its target head.  The rank of a
//                   row is the number of row-giving heads in front of it: those of its own side (block scan) plus those of
//                   the other side below its window (binary search, the windows of a side never decrease).
// Plain C++ with vector stores; nothing here is on the hot path of a step (a few microseconds per batch).
#include <string.h>

#include "svx_common.h"

namespace {

// Sum of v over the workgroup (256 threads), every thread gets it.  red: 4 slots of LDS.
__device__ __forceinline__ long long block_sum_ll(long long v, long long* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();  // (red may still be read from the call before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// Maximum of v (>= 0) over the workgroup, every thread gets it.
__device__ __forceinline__ int block_max_int(int v, long long* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const long long a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
    return (int)(a > b ? a : b);
}

// The ingest rules of svx_align_around in their order (include/svx.h) -> 0 with the two length sums, or the pair's
// failure code.  count, code and the result are uniform over the workgroup: every caller's branch on them is taken by
// all threads or by none.
__device__ __forceinline__ int prior_check(const int* rows, int count, int code, int cap, int n, int m, long long* red,
                                           long long* sx_out, long long* sy_out) {
    if (code != 0) return code;
    if (count < 0 || count > cap) return (int)SVX_ERR_ARG;
    long long sx = 0, sy = 0, bad = 0;
    for (int i = threadIdx.x; i < count; i += 256) {
        const int xl = gld(rows + 4 * (size_t)i + 1), yl = gld(rows + 4 * (size_t)i + 3);
        bad |= (xl < 0 || yl < 0 || (xl == 0 && yl == 0)) ? 1 : 0;
        sx += xl;
        sy += yl;
    }
    bad = block_sum_ll(bad, red);
    if (bad != 0) return (int)SVX_ERR_PATH;  // (the sums mean nothing then)
    sx = block_sum_ll(sx, red);
    sy = block_sum_ll(sy, red);
    if (sx > n || sy > m) return (int)SVX_ERR_EXTEND;
    *sx_out = sx;
    *sy_out = sy;
    return 0;
}

__global__ __launch_bounds__(256) void k_prior_ingest(const SvxPairDev* __restrict__ pairs) {
    __shared__ long long red[4];
    const SvxPairDev& P = pairs[blockIdx.x];
    const int* rows = P.prior_rows;
    const int tid = threadIdx.x;
    const int count = gld(P.prior_info), code = gld(P.prior_info + 1);
    const int n = P.lev[0].n[0], m = P.lev[0].n[1];
    long long sx = 0, sy = 0;
    const int fail = prior_check(rows, count, code, P.prior_cap, n, m, red, &sx, &sy);
    if (fail != 0) {
        if (tid == 0) gst(P.status, fail);
        return;
    }
    // every row takes at least one segment of a side, so count <= sx + sy <= n + m: the rows and the remainder fit the
    // n + m + 2 rows of lev[0].align.  The path kernel reads the lengths only (no up-sampling at level 0).
    int* dst = P.lev[0].align;
    for (int i = tid; i < count; i += 256) {
        const int xl = gld(rows + 4 * (size_t)i + 1), yl = gld(rows + 4 * (size_t)i + 3);
        gst16(dst + 4 * (size_t)i, 0u, (uint32_t)xl, 0u, (uint32_t)yl);
    }
    if (tid == 0) {
        const int rx = n - (int)sx, ry = m - (int)sy;
        int total = count;
        if (rx > 0 || ry > 0) {
            gst16(dst + 4 * (size_t)count, (uint32_t)(int)sx, (uint32_t)rx, (uint32_t)(int)sy, (uint32_t)ry);
            total++;
        }
        gst(P.lev[0].n_align, total);
    }
}

// ------------------------------------------------------------------------------ covering width
struct WidthPair {
    const int* rows;   // [cap][4]
    const int* info;   // [2]
    int* out;          // the pair's slot of width[]
    int cap, n, m, pad;
};

// width_over2 from which the band around the prior's search path holds every node of every ingested block:
// 1 + max over the rows the ingest would hand to the path kernel (remainder row included) of min(x_len, y_len), at
// least 3 (what svx_align_around raises smaller widths to); 0 for a prior the ingest would fail.
__global__ __launch_bounds__(256) void k_prior_width(const WidthPair* __restrict__ pairs) {
    __shared__ long long red[4];
    const WidthPair P = pairs[blockIdx.x];
    const int count = gld(P.info), code = gld(P.info + 1);
    long long sx = 0, sy = 0;
    if (prior_check(P.rows, count, code, P.cap, P.n, P.m, red, &sx, &sy) != 0) {
        if (threadIdx.x == 0) gst(P.out, 0);
        return;
    }
    int best = 0;
    for (int i = threadIdx.x; i < count; i += 256) {
        const int xl = gld(P.rows + 4 * (size_t)i + 1), yl = gld(P.rows + 4 * (size_t)i + 3);
        const int v = xl < yl ? xl : yl;
        best = v > best ? v : best;
    }
    best = block_max_int(best, red);
    if (threadIdx.x == 0) {
        const int rx = P.n - (int)sx, ry = P.m - (int)sy;   // the remainder row (a deletion run has min = 0)
        const int v = rx < ry ? rx : ry;
        best = v > best ? v : best;
        gst(P.out, best + 1 < 3 ? 3 : best + 1);
    }
}

// ------------------------------------------------------------------------------ time prior
struct TimePair {
    const int* f[2];   // [n][2], [m][2] (start, end) sample positions
    int* rows;         // [cap][4]
    int* info;         // [2]
    int* pre[2];       // scratch [n + 1], [m + 1]: row-giving heads in front of segment i of the side
    int n[2];
};

__device__ __forceinline__ long long floor_div(long long a, long long b) {  // b > 0
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// window of segment i of side s
__device__ __forceinline__ long long seg_window(const TimePair& P, int s, int i, long long window, long long lag) {
    const long long t = gld(P.f[s] + 2 * (size_t)i);
    if (s == 0) return floor_div(t, window);
    const long long u = t - lag;
    return floor_div(u > 0 ? u : 0, window);
}

// first segment of side s whose window is >= w (upper = false) or > w (upper = true); the windows never decrease
__device__ __forceinline__ int win_bound(const TimePair& P, int s, long long w, bool upper, long long window, long long lag) {
    int lo = 0, hi = P.n[s];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const long long wm = seg_window(P, s, mid, window, lag);
        if (upper ? wm <= w : wm < w) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_time_prior(const TimePair* __restrict__ pairs, long long window, long long lag) {
    __shared__ int wsum[4];
    __shared__ int sh_bad;
    const TimePair P = pairs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) sh_bad = 0;
    __syncthreads();
    for (int s = 0; s < 2; s++) {
        int bad = 0;
        for (int i = 1 + tid; i < P.n[s]; i += 256) bad |= gld(P.f[s] + 2 * (size_t)i) < gld(P.f[s] + 2 * (size_t)(i - 1));
        if (bad) sh_bad = 1;
    }
    __syncthreads();
    if (sh_bad) {  // uniform
        if (tid == 0) { gst(P.info, 0); gst(P.info + 1, (int)SVX_ERR_PATH); }
        return;
    }
    // row-giving heads and their exclusive prefix counts, side 0 then side 1 (a target head gives a row only when the
    // source side has no segment in its window)
    int total[2] = {0, 0};
    for (int s = 0; s < 2; s++) {
        int carry = 0;
        for (int base = 0; base < P.n[s]; base += 256) {
            const int i = base + tid;
            int v = 0;
            if (i < P.n[s]) {
                const long long wi = seg_window(P, s, i, window, lag);
                const bool head = i == 0 || seg_window(P, s, i - 1, window, lag) != wi;
                v = head ? 1 : 0;
                if (head && s == 1) {
                    const int j = win_bound(P, 0, wi, false, window, lag);
                    if (j < P.n[0] && seg_window(P, 0, j, window, lag) == wi) v = 0;
                }
            }
            int inc = v;  // inclusive scan inside the wave
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(inc, o, 64);
                if (lane >= o) inc += t;
            }
            if (lane == 63) wsum[w] = inc;
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                before += u < w ? wsum[u] : 0;
                all += wsum[u];
            }
            if (i < P.n[s]) gst(P.pre[s] + i, carry + before + (inc - v));
            carry += all;
            __syncthreads();  // wsum is rewritten by the next stretch
        }
        if (tid == 0) gst(P.pre[s] + P.n[s], carry);
        total[s] = carry;
    }
    __threadfence_block();
    __syncthreads();  // the prefix counts of both sides are visible to the whole workgroup
    // rows: at most one per segment, so total[0] + total[1] <= n + m <= cap
    for (int s = 0; s < 2; s++) {
        const int o = 1 - s;
        for (int i = tid; i < P.n[s]; i += 256) {
            if (gld(P.pre[s] + i + 1) == gld(P.pre[s] + i)) continue;  // gives no row
            const long long wi = seg_window(P, s, i, window, lag);
            const int own_end = win_bound(P, s, wi, true, window, lag);
            const int oth_lo = win_bound(P, o, wi, false, window, lag);
            const int oth_hi = s == 0 ? win_bound(P, o, wi, true, window, lag) : oth_lo;  // (a target-only window: no source segment)
            const int rank = gld(P.pre[s] + i) + gld(P.pre[o] + oth_lo);
            const int mine[2] = {i, own_end - i}, theirs[2] = {oth_lo, oth_hi - oth_lo};
            const int* x = s == 0 ? mine : theirs;
            const int* y = s == 0 ? theirs : mine;
            gst16(P.rows + 4 * (size_t)rank, (uint32_t)x[0], (uint32_t)x[1], (uint32_t)y[0], (uint32_t)y[1]);
        }
    }
    if (tid == 0) { gst(P.info, total[0] + total[1]); gst(P.info + 1, 0); }
}

}  // namespace

int svxl_prior_ingest_batch(svx_ctx* ctx, const SvxPairDev* pairs, int n_pairs) {
    if (n_pairs <= 0) return SVX_OK;
    hipLaunchKernelGGL(k_prior_ingest, dim3(n_pairs), dim3(256), 0, ctx->stream, pairs);
    SVX_LAUNCH_CHECK(ctx, "k_prior_ingest");
    return SVX_OK;
}

extern "C" int svx_time_prior(svx_ctx* ctx, const svx_pair* pairs, const svx_frames* frames, int n_pairs, int64_t window,
                              int64_t lag, const svx_prior* out) {
    if (!ctx) return svx_fail(nullptr, SVX_ERR_ARG, "svx_time_prior: ctx is NULL");
    NEED(ctx, n_pairs >= 0, "svx_time_prior: negative n_pairs");
    NEED(ctx, n_pairs == 0 || (pairs && frames && out), "svx_time_prior: null argument");
    NEED(ctx, window > 0, "svx_time_prior: window must be positive (got %lld)", (long long)window);
    NEED(ctx, lag > -(1ll << 62) && lag < (1ll << 62), "svx_time_prior: lag %lld out of range", (long long)lag);
    if (n_pairs == 0) return SVX_OK;
    size_t ints = 0;
    for (int p = 0; p < n_pairs; p++) {
        const svx_pair& q = pairs[p];
        NEED(ctx, q.n >= 0 && q.m >= 0, "svx_time_prior: pair %d: sizes n=%d m=%d", p, q.n, q.m);
        NEED(ctx, (frames[p].src || q.n == 0) && (frames[p].tgt || q.m == 0), "svx_time_prior: pair %d: null frames", p);
        NEED(ctx, out[p].rows && out[p].info, "svx_time_prior: pair %d: null output buffer", p);
        NEED(ctx, aligned16(out[p].rows), "svx_time_prior: pair %d: rows must be 16-byte aligned", p);
        NEED(ctx, (long long)out[p].cap >= (long long)q.n + q.m, "svx_time_prior: pair %d: cap %d is below n + m = %lld", p, out[p].cap,
             (long long)q.n + q.m);
        ints += (size_t)q.n + q.m + 2;
    }
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // ---- scratch: [descriptors][prefix counts]; the descriptors are uploaded
    const size_t b_up = up256((size_t)n_pairs * sizeof(TimePair)), b_all = b_up + up256(ints * sizeof(int));
    char *pin, *dev;
    int rc = svxl_scratch_begin(ctx, "svx_time_prior", b_up, b_all, &pin, &dev);
    if (rc) return rc;
    TimePair* hp = reinterpret_cast<TimePair*>(pin);
    int* pre = reinterpret_cast<int*>(dev + b_up);
    for (int p = 0; p < n_pairs; p++) {
        const svx_pair& q = pairs[p];
        TimePair& r = hp[p];
        r.f[0] = frames[p].src; r.f[1] = frames[p].tgt;
        r.rows = const_cast<int*>(out[p].rows);
        r.info = const_cast<int*>(out[p].info);
        r.n[0] = q.n; r.n[1] = q.m;
        r.pre[0] = pre;
        r.pre[1] = pre + q.n + 1;
        pre += (size_t)q.n + q.m + 2;
    }
    rc = svxl_scratch_upload(ctx, (size_t)n_pairs * sizeof(TimePair));  // (behind them the upload area is padding)
    if (rc) return rc;
    hipLaunchKernelGGL(k_time_prior, dim3(n_pairs), dim3(256), 0, st, reinterpret_cast<const TimePair*>(dev),
                       (long long)window, (long long)lag);
    SVX_LAUNCH_CHECK(ctx, "k_time_prior");
    return SVX_OK;
}

extern "C" int svx_prior_width(svx_ctx* ctx, const svx_pair* pairs, const svx_prior* priors, int n_pairs, int32_t* width) {
    if (!ctx) return svx_fail(nullptr, SVX_ERR_ARG, "svx_prior_width: ctx is NULL");
    NEED(ctx, n_pairs >= 0, "svx_prior_width: negative n_pairs");
    NEED(ctx, n_pairs == 0 || (pairs && priors && width), "svx_prior_width: null argument");
    if (n_pairs == 0) return SVX_OK;
    for (int p = 0; p < n_pairs; p++) {
        const svx_prior& q = priors[p];
        NEED(ctx, pairs[p].n >= 0 && pairs[p].m >= 0, "svx_prior_width: pair %d: sizes n=%d m=%d", p, pairs[p].n, pairs[p].m);
        NEED(ctx, q.cap >= 0, "svx_prior_width: pair %d: prior cap %d", p, q.cap);
        NEED(ctx, q.info && (q.rows || q.cap == 0), "svx_prior_width: pair %d: null prior buffer", p);
    }
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    // ---- scratch: the descriptors only, uploaded
    const size_t b_up = ((size_t)n_pairs * sizeof(WidthPair) + 255) & ~(size_t)255;
    char *pin, *dev;
    int rc = svxl_scratch_begin(ctx, "svx_prior_width", b_up, b_up, &pin, &dev);
    if (rc) return rc;
    WidthPair* hp = reinterpret_cast<WidthPair*>(pin);
    for (int p = 0; p < n_pairs; p++) {
        WidthPair& r = hp[p];
        r.rows = priors[p].rows;
        r.info = priors[p].info;
        r.out = width + p;
        r.cap = priors[p].cap;
        r.n = pairs[p].n;
        r.m = pairs[p].m;
        r.pad = 0;
    }
    rc = svxl_scratch_upload(ctx, (size_t)n_pairs * sizeof(WidthPair));
    if (rc) return rc;
    hipLaunchKernelGGL(k_prior_width, dim3(n_pairs), dim3(256), 0, ctx->stream, reinterpret_cast<const WidthPair*>(dev));
    SVX_LAUNCH_CHECK(ctx, "k_prior_width");
    return SVX_OK;
}
