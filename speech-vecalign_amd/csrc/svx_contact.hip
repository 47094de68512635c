// svx_contact.hip -- band-edge contact of a returned path and band doubling (include/svx.h: svx_band_contact,
// svx_align_widen; gfx950 only).
//
//   k_band_contact  one workgroup per pair of the last batch.  Node i of a level is (0, 0) for i = 0 and the end of
//                   alignment row i - 1 otherwise; the nodes are strided over the 256 threads, 256 consecutive nodes
//                   per stretch.  A node's clearance is its distance in cells to the band edges that have a lattice node
//                   behind them.  Touch count and minimum clearance are plain block reductions; the longest run of
//                   consecutive touching nodes is a segmented combine of (length, prefix run, suffix run, best run):
//                   butterfly inside the wave with the lower lanes as the left operand, the four wave summaries through
//                   LDS, and a carry from stretch to stretch that every thread keeps (it is uniform).
//   k_stage_prior   one workgroup per pair: copies a pair's current result (rows up to the count it reads on the
//                   device, and the two info words) into the post-processing scratch, where the next round of
//                   svx_align_widen reads it as the prior -- a prior may not be the pair's own output buffer.
// Integers only, vector stores only; nothing here is on the hot path of a step.
#include <limits.h>

#include <vector>

#include "svx_common.h"

namespace {

struct ContactPair {
    const int* align;     // [n_align][4] rows of the level
    const int* n_align;
    const int* boff_out;  // [path_len + 2]
    const int* path_len;
    const int* status;    // the pair's info[1]
    int* out;             // [4]
    int size0, size1;
    int rows_cap;         // rows the align buffer holds
    int refined;          // 0: the pair has no band at this level (-1 row)
};

struct Run {  // summary of a stretch of nodes: its length, touching runs at its two ends, longest run inside
    int len, pre, suf, best;
};

__device__ __forceinline__ Run run_join(const Run& l, const Run& r) {
    Run o;
    o.len = l.len + r.len;
    o.pre = l.pre == l.len ? l.len + r.pre : l.pre;
    o.suf = r.suf == r.len ? r.len + l.suf : r.suf;
    const int mid = l.suf + r.pre;
    o.best = l.best > r.best ? l.best : r.best;
    o.best = mid > o.best ? mid : o.best;
    return o;
}

__global__ __launch_bounds__(256) void k_band_contact(const ContactPair* __restrict__ pairs, int B, int guard) {
    __shared__ int sh_run[4][4];
    __shared__ int sh_touch[4], sh_clear[4];
    const ContactPair P = pairs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int code = gld(P.status);
    int cnt = P.refined ? gld(P.n_align) : -1;
    if (code != 0 || cnt < 0 || cnt > P.rows_cap) {  // uniform: a failed pair, or a level without a band
        if (tid == 0) gst16(P.out, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
        return;
    }
    const int a_out = gld(P.path_len) + 2;
    const int nodes = cnt + 1;
    Run carry = {0, 0, 0, 0};
    int touch = 0, clear = INT_MAX;
    for (int base = 0; base < nodes; base += 256) {
        const int i = base + tid;
        Run me = {0, 0, 0, 0};
        if (i < nodes) {
            int x = 0, y = 0;
            if (i > 0) {
                const uint4 r = gld16(P.align + 4 * (size_t)(i - 1));
                x = (int)r.x + (int)r.y;
                y = (int)r.z + (int)r.w;
            }
            int c = INT_MAX;
            const long long a = (long long)x + y;
            if (x >= 0 && y >= 0 && a < a_out) {  // (a node outside the level's diagonals has no band to touch)
                const int o = gld(P.boff_out + a);
                const int b = y - o;
                const long long yl = (long long)o - 1, xl = a - yl;          // the cell below the band on this diagonal
                const long long yh = (long long)o + B, xh = a - yh;          // the cell above it
                if (xl >= 0 && xl <= P.size0 && yl >= 0 && yl <= P.size1) c = b;
                if (xh >= 0 && xh <= P.size0 && yh >= 0 && yh <= P.size1 && B - 1 - b < c) c = B - 1 - b;
            }
            const int t = c <= guard ? 1 : 0;
            me.len = 1; me.pre = me.suf = me.best = t;
            touch += t;
            clear = c < clear ? c : clear;
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {  // lane's aligned block of o nodes joins its neighbour block; the lower one is the left
            Run other;
            other.len = __shfl_xor(me.len, o, 64);
            other.pre = __shfl_xor(me.pre, o, 64);
            other.suf = __shfl_xor(me.suf, o, 64);
            other.best = __shfl_xor(me.best, o, 64);
            me = (lane & o) ? run_join(other, me) : run_join(me, other);
        }
        __syncthreads();  // (sh_run may still be read from the stretch before)
        if (lane == 0) { sh_run[w][0] = me.len; sh_run[w][1] = me.pre; sh_run[w][2] = me.suf; sh_run[w][3] = me.best; }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const Run r = {sh_run[u][0], sh_run[u][1], sh_run[u][2], sh_run[u][3]};
            carry = run_join(carry, r);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        touch += __shfl_xor(touch, o, 64);
        const int t = __shfl_xor(clear, o, 64);
        clear = t < clear ? t : clear;
    }
    __syncthreads();
    if (lane == 0) { sh_touch[w] = touch; sh_clear[w] = clear; }
    __syncthreads();
    if (tid == 0) {
        int ts = 0, cm = INT_MAX;
        for (int u = 0; u < 4; u++) { ts += sh_touch[u]; cm = sh_clear[u] < cm ? sh_clear[u] : cm; }
        gst16(P.out, (uint32_t)ts, (uint32_t)carry.best, (uint32_t)cm, (uint32_t)nodes);
    }
}

struct StagePair {
    const int* rows;   // the pair's align output, [cap][4]
    const int* info;   // [2]
    int* dst_rows;     // [cap][4] in the scratch
    int* dst_info;     // [2]
    int cap, pad;
};

__global__ __launch_bounds__(256) void k_stage_prior(const StagePair* __restrict__ pairs) {
    const StagePair P = pairs[blockIdx.x];
    const int count = gld(P.info), code = gld(P.info + 1);
    const int n = count < 0 ? 0 : (count > P.cap ? P.cap : count);   // (the ingest rejects a count outside [0, cap])
    for (int i = threadIdx.x; i < n; i += 256) {
        const uint4 r = gld16(P.rows + 4 * (size_t)i);
        gst16(P.dst_rows + 4 * (size_t)i, r.x, r.y, r.z, r.w);
    }
    if (threadIdx.x == 0) { gst(P.dst_info, count); gst(P.dst_info + 1, code); }
}

// svx_band_contact.  out == nullptr: the rows go to the scratch behind the descriptors and *out_scratch points at them
// (svx_align_widen reads them back from there).
int contact_impl(svx_ctx* ctx, const char* who, int level, int guard, int32_t* out, int32_t** out_scratch) {
    NEED(ctx, level >= 0, "%s: level %d", who, level);
    NEED(ctx, guard >= 0, "%s: guard %d", who, guard);
    SvxLastCall lc;
    int rc = svxl_last_call(ctx, who, -1, nullptr, &lc);
    if (rc) return rc;
    const int n_pairs = lc.n_pairs;
    const size_t b_up = up256((size_t)n_pairs * sizeof(ContactPair));
    const size_t b_all = b_up + (out ? 0 : up256((size_t)n_pairs * 4 * sizeof(int32_t)));
    char *pin, *dev;
    rc = svxl_scratch_begin(ctx, who, b_up, b_all, &pin, &dev);
    if (rc) return rc;
    int32_t* dst = out ? out : reinterpret_cast<int32_t*>(dev + b_up);
    ContactPair* hp = reinterpret_cast<ContactPair*>(pin);
    for (int p = 0; p < n_pairs; p++) {
        const SvxPairDev& P = lc.pair(p);
        ContactPair& r = hp[p];
        const bool refined = level <= P.L && (level < P.L || P.L == 0);
        const SvxLevel& Lv = P.lev[refined ? level : 0];
        r.align = Lv.align;
        r.n_align = Lv.n_align;
        r.boff_out = Lv.boff_out;
        r.path_len = Lv.path_len;
        r.status = P.status;
        r.out = dst + 4 * (size_t)p;
        r.size0 = Lv.n[0];
        r.size1 = Lv.n[1];
        r.rows_cap = Lv.n[0] + Lv.n[1] + 2;
        r.refined = refined ? 1 : 0;
    }
    rc = svxl_scratch_upload(ctx, (size_t)n_pairs * sizeof(ContactPair));
    if (rc) return rc;
    hipLaunchKernelGGL(k_band_contact, dim3(n_pairs), dim3(256), 0, ctx->stream, reinterpret_cast<const ContactPair*>(dev), lc.band, guard);
    SVX_LAUNCH_CHECK(ctx, "k_band_contact");
    if (out_scratch) *out_scratch = dst;
    return SVX_OK;
}

// contact of the last call at level 0, read back: rows [n][4] (synchronises the stream)
int contact_to_host(svx_ctx* ctx, int guard, int n, std::vector<int32_t>& rows) {
    int32_t* dev = nullptr;
    int rc = contact_impl(ctx, "svx_align_widen", 0, guard, nullptr, &dev);
    if (rc) return rc;
    rows.resize((size_t)n * 4);
    SVX_HIP(ctx, hipMemcpyAsync(rows.data(), dev, (size_t)n * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SVX_OK;
}

}  // namespace

extern "C" int svx_band_contact(svx_ctx* ctx, int level, int guard, int32_t* out) {
    if (!ctx) return svx_fail(nullptr, SVX_ERR_ARG, "svx_band_contact: ctx is NULL");
    NEED(ctx, out, "svx_band_contact: null argument");
    NEED(ctx, aligned16(out), "svx_band_contact: out must be 16-byte aligned");
    return contact_impl(ctx, "svx_band_contact", level, guard, out, nullptr);
}

extern "C" int svx_align_widen(svx_ctx* ctx, const svx_align_params* params, const svx_pair* pairs, const svx_prior* priors,
                               int n_pairs, const svx_widen_params* wp, int32_t* report) {
    if (!ctx) return svx_fail(nullptr, SVX_ERR_ARG, "svx_align_widen: ctx is NULL");
    NEED(ctx, n_pairs >= 0, "svx_align_widen: negative n_pairs");
    NEED(ctx, params && wp && (n_pairs == 0 || (pairs && report)), "svx_align_widen: null argument");
    NEED(ctx, wp->guard >= 0 && wp->max_width_over2 >= 0 && wp->max_rounds >= 0, "svx_align_widen: negative field (guard %d, max_width_over2 %d, max_rounds %d)",
         wp->guard, wp->max_width_over2, wp->max_rounds);
    const int W0 = params->width_over2 < 3 ? 3 : params->width_over2;
    NEED(ctx, wp->max_width_over2 >= W0, "svx_align_widen: max_width_over2 %d is below width_over2 %d", wp->max_width_over2, W0);
    if (n_pairs == 0) return SVX_OK;
    for (int p = 0; p < n_pairs; p++) {
        NEED(ctx, pairs[p].align && pairs[p].info, "svx_align_widen: pair %d: null pointer", p);
        NEED(ctx, pairs[p].n >= 1 && pairs[p].m >= 1, "svx_align_widen: pair %d: empty document", p);
    }
    // ---- round 0: the caller's search as it stands
    int rc = priors ? svx_align_around(ctx, params, pairs, priors, n_pairs) : svx_align_batch(ctx, params, pairs, n_pairs);
    if (rc) return rc;
    std::vector<int32_t> rows;
    if ((rc = contact_to_host(ctx, wp->guard, n_pairs, rows))) return rc;
    for (int p = 0; p < n_pairs; p++) {
        int32_t* r = report + 4 * (size_t)p;
        r[0] = 0; r[1] = W0; r[2] = r[3] = rows[4 * (size_t)p];
    }
    svx_align_params prm = *params;
    prm.search_mode = SVX_SEARCH_AROUND_WIDE;
    std::vector<int> idx;
    std::vector<svx_pair> sub;
    std::vector<svx_prior> pri;
    long long Wprev = W0;
    for (int round = 1; round <= wp->max_rounds; round++) {
        long long W = Wprev * 2;
        if (W > wp->max_width_over2) W = wp->max_width_over2;
        if (W == Wprev) break;   // at the cap
        idx.clear();
        for (int p = 0; p < n_pairs; p++)
            if (report[4 * (size_t)p + 3] > 0) idx.push_back(p);   // (a failed pair carries -1)
        if (idx.empty()) break;
        const int k = (int)idx.size();
        // ---- stage the current results as priors: [descriptors][rows and info of every pair]
        const size_t b_up = up256((size_t)k * sizeof(StagePair));
        size_t b_all = b_up;
        for (int j = 0; j < k; j++) b_all += up256(((size_t)pairs[idx[j]].n + pairs[idx[j]].m + 2) * 16) + 256;
        char *pin, *dev;
        if ((rc = svxl_scratch_begin(ctx, "svx_align_widen", b_up, b_all, &pin, &dev))) return rc;
        StagePair* hp = reinterpret_cast<StagePair*>(pin);
        sub.resize(k);
        pri.resize(k);
        char* at = dev + b_up;
        for (int j = 0; j < k; j++) {
            const svx_pair& q = pairs[idx[j]];
            const int cap = q.n + q.m + 2;
            StagePair& s = hp[j];
            s.rows = q.align;
            s.info = q.info;
            s.dst_rows = reinterpret_cast<int*>(at);
            at += up256((size_t)cap * 16);
            s.dst_info = reinterpret_cast<int*>(at);
            at += 256;
            s.cap = cap;
            s.pad = 0;
            sub[j] = q;
            pri[j].rows = s.dst_rows;
            pri[j].info = s.dst_info;
            pri[j].cap = cap;
            pri[j].pad = 0;
        }
        if ((rc = svxl_scratch_upload(ctx, (size_t)k * sizeof(StagePair)))) return rc;
        hipLaunchKernelGGL(k_stage_prior, dim3(k), dim3(256), 0, ctx->stream, reinterpret_cast<const StagePair*>(dev));
        SVX_LAUNCH_CHECK(ctx, "k_stage_prior");
        prm.width_over2 = (int32_t)W;
        if ((rc = svx_align_around(ctx, &prm, sub.data(), pri.data(), k))) return rc;
        if ((rc = contact_to_host(ctx, wp->guard, k, rows))) return rc;
        for (int j = 0; j < k; j++) {
            int32_t* r = report + 4 * (size_t)idx[j];
            r[0] = round; r[1] = (int32_t)W; r[3] = rows[4 * (size_t)j];
        }
        Wprev = W;
    }
    return SVX_OK;
}
