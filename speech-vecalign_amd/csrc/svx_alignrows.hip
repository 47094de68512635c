// svx_alignrows.hip -- svx_alignment_rows: the alignment rows of a batch -> the two row matrices the margin half
// expects (gfx950 only).
//
// The reference embeds the audio span of every mined alignment again (svecalign/postprocess/embed_align.py,
// svecalign/utils/file_utils.py:158-163).  For an alignment of at most k0 x k1 segments that span is a line of the
// candidate file, and its embedding is the candidate row vecs[len - 1][start + len - 1] the DP has just read: the rows
// are in HBM already.  Three launches on the context's stream, no host round trip:
//   k_rows_count   one workgroup per chunk of SVX_AR_CHUNK alignment rows of ONE pair: how many rows are kept
//   k_rows_scan    exclusive scan of the chunk counts (one workgroup, carry across its width) + the total
//   k_rows_gather  a chunk's flags again, ranked inside the workgroup, then one wave per kept alignment moves the
//                  source and the target row: every row is read once, 16 bytes per lane, and feeds the raw copy and
//                  the unit-norm fp16 / bf16 row (the arithmetic of k_unit_rows, svx_unit.h)
// Ragged batches: the grid runs over chunks, a host-built table maps chunk -> (pair, first row).
#include <string.h>

#include "svx_unit.h"

#define SVX_AR_CHUNK 256

namespace {

struct RowsPair {
    const void* v[2];      // [k][n][d] candidate tensors
    const int* align;      // [rows_cap][4]
    const double* scores;  // [rows_cap]
    const int* info;       // [2]
    int n, m, k0, k1;
    int rows_cap;          // n + m + 2: what align / scores hold
    int pad;
};

struct RowsChunk {
    int pair, first;
};

// The keep rule of include/svx.h.  A row that fails is never used to form an address: xr / yr are only set on success.
__device__ __forceinline__ bool rows_keep(const RowsPair& P, int r, double max_score, long long& xr, long long& yr) {
    const int n_align = gld(P.info), status = gld(P.info + 1);
    if (status != 0 || r >= n_align || r >= P.rows_cap) return false;
    const int xs = gld(P.align + 4 * (size_t)r), xl = gld(P.align + 4 * (size_t)r + 1);
    const int ys = gld(P.align + 4 * (size_t)r + 2), yl = gld(P.align + 4 * (size_t)r + 3);
    if (xl < 1 || xl > P.k0 || yl < 1 || yl > P.k1) return false;
    if (xs < 0 || ys < 0) return false;
    if ((long long)xs + xl > P.n || (long long)ys + yl > P.m) return false;
    const double s = gld(P.scores + r);
    if (!(s <= max_score)) return false;  // NaN fails
    xr = (long long)(xl - 1) * P.n + xs + xl - 1;
    yr = (long long)(yl - 1) * P.m + ys + yl - 1;
    return true;
}

__global__ __launch_bounds__(SVX_AR_CHUNK) void k_rows_count(const RowsPair* __restrict__ pairs, const RowsChunk* __restrict__ chunks,
                                                             double max_score, int* __restrict__ counts) {
    __shared__ int wtot[SVX_AR_CHUNK / SVX_WAVE];
    const RowsChunk c = chunks[blockIdx.x];
    const RowsPair P = pairs[c.pair];
    long long xr, yr;
    const bool keep = rows_keep(P, c.first + (int)threadIdx.x, max_score, xr, yr);
    const unsigned long long b = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < SVX_AR_CHUNK / SVX_WAVE; w++) s += wtot[w];
        counts[blockIdx.x] = s;
    }
}

// offs[i] = counts[0] + ... + counts[i - 1], *total = the sum of all: one workgroup walks the chunks 256 at a time and
// carries the running sum from one stretch to the next.
__global__ __launch_bounds__(256) void k_rows_scan(const int* __restrict__ counts, int n, long long* __restrict__ offs,
                                                   long long* __restrict__ total) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long carry = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + (int)threadIdx.x;
        const int v = i < n ? counts[i] : 0;
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
        if (i < n) offs[i] = carry + before + (inc - v);
        carry += all;
        __syncthreads();  // wsum is rewritten by the next stretch
    }
    if (threadIdx.x == 0) *total = carry;
}

// Flags and ranks of one chunk.  -> number kept in the chunk; slot[j] = thread (= row - first) of the j-th kept row,
// xrow / yrow [j] its candidate rows.  src[(base + j)] = (pair, row) is written here for base + j < cap.
struct RowsLds {
    long long xrow[SVX_AR_CHUNK], yrow[SVX_AR_CHUNK];
    int wtot[SVX_AR_CHUNK / SVX_WAVE];
};

__device__ __forceinline__ int rows_rank_chunk(const RowsPair& P, const RowsChunk& c, double max_score, long long base,
                                               long long cap, int* __restrict__ src, RowsLds& L) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = c.first + (int)threadIdx.x;
    long long xr = 0, yr = 0;
    const bool keep = rows_keep(P, r, max_score, xr, yr);
    const unsigned long long b = __ballot(keep);
    if (lane == 0) L.wtot[w] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int u = 0; u < SVX_AR_CHUNK / SVX_WAVE; u++) {
        before += u < w ? L.wtot[u] : 0;
        all += L.wtot[u];
    }
    if (keep) {
        const int j = before + __popcll(b & ((1ull << lane) - 1ull));
        L.xrow[j] = xr;
        L.yrow[j] = yr;
        if (base + j < cap) {
            gst(src + 2 * (base + j), c.pair);
            gst(src + 2 * (base + j) + 1, r);
        }
    }
    __syncthreads();
    return all;
}

// Raw copies and unit rows.  QE: input element type; NT: 512-element stretches of a row (d <= 512 NT: 1, else 2).
// A lane holds the 8 elements [512 t + 8 lane, + 8) of both rows as they came out of memory (svx_unit.h's lane map);
// lanes past the row hold zeros, which add nothing to the sum of squares.
template <typename QE, int NT>
__global__ __launch_bounds__(SVX_AR_CHUNK) void k_rows_gather_unit(const RowsPair* __restrict__ pairs, const RowsChunk* __restrict__ chunks,
                                                                   const long long* __restrict__ offs, double max_score, long long cap,
                                                                   int d, int bf, char* __restrict__ x_rows, char* __restrict__ y_rows,
                                                                   uint16_t* __restrict__ x_unit, uint16_t* __restrict__ y_unit,
                                                                   int* __restrict__ src) {
    __shared__ RowsLds L;
    using S = typename QE::storage;
    constexpr int NP = 8 / QE::VEC;  // 16-byte pieces per 8 elements
    const long long base = offs[blockIdx.x];
    if (base >= cap) return;  // (uniform) nothing of this chunk is written
    const RowsChunk c = chunks[blockIdx.x];
    const RowsPair P = pairs[c.pair];
    const int kept = rows_rank_chunk(P, c, max_score, base, cap, src, L);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t row_bytes = (size_t)d * sizeof(S);
    for (int j = w; j < kept; j += SVX_AR_CHUNK / SVX_WAVE) {
        const long long o = base + j;
        if (o >= cap) break;
        const S* xs = reinterpret_cast<const S*>(P.v[0]) + (size_t)L.xrow[j] * d;
        const S* ys = reinterpret_cast<const S*>(P.v[1]) + (size_t)L.yrow[j] * d;
        uint4 px[NT][NP], py[NT][NP];
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const int col = 512 * t + 8 * lane;
#pragma unroll
            for (int q = 0; q < NP; q++) {
                px[t][q] = col < d ? gld16(xs + col + q * QE::VEC) : make_uint4(0, 0, 0, 0);
                py[t][q] = col < d ? gld16(ys + col + q * QE::VEC) : make_uint4(0, 0, 0, 0);
            }
        }
        float ssx = 0.f, ssy = 0.f;
#pragma unroll
        for (int t = 0; t < NT; t++) {
            float a[8], b[8];
#pragma unroll
            for (int q = 0; q < NP; q++) {
                decode_piece<QE>(px[t][q], a + q * QE::VEC);
                decode_piece<QE>(py[t][q], b + q * QE::VEC);
            }
            ssx = unit_sumsq8(ssx, a);
            ssy = unit_sumsq8(ssy, b);
        }
        const float ix = unit_scale(wave_sum(ssx)), iy = unit_scale(wave_sum(ssy));
        char* xo = x_rows + (size_t)o * row_bytes;
        char* yo = y_rows + (size_t)o * row_bytes;
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const int col = 512 * t + 8 * lane;
            if (col < d) {
                float a[8], b[8];
#pragma unroll
                for (int q = 0; q < NP; q++) {
                    gst16(xo + (size_t)(col + q * QE::VEC) * sizeof(S), px[t][q].x, px[t][q].y, px[t][q].z, px[t][q].w);
                    gst16(yo + (size_t)(col + q * QE::VEC) * sizeof(S), py[t][q].x, py[t][q].y, py[t][q].z, py[t][q].w);
                    decode_piece<QE>(px[t][q], a + q * QE::VEC);
                    decode_piece<QE>(py[t][q], b + q * QE::VEC);
                }
                const uint4 ux = unit_pack8(a, ix, bf != 0), uy = unit_pack8(b, iy, bf != 0);
                gst16(x_unit + (size_t)o * d + col, ux.x, ux.y, ux.z, ux.w);
                gst16(y_unit + (size_t)o * d + col, uy.x, uy.y, uy.z, uy.w);
            }
        }
    }
}

// Raw copies only (any alignment dimension: a row is `pieces` 16-byte pieces, up to 512 of them).
__global__ __launch_bounds__(SVX_AR_CHUNK) void k_rows_gather_raw(const RowsPair* __restrict__ pairs, const RowsChunk* __restrict__ chunks,
                                                                  const long long* __restrict__ offs, double max_score, long long cap,
                                                                  int pieces, uint4* __restrict__ x_rows, uint4* __restrict__ y_rows,
                                                                  int* __restrict__ src) {
    __shared__ RowsLds L;
    const long long base = offs[blockIdx.x];
    if (base >= cap) return;
    const RowsChunk c = chunks[blockIdx.x];
    const RowsPair P = pairs[c.pair];
    const int kept = rows_rank_chunk(P, c, max_score, base, cap, src, L);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int j = w; j < kept; j += SVX_AR_CHUNK / SVX_WAVE) {
        const long long o = base + j;
        if (o >= cap) break;
        const uint4* xs = reinterpret_cast<const uint4*>(P.v[0]) + (size_t)L.xrow[j] * pieces;
        const uint4* ys = reinterpret_cast<const uint4*>(P.v[1]) + (size_t)L.yrow[j] * pieces;
        uint4* xo = x_rows + (size_t)o * pieces;
        uint4* yo = y_rows + (size_t)o * pieces;
        for (int p0 = 0; p0 < pieces; p0 += 4 * SVX_WAVE) {  // eight loads in flight per lane
            uint4 vx[4], vy[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int p = p0 + u * SVX_WAVE + lane;
                if (p < pieces) {
                    vx[u] = gld16(xs + p);
                    vy[u] = gld16(ys + p);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int p = p0 + u * SVX_WAVE + lane;
                if (p < pieces) {
                    gst16(xo + p, vx[u].x, vx[u].y, vx[u].z, vx[u].w);
                    gst16(yo + p, vy[u].x, vy[u].y, vy[u].z, vy[u].w);
                }
            }
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

#define NEED(ctx, cond, ...) \
    do { if (!(cond)) return svx_fail(ctx, SVX_ERR_ARG, __VA_ARGS__); } while (0)

void svxl_alignrows_release(svx_ctx* ctx) {
    if (ctx->rows_buf) (void)hipFree(ctx->rows_buf);
    ctx->rows_buf = nullptr;
    ctx->rows_bytes = 0;
    for (int i = 0; i < 2; i++) {
        if (ctx->rows_pin[i]) (void)hipHostFree(ctx->rows_pin[i]);
        if (ctx->rows_up[i]) (void)hipEventDestroy(ctx->rows_up[i]);
        ctx->rows_pin[i] = nullptr;
        ctx->rows_pin_cap[i] = 0;
        ctx->rows_up[i] = nullptr;
        ctx->rows_up_valid[i] = 0;
    }
}

extern "C" int svx_alignment_rows(svx_ctx* ctx, int dtype, int d, const svx_pair* pairs, int n_pairs, double max_score, int64_t cap,
                                  void* x_rows, void* y_rows, void* x_unit, void* y_unit, int unit_dtype, int32_t* src,
                                  int64_t* count) {
    if (!ctx) return svx_fail(nullptr, SVX_ERR_ARG, "svx_alignment_rows: ctx is NULL");
    NEED(ctx, count, "svx_alignment_rows: count is NULL");
    NEED(ctx, n_pairs >= 0 && cap >= 0, "svx_alignment_rows: negative n_pairs or cap");
    NEED(ctx, n_pairs == 0 || pairs, "svx_alignment_rows: pairs is NULL");
    NEED(ctx, dtype == SVX_F32 || dtype == SVX_F16 || dtype == SVX_BF16, "svx_alignment_rows: unknown dtype %d", dtype);
    NEED(ctx, (x_unit == nullptr) == (y_unit == nullptr), "svx_alignment_rows: x_unit and y_unit are given together or not at all");
    const bool unit = x_unit != nullptr;
    if (unit) {
        NEED(ctx, unit_dtype == SVX_F16 || unit_dtype == SVX_BF16, "svx_alignment_rows: unit rows are kept in fp16 or bf16 (got dtype %d)", unit_dtype);
        NEED(ctx, d > 0 && d % 32 == 0 && d <= 32 * KNN_KSTEPS,
             "svx_alignment_rows: embedding dimension %d: with unit rows it must be a positive multiple of 32, at most %d", d, 32 * KNN_KSTEPS);
    } else {
        NEED(ctx, d > 0 && d % 8 == 0 && d <= SVX_MAX_DIM,
             "svx_alignment_rows: embedding dimension %d: must be a positive multiple of 8, at most %d", d, SVX_MAX_DIM);
    }
    const bool writes = cap > 0 && n_pairs > 0;
    if (writes) {
        NEED(ctx, x_rows && y_rows && src, "svx_alignment_rows: null output buffer");
        NEED(ctx, aligned16(x_rows) && aligned16(y_rows) && aligned16(x_unit) && aligned16(y_unit),
             "svx_alignment_rows: the row buffers must be 16-byte aligned");
    }
    long long n_chunks = 0;
    for (int p = 0; p < n_pairs; p++) {
        const svx_pair& q = pairs[p];
        NEED(ctx, q.n >= 0 && q.m >= 0 && q.k0 >= 1 && q.k1 >= 1, "svx_alignment_rows: pair %d: sizes n=%d m=%d k0=%d k1=%d", p, q.n, q.m, q.k0, q.k1);
        NEED(ctx, q.align && q.scores && q.info, "svx_alignment_rows: pair %d: null align / scores / info", p);
        NEED(ctx, (q.vecs0 || q.n == 0) && (q.vecs1 || q.m == 0), "svx_alignment_rows: pair %d: null vecs", p);
        NEED(ctx, aligned16(q.vecs0) && aligned16(q.vecs1), "svx_alignment_rows: pair %d: vecs must be 16-byte aligned", p);
        NEED(ctx, (long long)q.n + q.m + 2 <= 0x7fffffffLL, "svx_alignment_rows: pair %d: too many alignment rows", p);
        n_chunks += ((long long)q.n + q.m + 2 + SVX_AR_CHUNK - 1) / SVX_AR_CHUNK;
    }
    NEED(ctx, n_chunks <= 0x7fffffffLL, "svx_alignment_rows: %lld chunks of alignment rows", n_chunks);
    int rc = svx_flush(ctx);  // with the software pipeline on, the alignment outputs are complete only behind this
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    if (n_pairs == 0) {
        SVX_HIP(ctx, hipMemsetAsync(count, 0, sizeof(int64_t), st));
        return SVX_OK;
    }
    // ---- scratch: [descriptors][chunk table][chunk counts][chunk offsets]; the first two are uploaded
    auto up256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_desc = up256((size_t)n_pairs * sizeof(RowsPair)), b_tab = up256((size_t)n_chunks * sizeof(RowsChunk));
    const size_t b_cnt = up256((size_t)n_chunks * sizeof(int)), b_off = up256((size_t)n_chunks * sizeof(long long));
    const size_t b_up = b_desc + b_tab, b_all = b_up + b_cnt + b_off;
    if (b_all > ctx->rows_bytes) {
        SVX_HIP(ctx, hipStreamSynchronize(st));  // (an earlier call may still read the old buffer)
        if (ctx->rows_buf) SVX_HIP(ctx, hipFree(ctx->rows_buf));
        ctx->rows_buf = nullptr;
        ctx->rows_bytes = 0;
        const size_t want = b_all + b_all / 4;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&ctx->rows_buf), want);
        if (e != hipSuccess) return svx_fail(ctx, SVX_ERR_NOMEM, "svx_alignment_rows: hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        ctx->rows_bytes = want;
    }
    // pinned staging, two buffers in turn: the host may run a call ahead of the device without waiting for the upload of
    // the call before
    const int turn = ctx->rows_turn;
    ctx->rows_turn = 1 - turn;
    if (!ctx->rows_up[turn]) SVX_HIP(ctx, hipEventCreateWithFlags(&ctx->rows_up[turn], hipEventDisableTiming));
    if (ctx->rows_up_valid[turn]) SVX_HIP(ctx, hipEventSynchronize(ctx->rows_up[turn]));
    if (b_up > ctx->rows_pin_cap[turn]) {
        if (ctx->rows_pin[turn]) SVX_HIP(ctx, hipHostFree(ctx->rows_pin[turn]));
        ctx->rows_pin[turn] = nullptr;
        ctx->rows_pin_cap[turn] = 0;
        SVX_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->rows_pin[turn]), b_up + b_up / 4, hipHostMallocDefault));
        ctx->rows_pin_cap[turn] = b_up + b_up / 4;
    }
    RowsPair* hp = reinterpret_cast<RowsPair*>(ctx->rows_pin[turn]);
    RowsChunk* hc = reinterpret_cast<RowsChunk*>(ctx->rows_pin[turn] + b_desc);
    long long at = 0;
    for (int p = 0; p < n_pairs; p++) {
        const svx_pair& q = pairs[p];
        RowsPair& r = hp[p];
        r.v[0] = q.vecs0; r.v[1] = q.vecs1;
        r.align = q.align; r.scores = q.scores; r.info = q.info;
        r.n = q.n; r.m = q.m; r.k0 = q.k0; r.k1 = q.k1;
        r.rows_cap = q.n + q.m + 2;
        r.pad = 0;
        for (int first = 0; first < r.rows_cap; first += SVX_AR_CHUNK) {
            hc[at].pair = p;
            hc[at].first = first;
            at++;
        }
    }
    SVX_HIP(ctx, hipMemcpyAsync(ctx->rows_buf, ctx->rows_pin[turn], b_up, hipMemcpyHostToDevice, st));
    SVX_HIP(ctx, hipEventRecord(ctx->rows_up[turn], st));
    ctx->rows_up_valid[turn] = 1;
    const RowsPair* dp = reinterpret_cast<const RowsPair*>(ctx->rows_buf);
    const RowsChunk* dc = reinterpret_cast<const RowsChunk*>(ctx->rows_buf + b_desc);
    int* dcnt = reinterpret_cast<int*>(ctx->rows_buf + b_up);
    long long* doff = reinterpret_cast<long long*>(ctx->rows_buf + b_up + b_cnt);
    const dim3 grid((unsigned)n_chunks), block(SVX_AR_CHUNK);
    k_rows_count<<<grid, block, 0, st>>>(dp, dc, max_score, dcnt);
    SVX_LAUNCH_CHECK(ctx, "k_rows_count");
    k_rows_scan<<<dim3(1), dim3(256), 0, st>>>(dcnt, (int)n_chunks, doff, reinterpret_cast<long long*>(count));
    SVX_LAUNCH_CHECK(ctx, "k_rows_scan");
    if (!writes) return SVX_OK;
    if (unit) {
        const int bf = unit_dtype == SVX_BF16;
        char* xr = reinterpret_cast<char*>(x_rows);
        char* yr = reinterpret_cast<char*>(y_rows);
        uint16_t* xu = reinterpret_cast<uint16_t*>(x_unit);
        uint16_t* yu = reinterpret_cast<uint16_t*>(y_unit);
#define G(QE, NT) k_rows_gather_unit<QE, NT><<<grid, block, 0, st>>>(dp, dc, doff, max_score, (long long)cap, d, bf, xr, yr, xu, yu, src)
#define GD(QE) do { if (d <= 512) G(QE, 1); else G(QE, 2); } while (0)
        if (dtype == SVX_F32) GD(ElemF32);
        else if (dtype == SVX_F16) GD(ElemF16);
        else GD(ElemBF16);
#undef GD
#undef G
    } else {
        const int pieces = d * (dtype == SVX_F32 ? 4 : 2) / 16;
        k_rows_gather_raw<<<grid, block, 0, st>>>(dp, dc, doff, max_score, (long long)cap, pieces, reinterpret_cast<uint4*>(x_rows),
                                                  reinterpret_cast<uint4*>(y_rows), src);
    }
    SVX_LAUNCH_CHECK(ctx, "k_rows_gather");
    return SVX_OK;
}
