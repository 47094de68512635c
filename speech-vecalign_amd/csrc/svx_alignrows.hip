// svx_alignrows.hip -- svx_alignment_rows and svx_concat_rows: the alignment rows of a batch -> the two row matrices the
// margin half expects (gfx950 only).
//
// The reference embeds the audio span of every mined alignment again (svecalign/postprocess/embed_align.py,
// svecalign/utils/file_utils.py:158-163).  For an alignment of at most k0 x k1 segments that span is a line of the
// candidate file, and its embedding is the candidate row vecs[len - 1][start + len - 1] the DP has just read: the rows
// are in HBM already.  Both calls run on the context's stream with no host round trip; ragged batches: the grids run over
// chunks of SVX_AR_CHUNK alignment rows of ONE pair, a host-built table maps chunk -> (pair, first row).
//
// svx_alignment_rows, three launches:
//   k_rows_count        one workgroup per chunk: how many rows are kept
//   k_scan              exclusive scan of the chunk counts (one workgroup, carry across its width) + the total
//   k_rows_gather_*     a chunk's flags again, ranked inside the workgroup, then one wave per kept alignment moves the
//                       source and the target row
//
// svx_concat_rows, the reference's post-filter chain filter_by_cost -> concat_aligns -> filter_by_dur.  concat_aligns only
// joins alignments that are directly connected on both sides, so a joined alignment is a contiguous run of segments on each
// side; while that run is at most k0 x k1 segments its embedding is again a candidate row.  Two compactions and a gather:
//   k_cat_base_count    one workgroup per chunk: how many are base rows
//   k_scan              exclusive scan of the chunk counts, the total behind the last
//   k_cat_base_write    the base rows of the batch, compacted in (pair, row) order: span, row number, pair
//   k_cat_out_count     one thread per base row walks its run (at most SVX_CONCAT_MAX rows ahead in the compacted list, which
//                       is why a successor in the next chunk, or 300 deletions later, costs nothing); fitting and wide
//                       outputs per workgroup
//   k_scan              again, + the two totals
//   k_cat_out_write     the walk again, ranked inside the workgroup: meta and the two candidate row numbers per output
//   k_cat_gather_*      one wave per output row, over an even split of the outputs
//
// What the two calls share is written once: the base-row rule (cat_base), the rank of a flag in its workgroup
// (block_rank), the scan (wave_scan, k_scan) and the row movers (move_unit, move_raw) -- every row is read once, 16 bytes
// per lane, and feeds the raw copy and the unit-norm fp16 / bf16 row (the arithmetic of k_unit_rows, svx_unit.h).  Where
// they differ they keep code of their own: the keep rule's width limit, and the split of the gather (ranked per chunk in
// k_rows_gather_*, even in k_cat_gather_*).  The scratch of both is the context's post-processing scratch (svx_common.h).
#include <string.h>

#include "svx_unit.h"

#define SVX_AR_CHUNK 256
#define SVX_CAT_ROWS_PER_BLOCK 16   // outputs per workgroup of svx_concat_rows' gather: four per wave

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

struct CatPair : RowsPair {
    const int* fr[2];      // [n][2], [m][2] (start, end) sample positions, or null
};

struct RowsChunk {
    int pair, first;
};

struct CatParams {
    double max_score, max_sil, max_dur, rate;
    long long min_frames;
    int max_num, both;
};

struct CatItem {
    long long xrow, yrow;
};

// The base-row rule of include/svx.h.  A row that fails is never used to form an address: `a` is only set on success.
__device__ __forceinline__ bool cat_base(const RowsPair& P, int r, double max_score, int4& a) {
    const int n_align = gld(P.info), status = gld(P.info + 1);
    if (status != 0 || r >= n_align || r >= P.rows_cap) return false;
    const int xs = gld(P.align + 4 * (size_t)r), xl = gld(P.align + 4 * (size_t)r + 1);
    const int ys = gld(P.align + 4 * (size_t)r + 2), yl = gld(P.align + 4 * (size_t)r + 3);
    if (xl < 1 || yl < 1 || xs < 0 || ys < 0) return false;
    if ((long long)xs + xl > P.n || (long long)ys + yl > P.m) return false;
    const double s = gld(P.scores + r);
    if (!(s <= max_score)) return false;  // NaN fails
    a = make_int4(xs, xl, ys, yl);
    return true;
}

// The keep rule of include/svx.h: a base row no wider than a candidate.  xr / yr, its candidate rows, are only set on success.
__device__ __forceinline__ bool rows_keep(const RowsPair& P, int r, double max_score, long long& xr, long long& yr) {
    int4 a;
    if (!cat_base(P, r, max_score, a)) return false;
    if (a.y > P.k0 || a.w > P.k1) return false;
    xr = (long long)(a.y - 1) * P.n + a.x + a.y - 1;
    yr = (long long)(a.w - 1) * P.m + a.z + a.w - 1;
    return true;
}

// number of set flags in the workgroup (SVX_AR_CHUNK threads) and, for a thread whose flag is set, its rank among them
__device__ __forceinline__ int block_rank(bool flag, int* wtot, int& rank) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) wtot[w] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int u = 0; u < SVX_AR_CHUNK / SVX_WAVE; u++) {
        before += u < w ? wtot[u] : 0;
        all += wtot[u];
    }
    rank = before + __popcll(b & ((1ull << lane) - 1ull));
    return all;
}

// inclusive scan inside the wave
__device__ __forceinline__ int wave_scan(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// offs[i] = counts[0] + ... + counts[i - 1] for i = 0 .. n (offs[n] is the total): one workgroup walks the counts 256 at a
// time and carries the running sum.  The total also goes to out[0] when `out` is given, the sum of `wide` to out[1] when
// `wide` is.
__global__ __launch_bounds__(256) void k_scan(const int* __restrict__ counts, int n, long long* __restrict__ offs,
                                              const int* __restrict__ wide, long long* __restrict__ out) {
    __shared__ int wsum[4];
    __shared__ long long wwide[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long carry = 0, mine = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + (int)threadIdx.x;
        const int v = i < n ? counts[i] : 0;
        if (wide && i < n) mine += wide[i];
        const int inc = wave_scan(v, lane);
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
    if (threadIdx.x == 0) {
        offs[n] = carry;
        if (out) out[0] = carry;
    }
    if (wide) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
        if (lane == 0) wwide[w] = mine;
        __syncthreads();
        if (threadIdx.x == 0) out[1] = wwide[0] + wwide[1] + wwide[2] + wwide[3];
    }
}

// ---- the row movers: one wave moves the source row xs and the target row ys to output row o
// Raw copies and unit rows.  QE: input element type; NT: 512-element stretches of a row (d <= 512 NT: 1, else 2).
// A lane holds the 8 elements [512 t + 8 lane, + 8) of both rows as they came out of memory (svx_unit.h's lane map);
// lanes past the row hold zeros, which add nothing to the sum of squares.
template <typename QE, int NT>
__device__ __forceinline__ void move_unit(const typename QE::storage* xs, const typename QE::storage* ys, long long o, int d, int bf,
                                          char* x_rows, char* y_rows, uint16_t* x_unit, uint16_t* y_unit, int lane) {
    using S = typename QE::storage;
    constexpr int NP = 8 / QE::VEC;  // 16-byte pieces per 8 elements
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
    // one element offset for the four stores: with a byte offset for the raw rows and an element offset for the unit rows
    // the compiler carries a pointer per output through the callers' loops, 8 VGPRs that cost
    // k_rows_gather_unit<ElemBF16, 2> a wave of occupancy (profiles/post_scratch_kernels.md)
    const size_t uo = (size_t)o * d;
    char* xo = x_rows + uo * sizeof(S);
    char* yo = y_rows + uo * sizeof(S);
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
            gst16(x_unit + uo + col, ux.x, ux.y, ux.z, ux.w);
            gst16(y_unit + uo + col, uy.x, uy.y, uy.z, uy.w);
        }
    }
}

// Raw copies only (any alignment dimension: a row is `pieces` 16-byte pieces, up to 512 of them).
__device__ __forceinline__ void move_raw(const uint4* xs, const uint4* ys, long long o, int pieces, uint4* x_rows, uint4* y_rows,
                                         int lane) {
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

// ------------------------------------------------------------------------------ svx_alignment_rows
__global__ __launch_bounds__(SVX_AR_CHUNK) void k_rows_count(const RowsPair* __restrict__ pairs, const RowsChunk* __restrict__ chunks,
                                                             double max_score, int* __restrict__ counts) {
    __shared__ int wtot[SVX_AR_CHUNK / SVX_WAVE];
    const RowsChunk c = chunks[blockIdx.x];
    const RowsPair P = pairs[c.pair];
    long long xr, yr;
    int rank;
    const int all = block_rank(rows_keep(P, c.first + (int)threadIdx.x, max_score, xr, yr), wtot, rank);
    if (threadIdx.x == 0) counts[blockIdx.x] = all;
}

// Flags and ranks of one chunk.  -> number kept in the chunk; xrow / yrow [j] the candidate rows of the j-th kept row.
// src[(base + j)] = (pair, row) is written here for base + j < cap.
struct RowsLds {
    long long xrow[SVX_AR_CHUNK], yrow[SVX_AR_CHUNK];
    int wtot[SVX_AR_CHUNK / SVX_WAVE];
};

__device__ __forceinline__ int rows_rank_chunk(const RowsPair& P, const RowsChunk& c, double max_score, long long base,
                                               long long cap, int* __restrict__ src, RowsLds& L) {
    const int r = c.first + (int)threadIdx.x;
    long long xr = 0, yr = 0;
    const bool keep = rows_keep(P, r, max_score, xr, yr);
    int j;
    const int all = block_rank(keep, L.wtot, j);
    if (keep) {
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

template <typename QE, int NT>
__global__ __launch_bounds__(SVX_AR_CHUNK) void k_rows_gather_unit(const RowsPair* __restrict__ pairs, const RowsChunk* __restrict__ chunks,
                                                                   const long long* __restrict__ offs, double max_score, long long cap,
                                                                   int d, int bf, char* __restrict__ x_rows, char* __restrict__ y_rows,
                                                                   uint16_t* __restrict__ x_unit, uint16_t* __restrict__ y_unit,
                                                                   int* __restrict__ src) {
    __shared__ RowsLds L;
    using S = typename QE::storage;
    const long long base = offs[blockIdx.x];
    if (base >= cap) return;  // (uniform) nothing of this chunk is written
    const RowsChunk c = chunks[blockIdx.x];
    const RowsPair P = pairs[c.pair];
    const int kept = rows_rank_chunk(P, c, max_score, base, cap, src, L);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int j = w; j < kept; j += SVX_AR_CHUNK / SVX_WAVE) {
        const long long o = base + j;
        if (o >= cap) break;
        move_unit<QE, NT>(reinterpret_cast<const S*>(P.v[0]) + (size_t)L.xrow[j] * d, reinterpret_cast<const S*>(P.v[1]) + (size_t)L.yrow[j] * d,
                          o, d, bf, x_rows, y_rows, x_unit, y_unit, lane);
    }
}

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
        move_raw(reinterpret_cast<const uint4*>(P.v[0]) + (size_t)L.xrow[j] * pieces, reinterpret_cast<const uint4*>(P.v[1]) + (size_t)L.yrow[j] * pieces,
                 o, pieces, x_rows, y_rows, lane);
    }
}

// ------------------------------------------------------------------------------ svx_concat_rows
__global__ __launch_bounds__(SVX_AR_CHUNK) void k_cat_base_count(const CatPair* __restrict__ pairs, const RowsChunk* __restrict__ chunks,
                                                                double max_score, int* __restrict__ counts) {
    __shared__ int wtot[SVX_AR_CHUNK / SVX_WAVE];
    const RowsChunk c = chunks[blockIdx.x];
    const CatPair P = pairs[c.pair];
    int4 a;
    int rank;
    const int all = block_rank(cat_base(P, c.first + (int)threadIdx.x, max_score, a), wtot, rank);
    if (threadIdx.x == 0) counts[blockIdx.x] = all;
}

__global__ __launch_bounds__(SVX_AR_CHUNK) void k_cat_base_write(const CatPair* __restrict__ pairs, const RowsChunk* __restrict__ chunks,
                                                                const long long* __restrict__ offs, double max_score,
                                                                int4* __restrict__ bspan, int* __restrict__ brow, int* __restrict__ bpair) {
    __shared__ int wtot[SVX_AR_CHUNK / SVX_WAVE];
    const RowsChunk c = chunks[blockIdx.x];
    const CatPair P = pairs[c.pair];
    const int r = c.first + (int)threadIdx.x;
    int4 a = make_int4(0, 0, 0, 0);
    int rank;
    const bool base = cat_base(P, r, max_score, a);
    block_rank(base, wtot, rank);
    if (base) {
        const long long g = offs[blockIdx.x] + rank;
        bspan[g] = a;
        brow[g] = r;
        bpair[g] = c.pair;
    }
}

// The run that starts at base row g (include/svx.h: joining, span, duration filter, fit).  -> bit e set: the output (g, e)
// fits a candidate row; wide: the outputs that pass the duration filter but do not fit.  end: one past the pair's base rows.
__device__ __forceinline__ unsigned cat_walk(const CatPair& P, const CatParams& C, const int4* __restrict__ bspan, long long g,
                                             long long end, int& wide) {
    const int4 f = bspan[g];
    const int* F0 = P.fr[0];
    const int* F1 = P.fr[1];
    unsigned fit = 0;
    wide = 0;
    int4 l = f;
    for (int e = 0; e < C.max_num; e++) {
        if (e > 0) {
            if (g + e >= end) break;
            const int4 nx = bspan[g + e];
            if ((double)((long long)gld(F0 + 2 * (size_t)(nx.x + nx.y - 1) + 1) - (long long)gld(F0 + 2 * (size_t)f.x)) / C.rate > C.max_dur) break;
            if (C.both && (double)((long long)gld(F1 + 2 * (size_t)(nx.z + nx.w - 1) + 1) - (long long)gld(F1 + 2 * (size_t)f.z)) / C.rate > C.max_dur) break;
            if (nx.x != l.x + l.y || nx.z != l.z + l.w) break;
            if ((double)((long long)gld(F0 + 2 * (size_t)nx.x) - (long long)gld(F0 + 2 * (size_t)(l.x + l.y - 1) + 1)) / C.rate > C.max_sil) break;
            if ((double)((long long)gld(F1 + 2 * (size_t)nx.z) - (long long)gld(F1 + 2 * (size_t)(l.z + l.w - 1) + 1)) / C.rate > C.max_sil) break;
            l = nx;
        }
        const int xl = l.x + l.y - f.x, yl = l.z + l.w - f.z;
        if (C.min_frames > 0) {
            const long long dx = (long long)gld(F0 + 2 * (size_t)(f.x + xl - 1) + 1) - (long long)gld(F0 + 2 * (size_t)f.x);
            const long long dy = (long long)gld(F1 + 2 * (size_t)(f.z + yl - 1) + 1) - (long long)gld(F1 + 2 * (size_t)f.z);
            if (!(C.min_frames <= dx && C.min_frames <= dy)) continue;
        }
        if (xl <= P.k0 && yl <= P.k1) fit |= 1u << e;
        else wide++;
    }
    return fit;
}

// pfirst[p]: the first chunk of pair p (pfirst[n_pairs] = the number of chunks), so offs[pfirst[p + 1]] ends p's base rows
__global__ __launch_bounds__(SVX_AR_CHUNK) void k_cat_out_count(const CatPair* __restrict__ pairs, const int* __restrict__ pfirst,
                                                               const long long* __restrict__ offs, int n_chunks, CatParams C,
                                                               const int4* __restrict__ bspan, const int* __restrict__ bpair,
                                                               int* __restrict__ nfit, int* __restrict__ nwide) {
    __shared__ int sf[SVX_AR_CHUNK / SVX_WAVE], sw[SVX_AR_CHUNK / SVX_WAVE];
    const long long g = (long long)blockIdx.x * SVX_AR_CHUNK + threadIdx.x;
    int fit = 0, wide = 0;
    if (g < offs[n_chunks]) {
        const int p = bpair[g];
        const CatPair P = pairs[p];
        fit = __popc(cat_walk(P, C, bspan, g, offs[pfirst[p + 1]], wide));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        fit += __shfl_down(fit, o, 64);
        wide += __shfl_down(wide, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sf[threadIdx.x >> 6] = fit;
        sw[threadIdx.x >> 6] = wide;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        nfit[blockIdx.x] = sf[0] + sf[1] + sf[2] + sf[3];
        nwide[blockIdx.x] = sw[0] + sw[1] + sw[2] + sw[3];
    }
}

__global__ __launch_bounds__(SVX_AR_CHUNK) void k_cat_out_write(const CatPair* __restrict__ pairs, const int* __restrict__ pfirst,
                                                               const long long* __restrict__ offs, int n_chunks, CatParams C,
                                                               const int4* __restrict__ bspan, const int* __restrict__ brow,
                                                               const int* __restrict__ bpair, const long long* __restrict__ offs2,
                                                               long long cap, int* __restrict__ meta, CatItem* __restrict__ items) {
    __shared__ int wsum[SVX_AR_CHUNK / SVX_WAVE];
    const long long base = offs2[blockIdx.x];
    if (base >= cap) return;  // (uniform) nothing of this workgroup is written
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long g = (long long)blockIdx.x * SVX_AR_CHUNK + threadIdx.x;
    unsigned fit = 0;
    int p = 0, wide;
    CatPair P = {};
    if (g < offs[n_chunks]) {
        p = bpair[g];
        P = pairs[p];
        fit = cat_walk(P, C, bspan, g, offs[pfirst[p + 1]], wide);
    }
    const int v = __popc(fit);
    const int inc = wave_scan(v, lane);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int u = 0; u < SVX_AR_CHUNK / SVX_WAVE; u++) before += u < w ? wsum[u] : 0;
    long long j = base + before + (inc - v);
    if (!fit) return;
    const int4 f = bspan[g];
    const int r0 = brow[g];
    for (int e = 0; e < C.max_num; e++) {
        if (!(fit >> e & 1u)) continue;
        if (j >= cap) break;
        const int4 l = bspan[g + e];
        const int xl = l.x + l.y - f.x, yl = l.z + l.w - f.z;
        int* m = meta + 8 * j;
        gst(m, p);
        gst(m + 1, r0);
        gst(m + 2, brow[g + e]);
        gst(m + 3, e + 1);
        gst(m + 4, f.x);
        gst(m + 5, xl);
        gst(m + 6, f.z);
        gst(m + 7, yl);
        CatItem it;
        it.xrow = (long long)(xl - 1) * P.n + f.x + xl - 1;
        it.yrow = (long long)(yl - 1) * P.m + f.z + yl - 1;
        items[j] = it;
        j++;
    }
}

// Outputs [0, min(total, cap)), SVX_CAT_ROWS_PER_BLOCK per workgroup.
template <typename QE, int NT>
__global__ __launch_bounds__(256) void k_cat_gather_unit(const CatPair* __restrict__ pairs, const CatItem* __restrict__ items,
                                                         const int* __restrict__ meta, const long long* __restrict__ total,
                                                         long long cap, int d, int bf, char* __restrict__ x_rows, char* __restrict__ y_rows,
                                                         uint16_t* __restrict__ x_unit, uint16_t* __restrict__ y_unit) {
    using S = typename QE::storage;
    const long long have = *total, stop = have < cap ? have : cap;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long first = (long long)blockIdx.x * SVX_CAT_ROWS_PER_BLOCK;
    for (long long o = first + w; o < first + SVX_CAT_ROWS_PER_BLOCK && o < stop; o += 4) {
        const CatItem it = items[o];
        const CatPair* P = pairs + gld(meta + 8 * o);
        move_unit<QE, NT>(reinterpret_cast<const S*>(P->v[0]) + (size_t)it.xrow * d, reinterpret_cast<const S*>(P->v[1]) + (size_t)it.yrow * d,
                          o, d, bf, x_rows, y_rows, x_unit, y_unit, lane);
    }
}

__global__ __launch_bounds__(256) void k_cat_gather_raw(const CatPair* __restrict__ pairs, const CatItem* __restrict__ items,
                                                        const int* __restrict__ meta, const long long* __restrict__ total,
                                                        long long cap, int pieces, uint4* __restrict__ x_rows, uint4* __restrict__ y_rows) {
    const long long have = *total, stop = have < cap ? have : cap;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long first = (long long)blockIdx.x * SVX_CAT_ROWS_PER_BLOCK;
    for (long long o = first + w; o < first + SVX_CAT_ROWS_PER_BLOCK && o < stop; o += 4) {
        const CatItem it = items[o];
        const CatPair* P = pairs + gld(meta + 8 * o);
        move_raw(reinterpret_cast<const uint4*>(P->v[0]) + (size_t)it.xrow * pieces, reinterpret_cast<const uint4*>(P->v[1]) + (size_t)it.yrow * pieces,
                 o, pieces, x_rows, y_rows, lane);
    }
}

// ------------------------------------------------------------------------------ host side
// The argument checks the two calls share; `who` is the entry point's name.  -> the chunks and the alignment rows of the batch.
int rows_check_args(svx_ctx* ctx, const char* who, int dtype, int d, const svx_pair* pairs, int n_pairs, int64_t cap, const void* x_rows,
                    const void* y_rows, const void* x_unit, const void* y_unit, int unit_dtype, const void* ids, long long* n_chunks,
                    long long* n_rows) {
    NEED(ctx, n_pairs >= 0 && cap >= 0, "%s: negative n_pairs or cap", who);
    NEED(ctx, n_pairs == 0 || pairs, "%s: pairs is NULL", who);
    NEED(ctx, dtype == SVX_F32 || dtype == SVX_F16 || dtype == SVX_BF16, "%s: unknown dtype %d", who, dtype);
    NEED(ctx, (x_unit == nullptr) == (y_unit == nullptr), "%s: x_unit and y_unit are given together or not at all", who);
    if (x_unit) {
        NEED(ctx, unit_dtype == SVX_F16 || unit_dtype == SVX_BF16, "%s: unit rows are kept in fp16 or bf16 (got dtype %d)", who, unit_dtype);
        NEED(ctx, d > 0 && d % 32 == 0 && d <= 32 * KNN_KSTEPS,
             "%s: embedding dimension %d: with unit rows it must be a positive multiple of 32, at most %d", who, d, 32 * KNN_KSTEPS);
    } else {
        NEED(ctx, d > 0 && d % 8 == 0 && d <= SVX_MAX_DIM, "%s: embedding dimension %d: must be a positive multiple of 8, at most %d", who, d,
             SVX_MAX_DIM);
    }
    if (cap > 0 && n_pairs > 0) {
        NEED(ctx, x_rows && y_rows && ids, "%s: null output buffer", who);
        NEED(ctx, aligned16(x_rows) && aligned16(y_rows) && aligned16(x_unit) && aligned16(y_unit), "%s: the row buffers must be 16-byte aligned", who);
    }
    *n_chunks = *n_rows = 0;
    for (int p = 0; p < n_pairs; p++) {
        const svx_pair& q = pairs[p];
        NEED(ctx, q.n >= 0 && q.m >= 0 && q.k0 >= 1 && q.k1 >= 1, "%s: pair %d: sizes n=%d m=%d k0=%d k1=%d", who, p, q.n, q.m, q.k0, q.k1);
        NEED(ctx, q.align && q.scores && q.info, "%s: pair %d: null align / scores / info", who, p);
        NEED(ctx, (q.vecs0 || q.n == 0) && (q.vecs1 || q.m == 0), "%s: pair %d: null vecs", who, p);
        NEED(ctx, aligned16(q.vecs0) && aligned16(q.vecs1), "%s: pair %d: vecs must be 16-byte aligned", who, p);
        NEED(ctx, (long long)q.n + q.m + 2 <= 0x7fffffffLL, "%s: pair %d: too many alignment rows", who, p);
        *n_chunks += ((long long)q.n + q.m + 2 + SVX_AR_CHUNK - 1) / SVX_AR_CHUNK;
        *n_rows += (long long)q.n + q.m + 2;
    }
    return SVX_OK;
}

// The common part of pair p's descriptor and the pair's entries of the chunk table; `at`: the chunks so far.
void rows_fill_pair(RowsPair& r, const svx_pair& q, int p, RowsChunk* hc, long long& at) {
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

}  // namespace

extern "C" int svx_alignment_rows(svx_ctx* ctx, int dtype, int d, const svx_pair* pairs, int n_pairs, double max_score, int64_t cap,
                                  void* x_rows, void* y_rows, void* x_unit, void* y_unit, int unit_dtype, int32_t* src,
                                  int64_t* count) {
    if (!ctx) return svx_fail(nullptr, SVX_ERR_ARG, "svx_alignment_rows: ctx is NULL");
    NEED(ctx, count, "svx_alignment_rows: count is NULL");
    long long n_chunks, n_rows;
    int rc = rows_check_args(ctx, "svx_alignment_rows", dtype, d, pairs, n_pairs, cap, x_rows, y_rows, x_unit, y_unit, unit_dtype, src, &n_chunks,
                             &n_rows);
    if (rc) return rc;
    NEED(ctx, n_chunks <= 0x7fffffffLL, "svx_alignment_rows: %lld chunks of alignment rows", n_chunks);
    const bool unit = x_unit != nullptr, writes = cap > 0 && n_pairs > 0;
    rc = svx_flush(ctx);  // with the software pipeline on, the alignment outputs are complete only behind this
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    if (n_pairs == 0) {
        SVX_HIP(ctx, hipMemsetAsync(count, 0, sizeof(int64_t), st));
        return SVX_OK;
    }
    // ---- scratch: [descriptors][chunk table][chunk counts][chunk offsets + 1]; the first two are uploaded
    const size_t b_desc = up256((size_t)n_pairs * sizeof(RowsPair)), b_tab = up256((size_t)n_chunks * sizeof(RowsChunk));
    const size_t b_cnt = up256((size_t)n_chunks * sizeof(int)), b_off = up256(((size_t)n_chunks + 1) * sizeof(long long));
    const size_t b_up = b_desc + b_tab;
    char *pin, *dev;
    rc = svxl_scratch_begin(ctx, "svx_alignment_rows", b_up, b_up + b_cnt + b_off, &pin, &dev);
    if (rc) return rc;
    RowsPair* hp = reinterpret_cast<RowsPair*>(pin);
    RowsChunk* hc = reinterpret_cast<RowsChunk*>(pin + b_desc);
    long long at = 0;
    for (int p = 0; p < n_pairs; p++) rows_fill_pair(hp[p], pairs[p], p, hc, at);
    rc = svxl_scratch_upload(ctx, b_up);
    if (rc) return rc;
    const RowsPair* dp = reinterpret_cast<const RowsPair*>(dev);
    const RowsChunk* dc = reinterpret_cast<const RowsChunk*>(dev + b_desc);
    int* dcnt = reinterpret_cast<int*>(dev + b_up);
    long long* doff = reinterpret_cast<long long*>(dev + b_up + b_cnt);
    const dim3 grid((unsigned)n_chunks), block(SVX_AR_CHUNK);
    k_rows_count<<<grid, block, 0, st>>>(dp, dc, max_score, dcnt);
    SVX_LAUNCH_CHECK(ctx, "k_rows_count");
    k_scan<<<dim3(1), dim3(256), 0, st>>>(dcnt, (int)n_chunks, doff, nullptr, reinterpret_cast<long long*>(count));
    SVX_LAUNCH_CHECK(ctx, "k_scan");
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

extern "C" int svx_concat_rows(svx_ctx* ctx, int dtype, int d, const svx_pair* pairs, const svx_frames* frames, int n_pairs,
                               const svx_concat_params* prm, int64_t cap, void* x_rows, void* y_rows, void* x_unit, void* y_unit,
                               int unit_dtype, int32_t* meta, int64_t* counts) {
    if (!ctx) return svx_fail(nullptr, SVX_ERR_ARG, "svx_concat_rows: ctx is NULL");
    NEED(ctx, counts, "svx_concat_rows: counts is NULL");
    NEED(ctx, prm, "svx_concat_rows: params is NULL");
    long long n_chunks, n_rows;
    int rc = rows_check_args(ctx, "svx_concat_rows", dtype, d, pairs, n_pairs, cap, x_rows, y_rows, x_unit, y_unit, unit_dtype, meta, &n_chunks,
                             &n_rows);
    if (rc) return rc;
    NEED(ctx, prm->max_num_align >= 1 && prm->max_num_align <= SVX_CONCAT_MAX, "svx_concat_rows: max_num_align %d: must be 1 .. %d",
         prm->max_num_align, SVX_CONCAT_MAX);
    const bool need_frames = prm->max_num_align > 1 || prm->min_frames > 0;
    NEED(ctx, frames || !need_frames || n_pairs == 0, "svx_concat_rows: frames is NULL: joining and the duration filter need the segment timestamps");
    NEED(ctx, !need_frames || prm->sample_rate > 0, "svx_concat_rows: sample_rate %d: must be positive", prm->sample_rate);
    NEED(ctx, !need_frames || (prm->max_sil == prm->max_sil && prm->max_dur == prm->max_dur), "svx_concat_rows: max_sil / max_dur is NaN");
    for (int p = 0; need_frames && p < n_pairs; p++)
        NEED(ctx, (frames[p].src || pairs[p].n == 0) && (frames[p].tgt || pairs[p].m == 0), "svx_concat_rows: pair %d: null frames", p);
    NEED(ctx, n_rows <= 0x7fffffffLL, "svx_concat_rows: %lld alignment rows in one batch", n_rows);
    const bool unit = x_unit != nullptr, writes = cap > 0 && n_pairs > 0;
    rc = svx_flush(ctx);  // with the software pipeline on, the alignment outputs are complete only behind this
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    if (n_pairs == 0) {
        SVX_HIP(ctx, hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
        return SVX_OK;
    }
    // ---- scratch: [descriptors][chunk table][first chunk of every pair] uploaded, then [chunk counts][chunk offsets + 1]
    //      [base spans][base rows][base pairs][block fits][block wides][block offsets + 1][items]
    const long long n_blocks = (n_rows + SVX_AR_CHUNK - 1) / SVX_AR_CHUNK;
    const long long most = n_rows * prm->max_num_align, n_items = writes ? ((long long)cap < most ? (long long)cap : most) : 0;
    const size_t b_desc = up256((size_t)n_pairs * sizeof(CatPair)), b_tab = up256((size_t)n_chunks * sizeof(RowsChunk));
    const size_t b_pf = up256(((size_t)n_pairs + 1) * sizeof(int));
    const size_t b_cnt = up256((size_t)n_chunks * sizeof(int)), b_off = up256(((size_t)n_chunks + 1) * sizeof(long long));
    const size_t b_span = up256((size_t)n_rows * sizeof(int4)), b_row = up256((size_t)n_rows * sizeof(int));
    const size_t b_fit = up256((size_t)n_blocks * sizeof(int)), b_off2 = up256(((size_t)n_blocks + 1) * sizeof(long long));
    const size_t b_items = up256((size_t)n_items * sizeof(CatItem));
    const size_t b_up = b_desc + b_tab + b_pf;
    const size_t b_all = b_up + b_cnt + b_off + b_span + 2 * b_row + 2 * b_fit + b_off2 + b_items;
    char *pin, *at_dev;
    rc = svxl_scratch_begin(ctx, "svx_concat_rows", b_up, b_all, &pin, &at_dev);
    if (rc) return rc;
    CatPair* hp = reinterpret_cast<CatPair*>(pin);
    RowsChunk* hc = reinterpret_cast<RowsChunk*>(pin + b_desc);
    int* hf = reinterpret_cast<int*>(pin + b_desc + b_tab);
    long long at = 0;
    for (int p = 0; p < n_pairs; p++) {
        hf[p] = (int)at;
        rows_fill_pair(hp[p], pairs[p], p, hc, at);
        hp[p].fr[0] = need_frames ? frames[p].src : nullptr;
        hp[p].fr[1] = need_frames ? frames[p].tgt : nullptr;
    }
    hf[n_pairs] = (int)at;
    rc = svxl_scratch_upload(ctx, b_up);
    if (rc) return rc;
    auto take = [&at_dev](size_t b) { char* p = at_dev; at_dev += b; return p; };
    const CatPair* dp = reinterpret_cast<const CatPair*>(take(b_desc));
    const RowsChunk* dc = reinterpret_cast<const RowsChunk*>(take(b_tab));
    const int* dpf = reinterpret_cast<const int*>(take(b_pf));
    int* dcnt = reinterpret_cast<int*>(take(b_cnt));
    long long* doff = reinterpret_cast<long long*>(take(b_off));
    int4* dspan = reinterpret_cast<int4*>(take(b_span));
    int* drow = reinterpret_cast<int*>(take(b_row));
    int* dpair = reinterpret_cast<int*>(take(b_row));
    int* dfit = reinterpret_cast<int*>(take(b_fit));
    int* dwide = reinterpret_cast<int*>(take(b_fit));
    long long* doff2 = reinterpret_cast<long long*>(take(b_off2));
    CatItem* ditems = reinterpret_cast<CatItem*>(take(b_items));
    CatParams C;
    C.max_score = prm->max_score;
    C.max_sil = prm->max_sil;
    C.max_dur = prm->max_dur;
    C.rate = (double)prm->sample_rate;
    C.min_frames = prm->min_frames;
    C.max_num = prm->max_num_align;
    C.both = prm->both_sides != 0;
    const dim3 grid((unsigned)n_chunks), grid2((unsigned)n_blocks), block(SVX_AR_CHUNK);
    k_cat_base_count<<<grid, block, 0, st>>>(dp, dc, C.max_score, dcnt);
    SVX_LAUNCH_CHECK(ctx, "k_cat_base_count");
    k_scan<<<dim3(1), dim3(256), 0, st>>>(dcnt, (int)n_chunks, doff, nullptr, nullptr);
    SVX_LAUNCH_CHECK(ctx, "k_scan");
    k_cat_base_write<<<grid, block, 0, st>>>(dp, dc, doff, C.max_score, dspan, drow, dpair);
    SVX_LAUNCH_CHECK(ctx, "k_cat_base_write");
    k_cat_out_count<<<grid2, block, 0, st>>>(dp, dpf, doff, (int)n_chunks, C, dspan, dpair, dfit, dwide);
    SVX_LAUNCH_CHECK(ctx, "k_cat_out_count");
    k_scan<<<dim3(1), dim3(256), 0, st>>>(dfit, (int)n_blocks, doff2, dwide, reinterpret_cast<long long*>(counts));
    SVX_LAUNCH_CHECK(ctx, "k_scan");
    if (!writes) return SVX_OK;
    k_cat_out_write<<<grid2, block, 0, st>>>(dp, dpf, doff, (int)n_chunks, C, dspan, drow, dpair, doff2, (long long)cap, meta, ditems);
    SVX_LAUNCH_CHECK(ctx, "k_cat_out_write");
    const dim3 grid3((unsigned)((n_items + SVX_CAT_ROWS_PER_BLOCK - 1) / SVX_CAT_ROWS_PER_BLOCK));
    const long long* dtotal = doff2 + n_blocks;
    if (unit) {
        const int bf = unit_dtype == SVX_BF16;
        char* xr = reinterpret_cast<char*>(x_rows);
        char* yr = reinterpret_cast<char*>(y_rows);
        uint16_t* xu = reinterpret_cast<uint16_t*>(x_unit);
        uint16_t* yu = reinterpret_cast<uint16_t*>(y_unit);
#define G(QE, NT) k_cat_gather_unit<QE, NT><<<grid3, dim3(256), 0, st>>>(dp, ditems, meta, dtotal, (long long)cap, d, bf, xr, yr, xu, yu)
#define GD(QE) do { if (d <= 512) G(QE, 1); else G(QE, 2); } while (0)
        if (dtype == SVX_F32) GD(ElemF32);
        else if (dtype == SVX_F16) GD(ElemF16);
        else GD(ElemBF16);
#undef GD
#undef G
    } else {
        const int pieces = d * (dtype == SVX_F32 ? 4 : 2) / 16;
        k_cat_gather_raw<<<grid3, dim3(256), 0, st>>>(dp, ditems, meta, dtotal, (long long)cap, pieces, reinterpret_cast<uint4*>(x_rows),
                                                      reinterpret_cast<uint4*>(y_rows));
    }
    SVX_LAUNCH_CHECK(ctx, "k_cat_gather");
    return SVX_OK;
}
