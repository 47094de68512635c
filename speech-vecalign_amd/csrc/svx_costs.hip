// svx_costs.hip -- similarity / cost kernels: coarse dense costs (MFMA) and the sampled path scores
// that feed the deletion-penalty estimate.  (Band costs along the search path: svx_band.hip.)
//
// Reference semantics (paths relative to the reference repository):
//   make_dense_costs   svecalign/vecalign/dp_core.pyx:36-77
//   score_path         svecalign/vecalign/dp_core.pyx:143-161
//
// Design.  A cost is 2pq(1 - <u,v>)/(1e-6 + n0 + n1) with u,v unit rows.  The rows stay in their
// storage type (bf16 / fp16 / fp32, exactly representable products, fp32 accumulate in the matrix
// cores) and the unit-normalisation is applied as the two scalars 1/(||u||+1e-5), 1/(||v||+1e-5)
// in the epilogue, so normalised copies of level 0 are never written to HBM.
#include <stdlib.h>

#include "svx_common.h"
#include "svx_slab.h"   // the vector typedefs and cost_formula

namespace {

constexpr int RS = 144;        // LDS row stride in bytes: 128-byte k-slab + 16 pad (conflict-free b128 reads)

template <typename E>
struct Mma;
// Mma<E>: KS = elements per 128-byte slab, NK = k-steps per slab, frag = one lane's operand of one
// k-step.  `lane_off(lane)` is the lane's byte offset inside a tile (row lane&15, k-group lane>>4).
template <>
struct Mma<ElemBF16> {
    static constexpr int KS = 64, NK = 2, KSTEP_BYTES = 64;
    using frag = uint4;
    __device__ static __forceinline__ int lane_off(int lane) { return (lane & 15) * RS + 16 * (lane >> 4); }
    __device__ static __forceinline__ frag load(const char* p) { return *reinterpret_cast<const uint4*>(p); }
    __device__ static __forceinline__ void mma(f32x4_t& acc, const frag& a, const frag& b) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
    }
};
template <>
struct Mma<ElemF16> {
    static constexpr int KS = 64, NK = 2, KSTEP_BYTES = 64;
    using frag = uint4;
    __device__ static __forceinline__ int lane_off(int lane) { return (lane & 15) * RS + 16 * (lane >> 4); }
    __device__ static __forceinline__ frag load(const char* p) { return *reinterpret_cast<const uint4*>(p); }
    __device__ static __forceinline__ void mma(f32x4_t& acc, const frag& a, const frag& b) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), acc, 0, 0, 0);
    }
};
template <>
struct Mma<ElemF32> {
    static constexpr int KS = 32, NK = 8, KSTEP_BYTES = 16;
    using frag = float;
    __device__ static __forceinline__ int lane_off(int lane) { return (lane & 15) * RS + 4 * (lane >> 4); }
    __device__ static __forceinline__ frag load(const char* p) { return *reinterpret_cast<const float*>(p); }
    __device__ static __forceinline__ void mma(f32x4_t& acc, const frag& a, const frag& b) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    }
};

// Stage one 128-byte k-slab of `nrows` rows into LDS.  rowptr[r] = byte pointer to the row start
// in global memory or nullptr for an all-zero row.
template <typename E>
__device__ __forceinline__ void stage_slab(char* slab, const char* const* rowptr, int nrows, int k0, int d, int tid,
                                           int nthreads) {
    using S = typename E::storage;
    const int npieces = nrows * 8;
    for (int q = tid; q < npieces; q += nthreads) {
        const int r = q >> 3, p = q & 7;
        const char* ptr = rowptr[r];
        const int kel = k0 + p * E::VEC;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (ptr != nullptr && kel < d) v = *reinterpret_cast<const uint4*>(ptr + (size_t)kel * sizeof(S));
        *reinterpret_cast<uint4*>(slab + r * RS + p * 16) = v;
    }
}

// ------------------------------------------------------------------------------ dense costs
struct DenseArgs {
    const void* v0;  // [s0][d] rows of the chosen layer
    const void* v1;
    int s0, s1, d;
    const float* inv0;  // [s0] or null
    const float* inv1;
    const float* n0;  // [s0]
    const float* n1;
    int mul0, mul1;  // (offset0+1), (offset1+1)
    float* costs;    // [s0][s1]
    float* dots;     // optional [s0][s1]: the normalised dot products themselves
};

// One workgroup = a DT x DT block of the cost matrix (DT = 64: every wave owns 32 x 32 = four MFMA tiles, so that a
// staged row is used against 64 rows of the other side instead of 32).
constexpr int DT = 64;
template <typename E>
__device__ void dense_block(const DenseArgs& g, int bx, int by, char* smem) {
    using S = typename E::storage;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;  // 4 waves: 2 x 2 blocks of 32
    const char** rowptr = reinterpret_cast<const char**>(smem);    // 2 * DT rows: x rows then y rows
    char* slab = smem + 2 * DT * sizeof(char*);
    const int x0 = bx * DT, y0 = by * DT;
    if (tid < 2 * DT) {
        const int side = tid >= DT, loc = tid - side * DT;
        const int gi = (side ? y0 : x0) + loc;
        const int nn = side ? g.s1 : g.s0;
        const char* base = reinterpret_cast<const char*>(side ? g.v1 : g.v0);
        rowptr[tid] = (gi < nn) ? base + (size_t)gi * g.d * sizeof(S) : nullptr;
    }
    f32x4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const int xt = wave >> 1, yt = wave & 1;
    for (int k0 = 0; k0 < g.d; k0 += Mma<E>::KS) {
        __syncthreads();
        stage_slab<E>(slab, rowptr, 2 * DT, k0, g.d, tid, blockDim.x);
        __syncthreads();
        const char* ap = slab + xt * 32 * RS + Mma<E>::lane_off(lane);
        const char* bp = slab + (DT + yt * 32) * RS + Mma<E>::lane_off(lane);
#pragma unroll
        for (int ks = 0; ks < Mma<E>::NK; ks++) {
            const typename Mma<E>::frag a0 = Mma<E>::load(ap + ks * Mma<E>::KSTEP_BYTES);
            const typename Mma<E>::frag a1 = Mma<E>::load(ap + 16 * RS + ks * Mma<E>::KSTEP_BYTES);
            const typename Mma<E>::frag b0 = Mma<E>::load(bp + ks * Mma<E>::KSTEP_BYTES);
            const typename Mma<E>::frag b1 = Mma<E>::load(bp + 16 * RS + ks * Mma<E>::KSTEP_BYTES);
            Mma<E>::mma(acc[0][0], a0, b0);
            Mma<E>::mma(acc[0][1], a0, b1);
            Mma<E>::mma(acc[1][0], a1, b0);
            Mma<E>::mma(acc[1][1], a1, b1);
        }
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int y = y0 + yt * 32 + j * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int x = x0 + xt * 32 + i * 16 + (lane >> 4) * 4 + r;
                if (x < g.s0 && y < g.s1) {
                    float sumx = acc[i][j][r];
                    if (g.inv0) sumx = sumx * g.inv0[x] * g.inv1[y];
                    float c = cost_formula(sumx, 1, 1, g.n0[x], g.n1[y]);
                    c = (c * (float)g.mul0) * (float)g.mul1;  // dp_core.pyx:75 (float * int)
                    g.costs[(size_t)x * g.s1 + y] = c;
                    if (g.dots) g.dots[(size_t)x * g.s1 + y] = sumx;
                }
            }
        }
}

template <typename E>
__global__ __launch_bounds__(256) void k_dense_costs(DenseArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    dense_block<E>(g, blockIdx.x, blockIdx.y, smem);
}

template <typename E, bool LV0>
__global__ __launch_bounds__(256) void k_dense_costs_batch(const SvxPairDev* __restrict__ pairs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const SvxPairDev& P = pairs[blockIdx.z];
    if ((P.L == 0) != LV0) return;
    const SvxLevel& Lv = P.lev[P.L];
    DenseArgs g;
    g.s0 = Lv.n[0];
    g.s1 = Lv.n[1];
    if ((int)blockIdx.x * DT >= g.s0 || (int)blockIdx.y * DT >= g.s1) return;
    g.d = P.d;
    g.v0 = LV0 ? P.v[0] : (const void*)Lv.P[0];
    g.v1 = LV0 ? P.v[1] : (const void*)Lv.P[1];
    g.inv0 = LV0 ? Lv.inv[0] : nullptr;
    g.inv1 = LV0 ? Lv.inv[1] : nullptr;
    g.n0 = Lv.nrm[0];
    g.n1 = Lv.nrm[1];
    g.mul0 = 1;
    g.mul1 = 1;
    g.costs = P.dcost;
    g.dots = LV0 ? nullptr : P.ddot;
    dense_block<E>(g, blockIdx.x, blockIdx.y, smem);
}

// ------------------------------------------------------------------------------ score_path
template <typename E, int NCH>
__device__ __forceinline__ float row_dot(const typename E::storage* a, const typename E::storage* b, int d, int lane) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const int col = (c * SVX_WAVE + lane) * E::VEC;
        if (col < d) {
            float x[E::VEC], y[E::VEC];
            load_piece<E>(a + col, x);
            load_piece<E>(b + col, y);
#pragma unroll
            for (int i = 0; i < E::VEC; i++) s += x[i] * y[i];
        }
    }
    return wave_sum(s);
}

struct ScoreArgs {
    const void* v1;  // [rows][d]
    const void* v2;
    const float* inv1;  // or null
    const float* inv2;
    const float* n1;
    const float* n2;
    const int* xx;
    const int* yy;
    int64_t n;
    int rows1, rows2, d;
    float* out;
};

template <typename E, int NCH>
__device__ void score_block(const ScoreArgs& g, int64_t first, int64_t stride) {
    using S = typename E::storage;
    const int lane = threadIdx.x & 63;
    for (int64_t i = first; i < g.n; i += stride) {
        int xi = g.xx[i], yi = g.yy[i];
        xi = xi < 0 ? 0 : (xi >= g.rows1 ? g.rows1 - 1 : xi);  // validated on the host; never fault
        yi = yi < 0 ? 0 : (yi >= g.rows2 ? g.rows2 - 1 : yi);
        float dot = row_dot<E, NCH>(reinterpret_cast<const S*>(g.v1) + (size_t)xi * g.d,
                                    reinterpret_cast<const S*>(g.v2) + (size_t)yi * g.d, g.d, lane);
        if (lane == 0) {
            if (g.inv1) dot = dot * g.inv1[xi] * g.inv2[yi];
            const float den = g.n1[xi] + g.n2[yi];  // float add, no epsilon (dp_core.pyx:161)
            g.out[i] = (float)((2.0 * (1.0 - (double)dot)) / (double)den);
        }
    }
}

template <typename E, int NCH>
__global__ __launch_bounds__(256) void k_score_path(ScoreArgs g) {
    score_block<E, NCH>(g, (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), (int64_t)gridDim.x * 4);
}

// Counting sort of one level's knob samples by source row (one workgroup per (level, pair)):
// korder = sample ids grouped by x, kstart[x] = first position of row x.  max and histogram do not
// care about sample order, so the scoring kernel may visit the samples row by row and read every
// source row once instead of once per sample.
//
// The scatter is staged in LDS when the workgroup's dynamic LDS (`lds_bytes`) holds cnt[n + 1] and ord[kn]: sample ids
// go to ord[pos], and after a barrier korder and kys leave position by position, as full lines (kys gathers ky, an
// 80 KB array that sits in L2).  Scattered straight to memory, the 4-byte stores of a thousand workgroups in flight
// leave L2 as one 32-byte sector each: 5.05 MB written per pair for 0.7 MB of lists.  A level too long for that takes the
// direct scatter in the same workgroup.  The order inside one source row is the arrival order of the atomics either way.
template <int NT>
__device__ __forceinline__ void knob_sort_block(const int* __restrict__ kx, const int* __restrict__ ky, int kn, int n, int m,
                                                int* __restrict__ korder, int* __restrict__ kys, int* __restrict__ kstart,
                                                int* cnt, int* part, size_t lds_bytes) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool staged = ((size_t)n + 1 + (size_t)kn) * sizeof(int) <= lds_bytes;  // uniform for the workgroup
    int* ord = cnt + n + 1;  // [kn], staged way only
    for (int i = tid; i < n; i += NT) cnt[i] = 0;
    __syncthreads();
    for (int i = tid; i < kn; i += NT) {
        int x = kx[i];
        x = x < 0 ? 0 : (x >= n ? n - 1 : x);
        atomicAdd(&cnt[x], 1);
    }
    __syncthreads();
    // exclusive scan: each thread owns a contiguous slice
    const int per = (n + NT - 1) / NT;
    const int lo = tid * per < n ? tid * per : n, hi = (lo + per) < n ? (lo + per) : n;
    int sum = 0;
    for (int i = lo; i < hi; i++) sum += cnt[i];
    int inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    int run = inc - sum;
    for (int w = 0; w < wave; w++) run += part[w];
    for (int i = lo; i < hi; i++) {
        const int v = cnt[i];
        cnt[i] = run;  // becomes the scatter cursor
        kstart[i] = run;
        run += v;
    }
    if (tid == 0) kstart[n] = kn;
    __syncthreads();
    if (staged) {
        for (int i = tid; i < kn; i += NT) {
            int x = kx[i];
            x = x < 0 ? 0 : (x >= n ? n - 1 : x);
            ord[atomicAdd(&cnt[x], 1)] = i;
        }
        __syncthreads();
        for (int p = tid; p < kn; p += NT) {
            const int i = ord[p];
            int y = ky[i];
            y = y < 0 ? 0 : (y >= m ? m - 1 : y);
            korder[p] = i;
            kys[p] = y;
        }
        return;
    }
    for (int i = tid; i < kn; i += NT) {
        int x = kx[i];
        x = x < 0 ? 0 : (x >= n ? n - 1 : x);
        const int pos = atomicAdd(&cnt[x], 1);
        int y = ky[i];
        y = y < 0 ? 0 : (y >= m ? m - 1 : y);
        korder[pos] = i;
        kys[pos] = y;
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void k_knob_sort(const SvxPairDev* __restrict__ pairs, unsigned lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int part[NT / 64];
    const SvxPairDev& P = pairs[blockIdx.y];
    const int level = blockIdx.x;
    if (level > P.L) return;
    if (P.L >= 1 && level == P.L) return;  // the coarsest level's samples are scored unsorted (k_knob_from_dots)
    const SvxLevel& Lv = P.lev[level];
    knob_sort_block<NT>(Lv.kx, Lv.ky, Lv.kn, Lv.n[0], Lv.n[1], Lv.korder, Lv.kys, Lv.kstart, reinterpret_cast<int*>(smem), part,
                        lds_bytes);
}

// svx_knob_sort: the same device code on plain arrays
template <int NT>
__global__ __launch_bounds__(NT) void k_knob_sort_plain(const int* __restrict__ kx, const int* __restrict__ ky, int kn, int n, int m,
                                                        int* __restrict__ korder, int* __restrict__ kys, int* __restrict__ kstart,
                                                        unsigned lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int part[NT / 64];
    knob_sort_block<NT>(kx, ky, kn, n, m, korder, kys, kstart, reinterpret_cast<int*>(smem), part, lds_bytes);
}

// Target rows in flight per wave in k_knob_scores. Measured on the 1024-pair batch (levels >= 1, fp32): 1 -> 15.3 ms,
// 2 -> 14.9 ms, 3 -> 16.6 ms, 4 -> 16.6 ms, 6 -> 18.6 ms: past 2 the registers cost more waves than the depth gains.
constexpr int KNOB_PF = 2;  // target rows in flight per wave in k_knob_scores

// One wave per source row x: the row stays in registers while the wave walks the samples (x, y_s).
// The grid is 1-D over (pair, level) tasks x `bpt` workgroups; after the XCD remap a task's workgroups
// share one XCD, so the randomly gathered target rows of that level are served by one L2 instead of
// being spread over eight.  level = task % nlev + (LV0 ? 0 : 1).
template <typename E, int NCH, bool LV0>
__global__ __launch_bounds__(256) void k_knob_scores(const SvxPairDev* __restrict__ pairs, int nlev, int bpt) {
    using S = typename E::storage;
    constexpr int EPL = NCH * E::VEC;
    const unsigned wg = xcd_remap(blockIdx.x, gridDim.x);
    const int task = wg / bpt, blk = wg % bpt;
    const SvxPairDev& P = pairs[task / nlev];
    const int level = task % nlev + (LV0 ? 0 : 1);
    if (level > P.L) return;
    if (!LV0 && level == P.L) return;  // the coarsest level's samples read the dense stage's dots (k_knob_from_dots)
    const SvxLevel& Lv = P.lev[level];
    const int lane = threadIdx.x & 63;
    const int n = Lv.n[0], d = P.d;
    const S* v1 = LV0 ? reinterpret_cast<const S*>(P.v[0]) : reinterpret_cast<const S*>(Lv.P[0]);
    const S* v2 = LV0 ? reinterpret_cast<const S*>(P.v[1]) : reinterpret_cast<const S*>(Lv.P[1]);
    const float* inv1 = LV0 ? Lv.inv[0] : nullptr;
    const float* inv2 = LV0 ? Lv.inv[1] : nullptr;
    for (int x = blk * 4 + (threadIdx.x >> 6); x < n; x += bpt * 4) {
        const int s0 = gld(Lv.kstart + x), s1 = gld(Lv.kstart + x + 1);
        if (s0 >= s1) continue;  // wave-uniform
        float xr[EPL];
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const int col = (c * SVX_WAVE + lane) * E::VEC;
            if (col < d) {
                gload_piece<E>(v1 + (size_t)x * d + col, xr + c * E::VEC);
            } else {
#pragma unroll
                for (int i = 0; i < E::VEC; i++) xr[c * E::VEC + i] = 0.f;
            }
        }
        const float nx = gld(Lv.nrm[0] + x);
        const float ix = LV0 ? gld(inv1 + x) : 1.0f;
        // The wave walks its samples with PF target rows in flight (a gather is one memory round trip per sample; the
        // register ring keeps PF of them outstanding per wave). Sample ids and target rows come 64 at a time, one per
        // lane, and are handed round with readlane, so no per-sample index load sits in front of a row load.
        constexpr int PF = KNOB_PF;
        const int ns = s1 - s0;
        for (int cb = 0; cb < ns; cb += SVX_WAVE) {
            const int cn = min(SVX_WAVE, ns - cb);
            const int ys_l = lane < cn ? gld(Lv.kys + s0 + cb + lane) : 0;
            const int is_l = lane < cn ? gld(Lv.korder + s0 + cb + lane) : 0;
            const float nrm_l = lane < cn ? gld(Lv.nrm[1] + ys_l) : 0.f;
            const float inv_l = (LV0 && lane < cn) ? gld(inv2 + ys_l) : 1.f;
            float dots_l = 0.f;
            uint4 yraw[PF][NCH];
#pragma unroll
            for (int u = 0; u < PF; u++) {
                const int yu = __builtin_amdgcn_readlane(ys_l, u);
#pragma unroll
                for (int c = 0; c < NCH; c++) {
                    const int col = (c * SVX_WAVE + lane) * E::VEC;
                    yraw[u][c] = (u < cn && col < d) ? gld16(v2 + (size_t)yu * d + col) : make_uint4(0, 0, 0, 0);
                }
            }
            for (int base = 0; base < cn; base += PF) {
#pragma unroll
                for (int u = 0; u < PF; u++) {
                    const int k = base + u;  // sample k of the chunk sits in slot u (PF divides base)
                    if (k >= cn) break;      // wave-uniform
                    float dot = 0.f;
#pragma unroll
                    for (int c = 0; c < NCH; c++) {
                        float yr[E::VEC];
                        decode_piece<E>(yraw[u][c], yr);
#pragma unroll
                        for (int e = 0; e < E::VEC; e++) dot += xr[c * E::VEC + e] * yr[e];
                    }
                    if (k + PF < cn) {  // refill the slot with sample k + PF
                        const int yn = __builtin_amdgcn_readlane(ys_l, k + PF);
#pragma unroll
                        for (int c = 0; c < NCH; c++) {
                            const int col = (c * SVX_WAVE + lane) * E::VEC;
                            yraw[u][c] = col < d ? gld16(v2 + (size_t)yn * d + col) : make_uint4(0, 0, 0, 0);
                        }
                    }
                    dot = wave_sum(dot);
                    dots_l = lane == k ? dot : dots_l;
                }
            }
            // one lane per sample finishes the chunk's scores side by side
            if (lane < cn) {
                float dot = dots_l;
                if (LV0) dot = dot * ix * inv_l;
                const float den = nx + nrm_l;  // float add, no epsilon (dp_core.pyx:161)
                gst(Lv.kscore + is_l, (float)((2.0 * (1.0 - (double)dot)) / (double)den));
            }
        }
    }
}

// Documents too long for the sort's LDS histogram (> ~38 000 segments): the samples are scored in their drawn
// order, one wave per sample (both rows fetched per sample; slower, no size limit).
template <typename E, int NCH, bool LV0>
__global__ __launch_bounds__(256) void k_knob_scores_unsorted(const SvxPairDev* __restrict__ pairs) {
    const SvxPairDev& P = pairs[blockIdx.z];
    const int level = (int)blockIdx.y + (LV0 ? 0 : 1);
    if (level > P.L) return;
    if (!LV0 && level == P.L) return;  // (k_knob_from_dots)
    const SvxLevel& Lv = P.lev[level];
    ScoreArgs g;
    g.v1 = LV0 ? P.v[0] : (const void*)Lv.P[0];
    g.v2 = LV0 ? P.v[1] : (const void*)Lv.P[1];
    g.inv1 = LV0 ? Lv.inv[0] : nullptr;
    g.inv2 = LV0 ? Lv.inv[1] : nullptr;
    g.n1 = Lv.nrm[0];
    g.n2 = Lv.nrm[1];
    g.xx = Lv.kx;
    g.yy = Lv.ky;
    g.n = Lv.kn;
    g.rows1 = Lv.n[0];
    g.rows2 = Lv.n[1];
    g.d = P.d;
    g.out = Lv.kscore;
    score_block<E, NCH>(g, (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), (int64_t)gridDim.x * 4);
}

// Sampled scores of the coarsest level (L >= 1): score_path (dp_core.pyx:143-161) from the dot products that the
// dense cost stage of the same level has just computed on the matrix cores -- no row is read again.
__global__ __launch_bounds__(256) void k_knob_from_dots(const SvxPairDev* __restrict__ pairs) {
    const SvxPairDev& P = pairs[blockIdx.y];
    if (P.L < 1) return;
    const SvxLevel& Lv = P.lev[P.L];
    const int n = Lv.n[0], m = Lv.n[1];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < Lv.kn; i += gridDim.x * 256) {
        int x = Lv.kx[i], y = Lv.ky[i];
        x = x < 0 ? 0 : (x >= n ? n - 1 : x);
        y = y < 0 ? 0 : (y >= m ? m - 1 : y);
        const float dot = P.ddot[(size_t)x * m + y];
        const float den = Lv.nrm[0][x] + Lv.nrm[1][y];  // float add, no epsilon (dp_core.pyx:161)
        Lv.kscore[i] = (float)((2.0 * (1.0 - (double)dot)) / (double)den);
    }
}

inline int nch_f32(int d) {
    int c = (d + 255) / 256;
    return c <= 1 ? 1 : c <= 2 ? 2 : c <= 4 ? 4 : 8;
}
inline int nch_16(int d) {
    int c = (d + 511) / 512;
    return c <= 1 ? 1 : c <= 2 ? 2 : 4;
}

constexpr size_t DENSE_SMEM = 2 * DT * sizeof(char*) + 2 * DT * RS;

}  // namespace

int svxl_dense_costs(svx_ctx* ctx, const float* v0, int s0, const float* v1, int s1, int d, const float* n0,
                     const float* n1, int mul0, int mul1, float* costs) {
    if (s0 <= 0 || s1 <= 0) return SVX_OK;
    DenseArgs g{v0, v1, s0, s1, d, nullptr, nullptr, n0, n1, mul0, mul1, costs, nullptr};
    hipLaunchKernelGGL(k_dense_costs<ElemF32>, dim3((s0 + DT - 1) / DT, (s1 + DT - 1) / DT), dim3(256), DENSE_SMEM, ctx->stream, g);
    SVX_LAUNCH_CHECK(ctx, "k_dense_costs");
    return SVX_OK;
}

int svxl_dense_costs_batch(svx_ctx* ctx, const SvxPairDev* pairs, int n_pairs, int max_s0, int max_s1, int dtype, int d) {
    (void)d;
    if (n_pairs <= 0 || max_s0 <= 0 || max_s1 <= 0) return SVX_OK;
    dim3 grid((max_s0 + DT - 1) / DT, (max_s1 + DT - 1) / DT, n_pairs);
    hipLaunchKernelGGL((k_dense_costs_batch<ElemF32, false>), grid, dim3(256), DENSE_SMEM, ctx->stream, pairs);
    if (dtype == SVX_F32)
        hipLaunchKernelGGL((k_dense_costs_batch<ElemF32, true>), grid, dim3(256), DENSE_SMEM, ctx->stream, pairs);
    else if (dtype == SVX_F16)
        hipLaunchKernelGGL((k_dense_costs_batch<ElemF16, true>), grid, dim3(256), DENSE_SMEM, ctx->stream, pairs);
    else
        hipLaunchKernelGGL((k_dense_costs_batch<ElemBF16, true>), grid, dim3(256), DENSE_SMEM, ctx->stream, pairs);
    SVX_LAUNCH_CHECK(ctx, "k_dense_costs_batch");
    return SVX_OK;
}

int svxl_score_path(svx_ctx* ctx, const int* xx, const int* yy, int64_t n, const float* n1, const float* n2,
                    const float* v1, int rows1, const float* v2, int rows2, int d, float* out) {
    if (n <= 0) return SVX_OK;
    ScoreArgs g{v1, v2, nullptr, nullptr, n1, n2, xx, yy, n, rows1, rows2, d, out};
    int64_t nb = (n + 3) / 4;
    if (nb > 16384) nb = 16384;
#define M(N) hipLaunchKernelGGL((k_score_path<ElemF32, N>), dim3((unsigned)nb), dim3(256), 0, ctx->stream, g)
    switch (nch_f32(d)) {
        case 1: M(1); break;
        case 2: M(2); break;
        case 4: M(4); break;
        default: M(8); break;
    }
#undef M
    SVX_LAUNCH_CHECK(ctx, "k_score_path");
    return SVX_OK;
}

int svxl_knob_from_dots(svx_ctx* ctx, const SvxPairDev* pairs, int n_pairs, int max_kn) {
    if (n_pairs <= 0 || max_kn <= 0) return SVX_OK;
    int nb = (max_kn + 255) / 256;
    if (nb > 16) nb = 16;
    hipLaunchKernelGGL(k_knob_from_dots, dim3(nb, n_pairs), dim3(256), 0, ctx->stream, pairs);
    SVX_LAUNCH_CHECK(ctx, "k_knob_from_dots");
    return SVX_OK;
}

constexpr size_t KNOB_SORT_HIST_LDS = 150 * 1024;                  // the sort's histogram cnt[n + 1] must fit: else the samples are scored unsorted
constexpr size_t KNOB_SORT_STAGE_LDS = SVX_KNOB_SORT_STAGE_LDS;     // cnt[n + 1] + ord[kn] within this: the scatter is staged in LDS
static_assert(KNOB_SORT_STAGE_LDS >= KNOB_SORT_HIST_LDS, "a launch sized for staging must still hold the longest histogram");

// Dynamic LDS of a sort launch for these (batch) maxima: room to stage if that fits the cap, else the cap, under which
// the shorter levels of the batch still stage; never less than the histogram.
static size_t knob_sort_lds(int max_n0, int max_kn) {
    const size_t want = ((size_t)max_n0 + 1 + (size_t)max_kn) * sizeof(int);
    return want < KNOB_SORT_STAGE_LDS ? want : KNOB_SORT_STAGE_LDS;
}

// Threads per sort workgroup.  Measured on the 1024-pair batch (step, median of 5 runs / `knob_sort` stage timer, which
// includes the wait for a CU with the LDS free): 256 -> 104.70 ms / 11.8 ms, 512 -> 104.74, 1024 -> 104.71 / 19.6 ms:
// the step does not care, and the small workgroup finds a CU with four free wave slots sooner than the large one finds
// sixteen beside the pyramid pass.
static int knob_sort_threads() {
    static const int nt = [] {
        const char* e = getenv("SVX_SORT_THREADS");  // tuning override: 256, 512 or 1024
        const int v = e ? atoi(e) : 0;
        return (v == 256 || v == 512 || v == 1024) ? v : 256;
    }();
    return nt;
}

template <int NT>
static int knob_sort_launch(svx_ctx* ctx, const SvxPairDev* pairs, int n_pairs, int max_L, size_t smem) {
    if (smem > 64 * 1024)
        SVX_HIP(ctx, hipFuncSetAttribute((const void*)k_knob_sort<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(k_knob_sort<NT>, dim3(max_L + 1, n_pairs), dim3(NT), smem, ctx->stream, pairs, (unsigned)smem);
    SVX_LAUNCH_CHECK(ctx, "k_knob_sort");
    return SVX_OK;
}

template <int NT>
static int knob_sort_plain_launch(svx_ctx* ctx, const int* kx, const int* ky, int kn, int n, int m, int* korder, int* kys,
                                  int* kstart, size_t smem) {
    if (smem > 64 * 1024)
        SVX_HIP(ctx, hipFuncSetAttribute((const void*)k_knob_sort_plain<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(k_knob_sort_plain<NT>, dim3(1), dim3(NT), smem, ctx->stream, kx, ky, kn, n, m, korder, kys, kstart,
                       (unsigned)smem);
    SVX_LAUNCH_CHECK(ctx, "k_knob_sort_plain");
    return SVX_OK;
}

int svxl_knob_sort(svx_ctx* ctx, const int* kx, const int* ky, int kn, int n, int m, int* korder, int* kys, int* kstart) {
    if ((size_t)(n + 1) * sizeof(int) > KNOB_SORT_HIST_LDS)
        return svx_fail(ctx, SVX_ERR_ARG, "knob_sort: %d source rows exceed the LDS histogram (max %d)", n,
                        (int)(KNOB_SORT_HIST_LDS / sizeof(int)) - 1);
    const size_t smem = knob_sort_lds(n, kn);
    switch (knob_sort_threads()) {
        case 256: return knob_sort_plain_launch<256>(ctx, kx, ky, kn, n, m, korder, kys, kstart, smem);
        case 512: return knob_sort_plain_launch<512>(ctx, kx, ky, kn, n, m, korder, kys, kstart, smem);
        default: return knob_sort_plain_launch<1024>(ctx, kx, ky, kn, n, m, korder, kys, kstart, smem);
    }
}

// part 0: counting sort by source row; part 1: levels >= 1 (fp32 rows); part 2: level 0 (input dtype)
int svxl_knob_scores(svx_ctx* ctx, const SvxPairDev* pairs, int n_pairs, int max_L, int max_kn, int max_n0, int dtype, int d,
                     int part) {
    if (n_pairs <= 0 || max_kn <= 0) return SVX_OK;
    hipStream_t st = ctx->stream;
    const bool unsorted = (size_t)(max_n0 + 1) * sizeof(int) > KNOB_SORT_HIST_LDS;  // the sort's histogram does not fit LDS
    if (unsorted) {
        if (part == 0) return SVX_OK;
        const int nbu = (max_kn + 3) / 4 < 2048 ? (max_kn + 3) / 4 : 2048;
#define U32(N, LV0, GY) hipLaunchKernelGGL((k_knob_scores_unsorted<ElemF32, N, LV0>), dim3(nbu, GY, n_pairs), dim3(256), 0, st, pairs)
#define U16(E, N) hipLaunchKernelGGL((k_knob_scores_unsorted<E, N, true>), dim3(nbu, 1, n_pairs), dim3(256), 0, st, pairs)
        if (part == 1) {
            if (max_L >= 1) {
                switch (nch_f32(d)) {
                    case 1: U32(1, false, max_L); break;
                    case 2: U32(2, false, max_L); break;
                    case 4: U32(4, false, max_L); break;
                    default: U32(8, false, max_L); break;
                }
            }
        } else if (dtype == SVX_F32) {
            switch (nch_f32(d)) {
                case 1: U32(1, true, 1); break;
                case 2: U32(2, true, 1); break;
                case 4: U32(4, true, 1); break;
                default: U32(8, true, 1); break;
            }
        } else if (dtype == SVX_F16) {
            switch (nch_16(d)) {
                case 1: U16(ElemF16, 1); break;
                case 2: U16(ElemF16, 2); break;
                default: U16(ElemF16, 4); break;
            }
        } else {
            switch (nch_16(d)) {
                case 1: U16(ElemBF16, 1); break;
                case 2: U16(ElemBF16, 2); break;
                default: U16(ElemBF16, 4); break;
            }
        }
#undef U32
#undef U16
        SVX_LAUNCH_CHECK(ctx, "k_knob_scores_unsorted");
        return SVX_OK;
    }
    if (part == 0) {
        const size_t smem = knob_sort_lds(max_n0, max_kn);
        switch (knob_sort_threads()) {
            case 256: return knob_sort_launch<256>(ctx, pairs, n_pairs, max_L, smem);
            case 512: return knob_sort_launch<512>(ctx, pairs, n_pairs, max_L, smem);
            default: return knob_sort_launch<1024>(ctx, pairs, n_pairs, max_L, smem);
        }
    }
    int nb = (max_n0 + 3) / 4;  // one wave per source row
    if (nb > 1024) nb = 1024;
#define M32(N, LV0, GY) hipLaunchKernelGGL((k_knob_scores<ElemF32, N, LV0>), dim3((unsigned)nb * (GY) * n_pairs), dim3(256), 0, st, pairs, GY, nb)
#define M16(E, N) hipLaunchKernelGGL((k_knob_scores<E, N, true>), dim3((unsigned)nb * n_pairs), dim3(256), 0, st, pairs, 1, nb)
    if (part == 1 && max_L >= 1) {
        switch (nch_f32(d)) {
            case 1: M32(1, false, max_L); break;
            case 2: M32(2, false, max_L); break;
            case 4: M32(4, false, max_L); break;
            default: M32(8, false, max_L); break;
        }
    }
    if (part != 2) {
    } else if (dtype == SVX_F32) {
        switch (nch_f32(d)) {
            case 1: M32(1, true, 1); break;
            case 2: M32(2, true, 1); break;
            case 4: M32(4, true, 1); break;
            default: M32(8, true, 1); break;
        }
    } else if (dtype == SVX_F16) {
        switch (nch_16(d)) {
            case 1: M16(ElemF16, 1); break;
            case 2: M16(ElemF16, 2); break;
            default: M16(ElemF16, 4); break;
        }
    } else {
        switch (nch_16(d)) {
            case 1: M16(ElemBF16, 1); break;
            case 2: M16(ElemBF16, 2); break;
            default: M16(ElemBF16, 4); break;
        }
    }
#undef M32
#undef M16
    SVX_LAUNCH_CHECK(ctx, "k_knob_scores");
    return SVX_OK;
}
