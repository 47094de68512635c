// svx_tile_plan.h -- what the tile sweeps share (svx_tiles.hip: k_band_tiles and k_band_tiles_gen, forward;
// svx_tiles_bwd.hip: k_band_tiles_bwd, backward with the fused cut minimum): the tile geometry, the plan of the two
// LDS-resident shapes, the phase stamps, the epilogue that turns MFMA accumulators into cost planes, and the scaffold of the
// persistent tile loop -- ticket claim, band offsets, neighbour wait, halo fill, publish -- with the sweep's direction as a
// compile-time parameter, the eight-lane (total, move) merge, and the host side of the SVX_TILE_PROF diagnostic.
// DESIGN.md 6, 6f.  gfx950 only.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "svx_common.h"
#include "svx_slab.h"

namespace {

constexpr int TL = 32;             // tile side in DP nodes
constexpr int TT_THREADS = 256, TT_WAVES = 4, TT_SLAB = SLAB_BYTES;
constexpr int TT_MAXSLOT = 12, TT_MAXT = 16, TT_HALO = 8;
constexpr int CS_W = TL + TT_HALO;  // csum tile with halo

struct TilePlan {
    int nt, nslot, halo;
    int slot_info[TT_MAXSLOT];  // side << 8 | layer
    int type_slots[TT_MAXT];    // x slot | y slot << 8
};

template <typename E, int NSLOT, int UPW, int S>
struct TileCfg {
    using Ring = SlabRing<E, TL, NSLOT, TT_WAVES, S>;   // svx_slab.h: stage size, DMA pieces, the k loop
    static constexpr int TPP = TT_WAVES * UPW / 2;
    static_assert(TPP <= TT_MAXT && NSLOT <= TT_MAXSLOT, "plan limits");
};

// (diagnostic build-in: with SVX_TILE_PROF=1 thread 0 sums the 100 MHz ticks of every phase into prof[0..6])
struct TileStamp {
    unsigned long long* prof;
    unsigned long long t_prev;
    __device__ __forceinline__ explicit TileStamp(unsigned long long* p) : prof(p), t_prev(p ? __builtin_amdgcn_s_memrealtime() : 0) {}
    __device__ __forceinline__ void operator()(int slot) {
        if (prof && threadIdx.x == 0) {
            const unsigned long long now = __builtin_amdgcn_s_memrealtime();
            atomicAdd(prof + slot, now - t_prev);
            t_prev = now;
        }
    }
};

// The cost planes of a wave's units: accumulators x the two inverse norms -> costs in double like the reference.
// plane_of(type of the pass) names the type's sizes, the first staged rows of its two slots and where the plane goes:
// cell (x row, y row) at dst[(x * TL + y) * YS] -- YS = 1: the LDS planes of k_band_tiles, 8: k_band_tiles_gen's
// slice of global scratch.
struct TilePlane {
    int p, q, xsl, ysl;
    float* dst;
};
template <int UPW, int YS, class PlaneOf>
__device__ __forceinline__ void tile_cost_planes(const f32x4_t (&acc)[UPW][2], int nunits, int wave, int lane, const float* snrm,
                                                 const float* sinv, PlaneOf plane_of) {
    const int lrow = lane & 15, lkg = lane >> 4;
#pragma unroll
    for (int u2 = 0; u2 < UPW; u2++) {
        const int u = wave + TT_WAVES * u2;
        if (u >= nunits) continue;
        const int xt = u % 2;
        const TilePlane tp = plane_of(u / 2);
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int yloc = 16 * j + lrow;
            const float ny = snrm[tp.ysl + yloc], iy = sinv[tp.ysl + yloc];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int xloc = 16 * xt + 4 * lkg + r;
                const float sumx = acc[u2][j][r] * sinv[tp.xsl + xloc] * iy;
                tp.dst[(xloc * TL + yloc) * YS] = cost_formula(sumx, tp.p, tp.q, snrm[tp.xsl + xloc], ny);
            }
        }
    }
}

// ---- the scaffold of the persistent tile loop ---------------------------------------------------------------------------
// A kernel's loop reads: tile_claim, its cost planes (phase 1), tile_band_offsets, tile_wait, tile_halo_fill, its node
// diagonals (phase 3), tile_publish.  BWD = false: the forward sweep (a tile reads the tiles above and to the left);
// BWD = true: the backward sweep (reverse tickets; below and to the right).

// The last entry e of [lo, hi] with gpref[e] <= tk (gpref[lo] <= tk holds).
__device__ __forceinline__ long long tile_bisect(const int* __restrict__ gpref, int tk, long long lo, long long hi) {
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (gpref[mid] <= tk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The (diagonal, pair) entry of forward ticket tk: the last e with gpref[e] <= tk, searched forward from the workgroup's
// previous entry (tickets grow).  Gallop, then bisect: a workgroup's next ticket is usually a few entries ahead.
__device__ __forceinline__ long long tile_entry(const int* __restrict__ gpref, long long nent, int tk, long long ecur) {
    if (gpref[ecur + 1] <= tk) {
        long long step = 1, lo = ecur + 1, hi = nent - 1;
        while (lo + step < nent && gpref[lo + step] <= tk) { lo += step; step <<= 1; }
        if (lo + step < hi) hi = lo + step;
        ecur = tile_bisect(gpref, tk, lo, hi);
    }
    return ecur;
}

struct TileAt {
    int s, p, I, J;   // tile anti-diagonal, pair of the batch (-1: no ticket is left), tile row, tile column
};

// The top of the loop: one ticket per tile, taken by thread 0 between two barriers (the first: the previous tile is finished
// with LDS).  Forward tickets run in (tile anti-diagonal, pair) order, so every dependency of a ticket has a smaller number
// and is claimed by a running workgroup: no deadlock under any dispatch order.  The backward sweep turns the order round:
// reverse ticket k is forward ticket total - 1 - k.  ecur is the workgroup's previous entry (start: 0 forward, nent - 1
// backward); it only moves one way.
template <bool BWD>
__device__ __forceinline__ TileAt tile_claim(const SvxPairDev* __restrict__ pairs, int n_pairs, const int* __restrict__ gpref, long long nent,
                                             int total, int* ticket, int* sh_ticket, long long& ecur, TileStamp& stamp) {
    __syncthreads();
    stamp(6);
    if (threadIdx.x == 0) *sh_ticket = atomicAdd(ticket, 1);
    __syncthreads();
    if (*sh_ticket >= total) return TileAt{0, -1, 0, 0};
    const int tk = BWD ? total - 1 - *sh_ticket : *sh_ticket;
    ecur = BWD ? tile_bisect(gpref, tk, 0, ecur) : tile_entry(gpref, nent, tk, ecur);   // (gpref[0] = 0)
    const int s = (int)(ecur / n_pairs), p = (int)(ecur % n_pairs);
    const int I = pairs[p].t_lo[s] + (tk - gpref[ecur]);
    return TileAt{s, p, I, s - I};
}

// Band offsets of the node diagonals a = abase .. abase + n - 1 that the tile and its halo touch, into LDS.
__device__ __forceinline__ void tile_band_offsets(int* bo_l, const int* __restrict__ boff_out, int abase, int n, int A) {
    for (int i = threadIdx.x; i < n; i += TT_THREADS) {
        const int a = abase + i;
        bo_l[i] = (a >= 0 && a < A + 2) ? boff_out[a] : (1 << 28);  // (no such diagonal: nothing is in its band)
    }
}

// Lattice and band of the tile's pair: node (x, y) is a band cell iff 0 <= x <= xs, 0 <= y <= ys, 0 <= y - bo[x + y] < B.
struct TileBand {
    int xs, ys, B, abase;
    const int* bo_l;   // tile_band_offsets from abase on
    __device__ __forceinline__ bool cell(int xx, int yy, size_t* o) const {   // *o: the node's place in an [A + 2][B] plane
        if (xx < 0 || yy < 0 || xx > xs || yy > ys) return false;
        const int a = xx + yy, b = yy - bo_l[a - abase];
        *o = (size_t)a * B + b;
        return b >= 0 && b < B;
    }
};

// The float64 tile in LDS (csum forward, Bk backward): node (32 I + i, 32 J + j) at pos(i, j); the halo is hx rows and hy
// columns deep, above and to the left forward (i >= -hx, j >= -hy), below and to the right backward (i < 32 + hx, j < 32 + hy).
struct TileGeo {
    int hx, hy, stride, oi, oj;
    __device__ __forceinline__ int pos(int i, int j) const { return (i + oi) * stride + (j + oj); }
};

__device__ __forceinline__ int tile_flag_at(const SvxPairDev& P, int s, int I) { return P.t_pref[s] + (I - P.t_lo[s]); }

// ---- The hand-off between tiles, and why it is sound (MI355X_MICROARCH.md, "hand-offs with sc1 loads"; tile_wait,
// tile_halo_fill and tile_publish are its three parts and the only code that touches a flag):
//   producer (tile_publish)   every node a later tile can read -- the `edge` nodes, within the halo depth of the side the
//                             sweep moves towards -- is stored sc1 (relaxed agent-scope atomic store); EVERY wave then drains
//                             its stores (s_waitcnt vmcnt(0)); a workgroup barrier; only then does one lane store the flag.
//                             The interior follows with plain stores: no tile reads it (the traceback kernel and
//                             k_slack_wide do, behind the kernel boundary).
//   consumer (tile_wait,      the flags are polled with sc1 loads, one lane per neighbour tile; a workgroup barrier; then
//             tile_halo_fill) EVERY load of a neighbour's node is an sc1 load to registers.  No agent-scope acquire is
//                             needed, and none of these bytes is ever read by a plain load while tiles are in flight.
//   one persistent workgroup per CU, hipMalloc memory, 8-byte payload, 4-byte flag: one row of that guide's table.
// The wait is bounded: a neighbour's (reverse) ticket is smaller, so its workgroup is running; the bound only turns a
// programming error into SVX_ERR_HIP in the pair's status instead of a hung GPU.

// Waits for the band tiles of the ri x rj rectangle of neighbours whose nodes the halo holds (own tile excluded): rows
// I - ri .. I, columns J - rj .. J forward; I .. I + ri, J .. J + rj backward.  flags: P.t_flag forward, the call's own backward.
template <bool BWD>
__device__ __forceinline__ void tile_wait(const SvxPairDev& P, const int* flags, int I, int J, int ri, int rj) {
    const int nnb = (ri + 1) * (rj + 1) - 1;
    for (int e = threadIdx.x; e < nnb; e += TT_THREADS) {
        const int q = BWD ? e + 1 : e;   // (the own tile is the rectangle's first backward, its last forward)
        const int ni = BWD ? I + q / (rj + 1) : I - ri + q / (rj + 1), nj = BWD ? J + q % (rj + 1) : J - rj + q % (rj + 1);
        const int ns = ni + nj;
        if (BWD ? ns >= P.t_nd : (ni < 0 || nj < 0)) continue;
        const int off = ni - P.t_lo[ns];
        if (off < 0 || off >= P.t_cnt[ns]) continue;  // not a band tile: nothing to wait for
        const int* flag = flags + tile_flag_at(P, ns, ni);
        long spins = 0;
        while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 && spins < (1l << 25)) {
            __builtin_amdgcn_s_sleep(2);
            spins++;
        }
        if (spins >= (1l << 25)) *P.status = SVX_ERR_HIP;
    }
    __syncthreads();
}

// The tile cs[0 .. ncs) (its spare +inf cells included) is cleared to +inf, then the halo nodes that are band cells are
// loaded from the neighbours' results in `plane`; nodes that do not exist or lie outside the band stay +inf (a move from /
// into them never wins).  Halo positions: hx rows of 32 + hy, then 32 rows of hy columns; NB per thread and round, their
// loads in flight together.  On return the tile is complete for every wave.
template <bool BWD, int NB>
__device__ __forceinline__ void tile_halo_fill(double* cs, int ncs, const TileGeo& g, const TileBand& bd, const double* plane, int I, int J) {
    const int tid = threadIdx.x;
    for (int e = tid; e < ncs; e += TT_THREADS) cs[e] = __builtin_inf();
    __syncthreads();
    const int roww = TL + g.hy, nrows = g.hx * roww, nhalo = nrows + TL * g.hy;
    for (int h0 = 0; h0 < nhalo; h0 += NB * TT_THREADS) {
        unsigned long long hv[NB];
        int hp[NB];
#pragma unroll
        for (int u = 0; u < NB; u++) {
            const int h = h0 + tid + u * TT_THREADS;
            hp[u] = -1;
            hv[u] = 0;
            if (h < nhalo) {
                int ii, jj;
                if (h < nrows) { ii = BWD ? TL + h / roww : h / roww - g.hx; jj = BWD ? h % roww : h % roww - g.hy; }
                else { ii = (h - nrows) / g.hy; jj = BWD ? TL + (h - nrows) % g.hy : (h - nrows) % g.hy - g.hy; }
                size_t o;
                if (bd.cell(TL * I + ii, TL * J + jj, &o)) {
                    hp[u] = g.pos(ii, jj);
                    hv[u] = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(plane) + o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < NB; u++)
            if (hp[u] >= 0) cs[hp[u]] = __longlong_as_double((long long)hv[u]);
    }
    __syncthreads();
}

// The tile's nodes into `plane`: the edge nodes sc1, drain, barrier, the flag, then the interior with plain stores.
// also(o, e) stores what travels with node e = 32 i + j at plane cell o (back-pointers forward, nothing backward).
template <bool BWD, class Also>
__device__ __forceinline__ void tile_publish(const double* cs, const TileGeo& g, const TileBand& bd, double* plane, int* flag, int I, int J,
                                             TileStamp& stamp, Also also) {
    const int tid = threadIdx.x;
    auto store_nodes = [&](bool edge) {
        for (int e = tid; e < TL * TL; e += TT_THREADS) {
            const int i = e / TL, j = e % TL;
            if ((BWD ? (i < g.hx || j < g.hy) : (i >= TL - g.hx || j >= TL - g.hy)) != edge) continue;
            size_t o;
            if (!bd.cell(TL * I + i, TL * J + j, &o)) continue;
            const double v = cs[g.pos(i, j)];
            if (edge) __hip_atomic_store(reinterpret_cast<unsigned long long*>(plane) + o, (unsigned long long)__double_as_longlong(v),
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else plane[o] = v;
            also(o, e);
        }
    };
    store_nodes(true);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    stamp(5);
    store_nodes(false);
}

// ---- the exchanges among a DP node's eight lanes (thread = (node, move slot), slot = tid & 7) ------------------------------
constexpr int DPP_QUAD_1032 = 0xB1, DPP_QUAD_2301 = 0x4E;   // quad_perm [1,0,3,2] (lane ^ 1), [2,3,0,1] (lane ^ 2)
constexpr int DPP_HALF_MIRROR = 0x141, DPP_ROW_MIRROR = 0x140;   // lane k of 8 <-> 7 - k (the other quad); lane k of 16 <-> 15 - k

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {   // (every lane has a source: no old value)
    const unsigned long long u = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)u, CTRL, 0xf, 0xf, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)(u >> 32), CTRL, 0xf, 0xf, true);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

struct DpMerge {
    double tot;
    int key;
};
template <int CTRL>
__device__ __forceinline__ void merge_step(DpMerge& best) {
    const double ot = dpp_f64<CTRL>(best.tot);
    const int ok = __builtin_amdgcn_mov_dpp(best.key, CTRL, 0xf, 0xf, true);
    const bool take = (ot < best.tot) | ((ot == best.tot) & (ok < best.key));
    best.tot = take ? ot : best.tot;
    best.key = take ? ok : best.key;
}
// The best (total, move index) of a node's eight slots, in every one of its lanes, without a short-circuit branch: the
// reference's "first strictly smaller candidate" order.
__device__ __forceinline__ void node_merge(DpMerge& best) {
    merge_step<DPP_QUAD_1032>(best);
    merge_step<DPP_QUAD_2301>(best);
    merge_step<DPP_HALF_MIRROR>(best);
}

// ---- host side --------------------------------------------------------------------------------------------------------
inline bool make_tile_plan(const SvxTypes& ty, int tpp, int nslot_max, TilePlan* plan) {
    memset(plan, 0, sizeof(*plan));
    if (ty.n < 1 || ty.n > tpp) return false;
    int xs[SVX_MAX_TYPES + 2], ys[SVX_MAX_TYPES + 2];
    memset(xs, 0, sizeof(xs));
    memset(ys, 0, sizeof(ys));
    int halo = 1;
    for (int t = 0; t < ty.n; t++) {
        const int lx = ty.x[t] - 1, ly = ty.y[t] - 1;
        if (ty.x[t] > 15 || ty.y[t] > 15) return false;  // packed back-pointers
        if (!xs[lx]) { if (plan->nslot >= nslot_max) return false; plan->slot_info[plan->nslot] = lx; xs[lx] = ++plan->nslot; }
        if (!ys[ly]) { if (plan->nslot >= nslot_max) return false; plan->slot_info[plan->nslot] = (1 << 8) | ly; ys[ly] = ++plan->nslot; }
        plan->type_slots[t] = (xs[lx] - 1) | ((ys[ly] - 1) << 8);
        if (ty.x[t] > halo) halo = ty.x[t];
        if (ty.y[t] > halo) halo = ty.y[t];
    }
    if (halo > TT_HALO) return false;
    plan->nt = ty.n;
    plan->halo = halo;
    return true;
}

inline int tile_cu_count() {
    int dev = 0, ncu = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    return ncu;
}

// LAUNCH(E) for the storage type of the batch.
#define SVX_TILE_BY_DTYPE(dtype, LAUNCH)            \
    do {                                            \
        if ((dtype) == SVX_F32) LAUNCH(ElemF32);    \
        else if ((dtype) == SVX_F16) LAUNCH(ElemF16); \
        else LAUNCH(ElemBF16);                      \
    } while (0)

// The SVX_TILE_PROF diagnostic of a sweep: the stamps' device counters (null when the knob is off).  The buffer does not
// outlive the call that began it: begin() frees it when it fails, end() frees it whatever the launches returned.
struct TileProf {
    unsigned long long* dev = nullptr;
    unsigned long long h[8] = {0};
    int begin(svx_ctx* ctx, hipStream_t st, const char* who) {
        const char* penv = getenv("SVX_TILE_PROF");
        if (!penv || atoi(penv) == 0) return SVX_OK;
        hipError_t e = hipMalloc(&dev, sizeof(h));
        if (e != hipSuccess) { dev = nullptr; return svx_fail(ctx, SVX_ERR_HIP, "%s: hipMalloc: %s", who, hipGetErrorString(e)); }
        e = hipMemsetAsync(dev, 0, sizeof(h), st);
        if (e == hipSuccess) return SVX_OK;
        (void)hipFree(dev);
        dev = nullptr;
        return svx_fail(ctx, SVX_ERR_HIP, "%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    }
    // le: what the launches returned.  -> le, or the first error of the read-back; true from print() only after hipSuccess
    hipError_t end(hipStream_t st, hipError_t le) {
        if (!dev) return le;
        if (le == hipSuccess) le = hipMemcpyAsync(h, dev, sizeof(h), hipMemcpyDeviceToHost, st);
        const hipError_t se = hipStreamSynchronize(st);
        (void)hipFree(dev);
        return le == hipSuccess ? se : le;
    }
    // one line to stderr: nm[i] names what ends at stamp slot i; the caller ends the line
    void print(const char* title, unsigned nwg, const char* const (&nm)[7]) const {
        fprintf(stderr, "[%s, summed over %u workgroups, ms]", title, nwg);
        for (int i = 0; i < 7; i++) fprintf(stderr, " p%d(%s)=%.2f", i, nm[i], (double)h[i] * 1e-5);
    }
};

}  // namespace
