// svx_tile_plan.h -- what the two tile sweeps share (svx_tiles.hip: k_band_tiles, forward; svx_tiles_bwd.hip:
// k_band_tiles_bwd, backward with the fused cut minimum): the tile geometry, the plan of the two LDS-resident shapes,
// the phase stamps and the epilogue that turns MFMA accumulators into cost planes.  DESIGN.md 6, 6f.  gfx950 only.
#pragma once
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

}  // namespace
