// svx_tiles.hip -- wide bands (Sakoe-Chiba search around the straight diagonal, and the dense "every cell"
// mode): similarity tiles on the matrix cores feeding the dynamic programme directly, swept as a wavefront of
// tiles over all CUs.
//
// Reference semantics: make_sparse_costs + sparse_dp (svecalign/vecalign/dp_core.pyx:165-267, 269-404) on a
// straight search path (append_slant, dp_utils.py:177-196) with band half-width W -- what
// dp_utils.vecalign() evaluates when max_size_full_dp is large and width_over2 covers the documents
// (Modes B and C).  The first-generation path materialised the [T][A][B] cost tensor (10.7 GB
// at 32768 x 32768, band 2048) and ran the DP of a pair in one workgroup.
//
// Here the lattice of DP nodes (x, y) is cut into 32 x 32 tiles.  A tile's T cost planes are 16 x 16 MFMA blocks
// of the raw 16-bit / fp32 rows (32 rows x all overlap layers per side, LDS-DMA ring of swizzled 64-byte k-slabs:
// SlabRing of svx_slab.h, shared with svx_band.hip), scaled by the two inverse norms and turned into costs in double like the
// reference; they never leave LDS.  The tile's nodes are then relaxed along its 63 anti-diagonals by one wave
// (two half-waves split the moves and merge by (total, move) so that the reference's "first strictly smaller
// candidate" order is kept), reading a 4..8 node halo of the float64 sums of the tiles above and to the left.
// Tiles depend on their upper, left and upper-left neighbours only, so all tiles of a tile anti-diagonal run
// concurrently: persistent workgroups take tickets in (pair, tile anti-diagonal) order -- every dependency of a
// ticket has a smaller number, hence is already claimed by a running workgroup: no deadlock under any dispatch
// order -- compute the cost planes first (they need no neighbour), then wait for the neighbours' flags.
// Results go to the reference's node arrays (csum [A+2][B] float64, packed back-pointers), which the existing
// traceback kernel walks.  Type sets beyond these two LDS-resident shapes run k_band_tiles_gen below (planes through
// a per-workgroup slice of global scratch, halo of the largest step, int32 back-pointers for steps above 15).
// What the two kernels here and the backward sweep of svx_tiles_bwd.hip share is in svx_tile_plan.h: tile geometry, TilePlan,
// the cost-plane epilogue, and the scaffold of the persistent loop (ticket claim, band offsets, neighbour wait, halo fill,
// publish: every flag and every load of a neighbour's node, with the one argument why that hand-off is sound).  The kernels
// below hold their cost phase and their node-diagonal loop.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "svx_common.h"
#include "svx_slab.h"
#include "svx_tile_plan.h"

namespace {

// b_offset_out of a pair, then per tile anti-diagonal s the run of tiles (I, s - I) that hold band nodes.  Everything
// comes from the level's search path: the straight line, or the path of a prior (SVX_SEARCH_AROUND_WIDE).  The run is
// the hull of the band tiles of the diagonal; the band rows of consecutive node diagonals overlap, so it has no holes.
// A pair that has failed by now (a prior the ingest refused, a path error) gets no tiles and takes no ticket.
// Node (x, y) is in the band iff 0 <= y - bo[x + y] < B and 0 <= x <= xs, 0 <= y <= ys.
__global__ __launch_bounds__(256) void k_tile_ranges(const SvxPairDev* __restrict__ pairs, int W, int B) {
    const SvxPairDev& P = pairs[blockIdx.x];
    const SvxLevel& Lv = P.lev[0];
    const int A = *Lv.path_len;
    const int tid = threadIdx.x;
    for (int i = tid; i < P.t_cap; i += 256) P.t_flag[i] = 0;
    if (A <= 0 || *P.status != 0) {
        if (tid == 0) P.t_pref[P.t_nd] = 0;
        for (int s = tid; s < P.t_nd; s += 256) { P.t_cnt[s] = 0; P.t_pref[s] = 0; }
        return;
    }
    const int2* path = reinterpret_cast<const int2*>(Lv.path);
    for (int a = tid; a < A + 2; a += 256) Lv.boff_out[a] = (a < 2 ? path[0].y : path[a - 2].y + 1) - W;
    for (int a = tid; a < A; a += 256) Lv.boff[a] = path[a].y - W;
    __syncthreads();
    const int xs = Lv.n[0], ys = Lv.n[1];
    for (int s = tid; s < P.t_nd; s += 256) {
        int ilo = 1 << 30, ihi = -1;
        for (int r = 0; r <= 2 * (TL - 1); r++) {
            const int a = TL * s + r;
            if (a > xs + ys || a >= A + 2) break;
            const int bo = Lv.boff_out[a];
            int ylo = bo > 0 ? bo : 0, yhi = bo + B - 1;
            if (a - xs > ylo) ylo = a - xs;
            if (yhi > ys) yhi = ys;
            if (yhi > a) yhi = a;
            if (ylo > yhi) continue;
            const int jm_lo = r - (TL - 1) > 0 ? r - (TL - 1) : 0, jm_hi = r < TL - 1 ? r : TL - 1;
            // tiles J on this diagonal whose rows 32 J + [jm_lo, jm_hi] meet [ylo, yhi]
            int jmin = (ylo - jm_hi + TL - 1) / TL;
            if (ylo - jm_hi < 0) jmin = 0;
            const int jmax = (yhi - jm_lo) >= 0 ? (yhi - jm_lo) / TL : -1;
            if (jmin > jmax) continue;
            if (s - jmax < ilo) ilo = s - jmax;
            if (s - jmin > ihi) ihi = s - jmin;
        }
        if (ilo < 0) ilo = 0;
        P.t_lo[s] = ilo <= ihi ? ilo : 0;
        P.t_cnt[s] = ilo <= ihi ? ihi - ilo + 1 : 0;
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int s = 0; s < P.t_nd; s++) {
            P.t_pref[s] = run;
            run += P.t_cnt[s];
        }
        P.t_pref[P.t_nd] = run > P.t_cap ? 0 : run;  // (cannot exceed the capacity plan_half derives for any unit-step path; the guard stays)
        if (run > P.t_cap) *P.status = SVX_ERR_ARG;
    }
}

// Ticket order: tile anti-diagonal s of every pair, then s + 1 of every pair, ...: the pairs of a batch advance
// together, so that the chip sees (pairs x tiles per diagonal) independent tiles instead of one pair's wavefront.
// gpref[s * n_pairs + p] = tickets before (s, p); gpref[max_nd * n_pairs] = total.  One workgroup, blocked scan.
__global__ __launch_bounds__(1024) void k_tile_prefix(const SvxPairDev* __restrict__ pairs, int n_pairs, int max_nd, int* gpref, int* ticket) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const long long n = (long long)max_nd * n_pairs;
    const long long per = (n + 1023) / 1024;
    const long long lo = tid * per, hi = (lo + per) < n ? (lo + per) : n;
    int sum = 0;
    for (long long e = lo; e < hi; e++) {
        const int s = (int)(e / n_pairs), p = (int)(e % n_pairs);
        sum += s < pairs[p].t_nd ? pairs[p].t_cnt[s] : 0;
    }
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 1024; i++) { const int v = part[i]; part[i] = run; run += v; }
        gpref[n] = run;
        *ticket = 0;
    }
    __syncthreads();
    int run = part[tid];
    for (long long e = lo; e < hi; e++) {
        const int s = (int)(e / n_pairs), p = (int)(e % n_pairs);
        gpref[e] = run;
        run += s < pairs[p].t_nd ? pairs[p].t_cnt[s] : 0;
    }
}

template <typename E, int NSLOT, int UPW, int S>
__global__ __launch_bounds__(TT_THREADS) void k_band_tiles(const SvxPairDev* __restrict__ pairs, int n_pairs, SvxTypes ty, TilePlan plan,
                                                           int W, int max_nd, const int* __restrict__ gpref, int* ticket,
                                                           unsigned long long* prof) {
    using C = TileCfg<E, NSLOT, UPW, S>;
    using St = typename E::storage;
    using R = typename C::Ring;
    __shared__ __attribute__((aligned(1024))) char st0[R::STAGE];
    __shared__ __attribute__((aligned(1024))) char st1[R::STAGE];
    __shared__ __attribute__((aligned(1024))) char st2[S >= 3 ? R::STAGE : 16];
    __shared__ __attribute__((aligned(1024))) char st3[S >= 4 ? R::STAGE : 16];
    __shared__ __attribute__((aligned(1024))) char st4[S >= 5 ? R::STAGE : 16];
    __shared__ __attribute__((aligned(16))) float planes[C::TPP * TL * TL];   // [type][x row][y row] costs of the tile
    __shared__ __attribute__((aligned(16))) double cs[CS_W * CS_W + 2];       // csum of the tile's nodes and halo; [CS_W^2] = +inf
    __shared__ unsigned char bpt[TL * TL];
    __shared__ float snrm[NSLOT * TL], sinv[NSLOT * TL];
    __shared__ int bo_l[2 * TL + 2 * TT_HALO + 2];
    __shared__ int tpk[TT_MAXT + 2];
    __shared__ int sh_ticket;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int B = 2 * W, T = ty.n, NTt = T + 2, H = plan.halo;
    const long long nent = (long long)max_nd * n_pairs;
    const int total = gpref[nent];
    for (int t = tid; t < NTt; t += TT_THREADS) tpk[t] = (int)ty.x[t] | ((int)ty.y[t] << 8);
    const double inf = __builtin_inf();
    long long ecur = 0;

    TileStamp stamp(prof);
    for (;;) {
        const TileAt at = tile_claim<false>(pairs, n_pairs, gpref, nent, total, ticket, &sh_ticket, ecur, stamp);
        if (at.p < 0) break;
        const int s = at.s, I = at.I, J = at.J;
        const SvxPairDev& P = pairs[at.p];
        const SvxLevel& Lv = P.lev[0];
        const int xs = Lv.n[0], ys = Lv.n[1], d = P.d;
        const int rowbytes = d * (int)sizeof(St);
        const int NK = (rowbytes + TT_SLAB - 1) / TT_SLAB;
        const int X0 = TL * I - 1, Y0 = TL * J - 1;  // cost cell of node (x, y) is (x - 1, y - 1)
        const int A = *Lv.path_len;
        const double pen = *Lv.pen;

        stamp(0);
        // ---- phase 1: cost planes (no neighbour needed)
        // (the ring of svx_slab.h over the plan's slots: per-row scalars in registers across the k loop, DMA sources, this
        //  wave's units (type, x tile of the two), the k loop)
        const SlabSide sx{P.v[0], Lv.nrm[0], Lv.inv[0], X0, TL, xs}, sy{P.v[1], Lv.nrm[1], Lv.inv[1], Y0, TL, ys};
        auto slot_of = [&](int slot) {
            return slot < plan.nslot ? SlabSlot{plan.slot_info[slot] >> 8, plan.slot_info[slot] & 255} : SlabSlot{-1, 0};
        };
        auto type_slots = [&](int tl) { return SlabPair{plan.type_slots[tl] & 255, plan.type_slots[tl] >> 8}; };
        float r_nrm[R::SPT], r_inv[R::SPT];
        R::row_scalars(slot_of, sx, sy, tid, r_nrm, r_inv);
        typename R::Src src;
        R::sources(slot_of, sx, sy, rowbytes, wave, lane, src);
        f32x4_t acc[UPW][2];
        typename R::template Units<UPW> un;
        const int nunits = T * 2;
        R::template units<UPW, 2>(type_slots, nunits, nullptr, wave, lane, un, acc);
        R::template run<UPW, 2>(NK, src, un, acc, st0, st1, st2, st3, st4);
        R::store_scalars(snrm, sinv, tid, r_nrm, r_inv);
        // band offsets of the node diagonals this tile and its halo touch: a in [32 s - 2 H, 32 s + 62]
        const int abase = TL * s - 2 * H;
        tile_band_offsets(bo_l, Lv.boff_out, abase, 2 * TL + 2 * H, A);
        __syncthreads();
        tile_cost_planes<UPW, 1>(acc, nunits, wave, lane, snrm, sinv, [&](int tl) {
            return TilePlane{tpk[tl] & 255, tpk[tl] >> 8, (plan.type_slots[tl] & 255) * TL, (plan.type_slots[tl] >> 8) * TL, planes + tl * TL * TL};
        });
        stamp(1);
        // ---- phase 2: wait for the neighbours (all three, when they exist, have smaller tickets), then their halo into the
        // csum tile: position (i + 8, j + 8) <-> node (32 I + i, 32 J + j), i, j in [-H, 32); <= 3 halo positions per thread
        // (the hand-off: svx_tile_plan.h)
        const TileBand band{xs, ys, B, abase, bo_l};
        const TileGeo geo{H, H, CS_W, TT_HALO, TT_HALO};
        tile_wait<false>(P, P.t_flag, I, J, 1, 1);
        stamp(2);
        tile_halo_fill<false, 3>(cs, CS_W * CS_W + 2, geo, band, Lv.csum, I, J);
        stamp(3);
        // ---- phase 3: the tile's 63 node anti-diagonals, all four waves: thread = (node j = tid >> 3, move slot = tid & 7).
        // A slot relaxes the moves t = slot, slot + 8, ... (kept in registers, unrolled) with every csum / cost read of the
        // diagonal issued up front and no branch; the eight slots of a node sit in eight adjacent lanes and merge by
        // (total, move index) with three DPP exchanges, so the reference's "first strictly smaller candidate" order holds.
        // Predecessors outside the lattice or the band, and the moves a slot does not have, read a +inf cell.
        {
            constexpr int MS = (C::TPP + 2 + 7) / 8;  // moves per slot: 2 for the 10-type shape (12 moves over 8 slots), 3 for the 16-type one
            const int j = tid >> 3, slot = tid & 7;
            int m_off[MS], m_key[MS], m_plb[MS];
            bool m_ok[MS], m_del[MS];
#pragma unroll
            for (int m = 0; m < MS; m++) {
                const int t = slot + 8 * m;
                const int pk = t < NTt ? tpk[t] : 0;
                m_ok[m] = t < NTt;
                m_off[m] = -((pk & 255) * CS_W + (pk >> 8));   // csum position of the predecessor, relative
                m_key[m] = (t << 16) | pk;
                m_del[m] = !(t < T);                           // a deletion costs `pen`
                m_plb[m] = t < T ? t * TL * TL : 0;            // cost plane of the move (any plane for the others: value unused)
            }
            // Loop invariants of this thread's node column j, and the band offsets of the tile's 63 diagonals (a = 32 (I + J) + dd
            // for every node of diagonal dd) one per lane, fetched by v_readlane in the loop: the loop body is instruction-bound
            // (~180 instructions per diagonal with the offsets read from LDS behind a branch and short-circuit merges; ~120 so).
            const int yy = TL * J + j;
            const bool y_in = yy <= ys, y_pos = yy >= 1;
            const int xrel_max = xs - TL * I;                  // node rows of the tile that exist: ic <= xrel_max
            const int a0 = TL * (I + J);
            const int bo_mine = bo_l[a0 + (tid & 63) - abase]; // (lane 63: one past the tile's last diagonal, never selected; inside bo_l)
            const bool edge_tile = I == 0 || J == 0;           // only these tiles hold nodes of row 0 / column 0
            double cconst[MS];
            bool use_cv[MS];
#pragma unroll
            for (int m = 0; m < MS; m++) {
                use_cv[m] = m_ok[m] && !m_del[m];
                cconst[m] = m_ok[m] ? pen : inf;               // a move this slot does not have can never win
                if (!m_ok[m]) m_off[m] = 0;                    // (its csum read is any valid cell)
            }
            for (int dd = 0; dd <= 2 * (TL - 1); dd++) {
                const int i = dd - j;
                const bool inside = (unsigned)i < (unsigned)TL;
                const int ic = inside ? i : 0;
                const int cpos = (ic + TT_HALO) * CS_W + (j + TT_HALO), ppos = ic * TL + j;
                double pv[MS];
                float cv[MS];
#pragma unroll
                for (int m = 0; m < MS; m++) {
                    pv[m] = cs[cpos + m_off[m]];
                    cv[m] = planes[m_plb[m] + ppos];
                    asm volatile("" : "+v"(cv[m]));   // (every read issued here, none sunk into a branch behind its own wait)
                }
                const int bo = __builtin_amdgcn_readlane(bo_mine, dd);
                const int b = yy - bo;
                const bool node = inside & (ic <= xrel_max) & y_in & ((unsigned)b < (unsigned)B);
                const bool general = node & (TL * I + ic >= 1) & y_pos & (a0 + dd - 2 < A);
                // (the slot's first move starts the minimum; "no move reaches this node" is read off the total at the end)
                DpMerge best{pv[0] + (use_cv[0] ? (double)cv[0] : cconst[0]), m_key[0]};
#pragma unroll
                for (int m = 1; m < MS; m++) {
                    const double tot = pv[m] + (use_cv[m] ? (double)cv[m] : cconst[m]);
                    const bool take = tot < best.tot;
                    best.tot = take ? tot : best.tot;
                    best.key = take ? m_key[m] : best.key;
                }
                node_merge(best);   // over the node's eight lanes
                const bool won = general & (best.tot < inf);
                double v = won ? best.tot : inf;
                int bpv = won ? (((best.key & 255) << 4) | ((best.key >> 8) & 255)) : 0xFF;
                if (edge_tile) {   // workgroup-uniform
                    const int xx = TL * I + ic;
                    if (node && xx == 0) { v = pen * (double)yy; bpv = (0 << 4) | 1; }
                    else if (node && yy == 0) { v = pen * (double)xx; bpv = (1 << 4) | 0; }
                }
                if (inside && slot == 0) {
                    cs[cpos] = node ? v : inf;
                    bpt[ppos] = (unsigned char)(node ? bpv : 0xFF);
                }
                __syncthreads();   // the diagonal is complete before any wave reads it
            }
        }
        __syncthreads();
        stamp(4);
        // ---- phase 4: results into the node arrays; the neighbours read the last H rows and columns
        tile_publish<false>(cs, geo, band, Lv.csum, P.t_flag + tile_flag_at(P, s, I), I, J, stamp, [&](size_t o, int e) { Lv.bpk[o] = bpt[e]; });
    }
}

// ---- general shape: any type set make_types accepts (<= 128 types, sizes <= 100).
// The costs phase runs once per GROUP of <= 16 types on <= 12 overlap slots (the medium shape's register and ring budget)
// and writes the group's planes to this workgroup's own slice of global scratch, laid out [t / 8][x row][y row][t % 8]:
// the eight move slots of a DP node read 32 contiguous bytes.  The DP phase reads them back one node diagonal ahead.
// The csum tile is (32 + Hx) x (32 + Hy) with Hx / Hy the largest x / y step (up to 100, beyond the tile side).
// Back-pointers leave as packed bytes when the steps allow it, else as the int32 xp / yp arrays.
// LDS: the four ring stages are separate objects, so that the compiler's LDS-DMA tracking lets a ring read wait for its
// own slab only (one array holding all four makes it wait for every slab in flight: vmcnt(0) in front of each read).
// Beside the 96 KB ring, the csum tile takes up to TG_CSSMALL doubles: every halo with (32 + Hx)(32 + Hy) within it.
// Larger halos (both steps large, e.g. (100, 1) and (1, 100) in one set) take the BIGH variant, whose csum tile shares
// one array with the ring (idle by then) -- and whose ring is serialised by that wait.
constexpr int TG_MAXG = 32, TG_MAXH = 100;
constexpr int TG_NSLOT = 12, TG_UPW = 8, TG_S = 4;
constexpr int TG_CSMAX = (TL + TG_MAXH) * (TL + TG_MAXH) + 1;
constexpr int TG_CSSMALL = 7040;

struct TileGroup {
    unsigned char nslot, nt, pad_[2];
    unsigned char slot_info[TT_MAXSLOT];  // side << 7 | layer
    unsigned char type_id[TT_MAXT];       // index into the type set
    unsigned char type_slots[TT_MAXT];    // x slot | y slot << 4
};

struct TilePlanGen {
    int ng, hx, hy, nplane;  // groups, largest x / y step, type planes per workgroup slice (T rounded up to 8)
    TileGroup g[TG_MAXG];
};

template <typename E, int MS, bool BIGH>
__global__ __launch_bounds__(TT_THREADS) void k_band_tiles_gen(const SvxPairDev* __restrict__ pairs, int n_pairs, SvxTypes ty, TilePlanGen plan,
                                                               int W, int max_nd, const int* __restrict__ gpref, int* ticket, float* planes_all,
                                                               unsigned long long* prof) {
    using C = TileCfg<E, TG_NSLOT, TG_UPW, TG_S>;
    using St = typename E::storage;
    using R = typename C::Ring;
    constexpr int RING = TG_S * R::STAGE;
    constexpr int LDS_MAIN = (RING > TG_CSMAX * 8 ? RING : TG_CSMAX * 8);
    constexpr int STG = BIGH ? 16 : R::STAGE;
    __shared__ __attribute__((aligned(1024))) char st0[STG];
    __shared__ __attribute__((aligned(1024))) char st1[STG];
    __shared__ __attribute__((aligned(1024))) char st2[STG];
    __shared__ __attribute__((aligned(1024))) char st3[STG];
    __shared__ __attribute__((aligned(16))) double csl[BIGH ? 2 : TG_CSSMALL];
    __shared__ __attribute__((aligned(1024))) char lmain[BIGH ? LDS_MAIN : 16];  // BIGH: DMA ring, then the csum tile
    __shared__ unsigned short bpt[TL * TL];                         // x step | y step << 8, 0xFFFF = unreachable
    __shared__ float snrm[TG_NSLOT * TL], sinv[TG_NSLOT * TL];
    __shared__ int bo_l[2 * TL + 2 * TG_MAXH + 2];
    __shared__ int tpk[SVX_MAX_TYPES + 2];
    __shared__ int sh_ticket;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int B = 2 * W, T = ty.n, NTt = T + 2, HX = plan.hx, HY = plan.hy, CSY = TL + plan.hy;
    const int NCS = (TL + HX) * CSY;   // cs[NCS] = +inf
    double* cs = BIGH ? reinterpret_cast<double*>(lmain) : csl;
    float* pl = planes_all + (size_t)blockIdx.x * plan.nplane * TL * TL;
    const long long nent = (long long)max_nd * n_pairs;
    const int total = gpref[nent];
    for (int t = tid; t < NTt; t += TT_THREADS) tpk[t] = (int)ty.x[t] | ((int)ty.y[t] << 8);
    const double inf = __builtin_inf();
    long long ecur = 0;

    TileStamp stamp(prof);
    for (;;) {
        const TileAt at = tile_claim<false>(pairs, n_pairs, gpref, nent, total, ticket, &sh_ticket, ecur, stamp);
        if (at.p < 0) break;
        const int s = at.s, I = at.I, J = at.J;
        const SvxPairDev& P = pairs[at.p];
        const SvxLevel& Lv = P.lev[0];
        const int xs = Lv.n[0], ys = Lv.n[1], d = P.d;
        const int rowbytes = d * (int)sizeof(St);
        const int NK = (rowbytes + TT_SLAB - 1) / TT_SLAB;
        const int X0 = TL * I - 1, Y0 = TL * J - 1;
        const int A = *Lv.path_len;
        const double pen = *Lv.pen;

        stamp(0);
        // ---- phase 1: cost planes, one group of types at a time, into this workgroup's scratch slice
        // (individual stage pointers, never an array indexed by stage: svx_slab.h)
        char* const rs0 = BIGH ? lmain : st0;
        char* const rs1 = BIGH ? lmain + R::STAGE : st1;
        char* const rs2 = BIGH ? lmain + 2 * R::STAGE : st2;
        char* const rs3 = BIGH ? lmain + 3 * R::STAGE : st3;
        const SlabSide sx{P.v[0], Lv.nrm[0], Lv.inv[0], X0, TL, xs}, sy{P.v[1], Lv.nrm[1], Lv.inv[1], Y0, TL, ys};
        for (int gi_ = 0; gi_ < plan.ng; gi_++) {
            const TileGroup& G = plan.g[gi_];
            __syncthreads();  // the previous group is finished with the ring and the row norms
            auto slot_of = [&](int slot) { return slot < G.nslot ? SlabSlot{G.slot_info[slot] >> 7, G.slot_info[slot] & 127} : SlabSlot{-1, 0}; };
            auto type_slots = [&](int tl) { return SlabPair{G.type_slots[tl] & 15, G.type_slots[tl] >> 4}; };
            float r_nrm[R::SPT], r_inv[R::SPT];   // (stored at once: no registers to spare across this k loop)
            R::row_scalars(slot_of, sx, sy, tid, r_nrm, r_inv);
            R::store_scalars(snrm, sinv, tid, r_nrm, r_inv);
            typename R::Src src;
            R::sources(slot_of, sx, sy, rowbytes, wave, lane, src);
            f32x4_t acc[TG_UPW][2];
            typename R::template Units<TG_UPW> un;
            const int nunits = G.nt * 2;
            R::template units<TG_UPW, 2>(type_slots, nunits, nullptr, wave, lane, un, acc);
            R::template run<TG_UPW, 2>(NK, src, un, acc, rs0, rs1, rs2, rs3, nullptr);
            tile_cost_planes<TG_UPW, 8>(acc, nunits, wave, lane, snrm, sinv, [&](int tl) {
                const int t = G.type_id[tl];
                return TilePlane{tpk[t] & 255, tpk[t] >> 8, (G.type_slots[tl] & 15) * TL, (G.type_slots[tl] >> 4) * TL,
                                 pl + (size_t)(t >> 3) * (TL * TL * 8) + (t & 7)};
            });
        }
        const int abase = TL * s - HX - HY;
        tile_band_offsets(bo_l, Lv.boff_out, abase, 2 * TL + HX + HY, A);
        __syncthreads();  // (also: the planes are written, and the ring is free for the csum tile)
        stamp(1);
        // ---- phase 2: wait for every band tile that holds halo nodes: rows I - ceil(Hx / 32) .. I, columns
        // J - ceil(Hy / 32) .. J (all on earlier tile anti-diagonals: smaller tickets, running workgroups), then the halo into
        // the csum tile: position (i + Hx, j + Hy) <-> node (32 I + i, 32 J + j), i in [-Hx, 32), j in [-Hy, 32)
        const TileBand band{xs, ys, B, abase, bo_l};
        const TileGeo geo{HX, HY, CSY, HX, HY};
        tile_wait<false>(P, P.t_flag, I, J, (HX + TL - 1) / TL, (HY + TL - 1) / TL);
        stamp(2);
        tile_halo_fill<false, 4>(cs, NCS + 1, geo, band, Lv.csum, I, J);
        stamp(3);
        // ---- phase 3: the tile's 63 node anti-diagonals; thread = (node column j, move slot), MS moves per slot in
        // registers, merged by (total, move index) over the node's eight lanes as in k_band_tiles.  The costs of
        // diagonal dd + 1 are loaded while diagonal dd is relaxed.
        {
            const int j = tid >> 3, slot = tid & 7;
            int m_off[MS], m_key[MS], m_pl[MS];
            bool use_cv[MS];
            double cconst[MS];
#pragma unroll
            for (int m = 0; m < MS; m++) {
                const int t = slot + 8 * m;
                const bool ok = t < NTt;
                const int pk = ok ? tpk[t] : 0;
                m_off[m] = ok ? -((pk & 255) * CSY + (pk >> 8)) : 0;
                m_key[m] = (t << 16) | pk;
                use_cv[m] = t < T;
                cconst[m] = ok ? pen : inf;
                m_pl[m] = (t < T ? m : 0) * (TL * TL * 8) + slot;  // (moves without a plane read any plane of the slice)
            }
            const int yy = TL * J + j;
            const bool y_in = yy <= ys, y_pos = yy >= 1;
            const int xrel_max = xs - TL * I;
            const int a0 = TL * (I + J);
            const int bo_mine = bo_l[a0 + (tid & 63) - abase];
            const bool edge_tile = I == 0 || J == 0;
            float cv[MS];
            auto load_cv = [&](int dd, float* out) {
                const int i = dd - j;
                const int ic = (unsigned)i < (unsigned)TL ? i : 0;
                const float* base = pl + (ic * TL + j) * 8;
#pragma unroll
                for (int m = 0; m < MS; m++) out[m] = base[m_pl[m]];
            };
            load_cv(0, cv);
            for (int dd = 0; dd <= 2 * (TL - 1); dd++) {
                const int i = dd - j;
                const bool inside = (unsigned)i < (unsigned)TL;
                const int ic = inside ? i : 0;
                const int cpos = (ic + HX) * CSY + (j + HY), ppos = ic * TL + j;
                double pv[MS];
                float cn[MS];
                load_cv(dd < 2 * (TL - 1) ? dd + 1 : dd, cn);
#pragma unroll
                for (int m = 0; m < MS; m++) pv[m] = cs[cpos + m_off[m]];
                const int bo = __builtin_amdgcn_readlane(bo_mine, dd);
                const int b = yy - bo;
                const bool node = inside & (ic <= xrel_max) & y_in & ((unsigned)b < (unsigned)B);
                const bool general = node & (TL * I + ic >= 1) & y_pos & (a0 + dd - 2 < A);
                DpMerge best{pv[0] + (use_cv[0] ? (double)cv[0] : cconst[0]), m_key[0]};
#pragma unroll
                for (int m = 1; m < MS; m++) {
                    const double tot = pv[m] + (use_cv[m] ? (double)cv[m] : cconst[m]);
                    const bool take = tot < best.tot;
                    best.tot = take ? tot : best.tot;
                    best.key = take ? m_key[m] : best.key;
                }
                node_merge(best);
                const bool won = general & (best.tot < inf);
                double v = won ? best.tot : inf;
                int bpv = won ? (best.key & 0xFFFF) : 0xFFFF;
                if (edge_tile) {
                    const int xx = TL * I + ic;
                    if (node && xx == 0) { v = pen * (double)yy; bpv = 0 | (1 << 8); }
                    else if (node && yy == 0) { v = pen * (double)xx; bpv = 1 | (0 << 8); }
                }
                if (inside && slot == 0) {
                    cs[cpos] = node ? v : inf;
                    bpt[ppos] = (unsigned short)(node ? bpv : 0xFFFF);
                }
#pragma unroll
                for (int m = 0; m < MS; m++) cv[m] = cn[m];
                // the diagonal is complete before any wave reads it (LDS only: the next diagonal's cost loads stay in flight)
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
            }
        }
        __syncthreads();
        stamp(4);
        // ---- phase 4: results into the node arrays; later tiles read the last Hx rows and the last Hy columns (all of the
        // tile once a step reaches 32)
        tile_publish<false>(cs, geo, band, Lv.csum, P.t_flag + tile_flag_at(P, s, I), I, J, stamp, [&](size_t o, int e) {
            const int bv = bpt[e];
            if (Lv.bpk) {
                Lv.bpk[o] = bv == 0xFFFF ? (unsigned char)0xFF : (unsigned char)(((bv & 255) << 4) | (bv >> 8));
            } else {
                Lv.xp[o] = bv == 0xFFFF ? -42 : (bv & 255);
                Lv.yp[o] = bv == 0xFFFF ? -42 : (bv >> 8);
            }
        });
    }
}

// Groups of <= 16 types on <= 12 overlap slots for k_band_tiles_gen.  Types are taken in blocks of 4 x 4 sizes (then by
// size), and a group is closed when the next type would need a 17th type or a 13th slot: neighbouring sizes share their
// layers.  restream = slots streamed per tile over distinct slots.
bool make_tile_plan_gen(const SvxTypes& ty, TilePlanGen* plan, double* restream) {
    memset(plan, 0, sizeof(*plan));
    const int T = ty.n;
    if (T < 1 || T > SVX_MAX_TYPES) return false;
    int order[SVX_MAX_TYPES];
    for (int t = 0; t < T; t++) order[t] = t;
    auto key = [&](int t) {
        const int x = ty.x[t] - 1, y = ty.y[t] - 1;
        return (((x / 4) * 32 + y / 4) * 128 + x) * 128 + y;
    };
    for (int a = 1; a < T; a++)  // (insertion sort: stable, at most 128 entries)
        for (int b = a; b > 0 && key(order[b]) < key(order[b - 1]); b--) { const int tmp = order[b]; order[b] = order[b - 1]; order[b - 1] = tmp; }
    bool seen[2][128];
    memset(seen, 0, sizeof(seen));
    int distinct = 0, streamed = 0;
    TileGroup* G = nullptr;
    int gslot[2][128];
    for (int k = 0; k < T; k++) {
        const int t = order[k], lx = ty.x[t] - 1, ly = ty.y[t] - 1;
        if (lx >= 127 || ly >= 127) return false;
        if (G) {
            const int need = (gslot[0][lx] < 0) + (gslot[1][ly] < 0);
            if (G->nt >= TT_MAXT || G->nslot + need > TG_NSLOT) G = nullptr;
        }
        if (!G) {
            if (plan->ng >= TG_MAXG) return false;
            G = &plan->g[plan->ng++];
            for (int s2 = 0; s2 < 2; s2++) for (int l = 0; l < 128; l++) gslot[s2][l] = -1;
        }
        const int lay[2] = {lx, ly};
        for (int s2 = 0; s2 < 2; s2++) {
            if (gslot[s2][lay[s2]] < 0) {
                gslot[s2][lay[s2]] = G->nslot;
                G->slot_info[G->nslot++] = (unsigned char)((s2 << 7) | lay[s2]);
                streamed++;
            }
            if (!seen[s2][lay[s2]]) { seen[s2][lay[s2]] = true; distinct++; }
        }
        G->type_id[G->nt] = (unsigned char)t;
        G->type_slots[G->nt] = (unsigned char)(gslot[0][lx] | (gslot[1][ly] << 4));
        G->nt++;
        if (ty.x[t] > plan->hx) plan->hx = ty.x[t];
        if (ty.y[t] > plan->hy) plan->hy = ty.y[t];
    }
    if (plan->hx < 1) plan->hx = 1;  // (the deletions step by one)
    if (plan->hy < 1) plan->hy = 1;
    if (plan->hx > TG_MAXH || plan->hy > TG_MAXH) return false;
    plan->nplane = (T + 7) / 8 * 8;
    if (restream) *restream = distinct ? (double)streamed / distinct : 1.0;
    return true;
}

}  // namespace

// Which tile shape takes this type set: 0 = <= 10 types on <= 8 layers, 1 = <= 16 types on <= 12 layers (both with
// steps of at most 8 segments), 2 = the general shape (any set make_types accepts), -1 = none.
int svxl_band_tiles_shape(const SvxTypes& types) {
    TilePlan plan;
    if (make_tile_plan(types, 10, 8, &plan)) return 0;
    if (make_tile_plan(types, 16, 12, &plan)) return 1;
    TilePlanGen gp;
    return make_tile_plan_gen(types, &gp, nullptr) ? 2 : -1;
}

// Global scratch of the general shape: one slice of cost planes per persistent workgroup (T rounded up to 8 planes of
// 32 x 32 fp32).  0 for the two LDS-resident shapes.
size_t svxl_band_tiles_scratch(const SvxTypes& types) {
    TilePlanGen gp;
    if (svxl_band_tiles_shape(types) != 2 || !make_tile_plan_gen(types, &gp, nullptr)) return 0;
    return (size_t)tile_cu_count() * gp.nplane * TL * TL * sizeof(float);
}

// b_offset_out, tile ranges (which also clear the pairs' tile flags), ticket table, then the persistent tile sweep.
// gpref [max_nd * n_pairs + 1] and ticket live in the arena.
int svxl_band_tiles_batch(svx_ctx* ctx, const SvxPairDev* pairs, int n_pairs, const SvxTypes& types, int W, int dtype, int max_nd,
                          int* gpref, int* ticket, float* planes) {
    if (n_pairs <= 0) return SVX_OK;
    hipStream_t st = ctx->stream;
    const int shape = svxl_band_tiles_shape(types);
    if (shape < 0)
        return svx_fail(ctx, SVX_ERR_ARG, "wide band: %d alignment types: no tile shape takes this set", types.n);
    TilePlan plan;
    TilePlanGen gplan;
    double restream = 1.0;
    if (shape < 2) make_tile_plan(types, shape == 0 ? 10 : 16, shape == 0 ? 8 : 12, &plan);
    else make_tile_plan_gen(types, &gplan, &restream);
    const bool bigh = shape == 2 && (TL + gplan.hx) * (TL + gplan.hy) + 1 > TG_CSSMALL;  // csum tile beside the ring or not
    if (shape == 2 && !planes) return svx_fail(ctx, SVX_ERR_ARG, "wide band: the general tile shape needs its plane scratch");
    hipLaunchKernelGGL(k_tile_ranges, dim3(n_pairs), dim3(256), 0, st, pairs, W, 2 * W);
    hipLaunchKernelGGL(k_tile_prefix, dim3(1), dim3(1024), 0, st, pairs, n_pairs, max_nd, gpref, ticket);
    SVX_LAUNCH_CHECK(ctx, "k_tile_ranges");
    const int ncu = tile_cu_count();  // (the general shape's plane scratch is sized by the same count)
    // one persistent workgroup per CU (> 100 KB of LDS each): all of them are resident, so a workgroup that waits for
    // a neighbour's flag always waits for a running workgroup
    dim3 grid((unsigned)ncu);
    TileProf tp;
    if (const int rc = tp.begin(ctx, st, "wide band")) return rc;
    unsigned long long* prof = tp.dev;
    // general shape: moves per DP slot MS = ceil((T + 2) / 8), rounded up to an instantiated count
    const int ms_need = (types.n + 2 + 7) / 8;
    static const int ms_set[] = {2, 3, 4, 6, 9, 17};
    int ms = 17;
    for (int v : ms_set)
        if (v >= ms_need) { ms = v; break; }
#define GEN(E, M, BH) hipLaunchKernelGGL((k_band_tiles_gen<E, M, BH>), grid, dim3(TT_THREADS), 0, st, pairs, n_pairs, types, gplan, W, max_nd, gpref, ticket, planes, prof)
#define TILES(E)                                                                                                                   \
    do {                                                                                                                           \
        if (shape == 0) hipLaunchKernelGGL((k_band_tiles<E, 8, 5, 5>), grid, dim3(TT_THREADS), 0, st, pairs, n_pairs, types, plan, W, max_nd, gpref, ticket, prof); \
        else if (shape == 1) hipLaunchKernelGGL((k_band_tiles<E, 12, 8, 2>), grid, dim3(TT_THREADS), 0, st, pairs, n_pairs, types, plan, W, max_nd, gpref, ticket, prof); \
        else if (bigh) GEN(E, 17, true);   /* (rare: both steps large; one instantiation for every type count) */                 \
        else if (ms == 2) GEN(E, 2, false);                                                                                        \
        else if (ms == 3) GEN(E, 3, false);                                                                                        \
        else if (ms == 4) GEN(E, 4, false);                                                                                        \
        else if (ms == 6) GEN(E, 6, false);                                                                                        \
        else if (ms == 9) GEN(E, 9, false);                                                                                        \
        else GEN(E, 17, false);                                                                                                    \
    } while (0)
    SVX_TILE_BY_DTYPE(dtype, TILES);
#undef TILES
#undef GEN
    const hipError_t le = hipGetLastError(), re = tp.end(st, le);
    if (le != hipSuccess) return svx_fail(ctx, SVX_ERR_HIP, "launch %s: %s", "k_band_tiles", hipGetErrorString(le));
    if (re != hipSuccess) return svx_fail(ctx, SVX_ERR_HIP, "wide band: tile profile read-back: %s", hipGetErrorString(re));
    if (prof) {
        static const char* const nm[7] = {"ticket+lookup", "costs", "wait", "clear+halo", "dp", "edge-store+flag", "interior-store+loop"};
        tp.print("svx tile sweep", grid.x, nm);
        if (shape == 2) {
            int streamed = 0;
            for (int g = 0; g < gplan.ng; g++) streamed += gplan.g[g].nslot;
            fprintf(stderr, " | general shape: %d types in %d groups, %d slot-rows streamed per tile, re-stream x%.2f, halo %d x %d%s",
                    types.n, gplan.ng, streamed, restream, gplan.hx, gplan.hy, bigh ? " (csum tile shares the ring's LDS)" : "");
        }
        fprintf(stderr, "\n");
    }
    return SVX_OK;
}
