// svx_tiles_bwd.hip -- row slack in wide bands: the tile sweep of svx_tiles.hip turned round, with the cut minimum of the
// slack definition folded into it (include/svx.h: svx_row_slack_wide; gfx950 only).
//
// The definition is svx_row_slack's (include/svx.h, "row slack"): slack[r] = min over the edges e != e* that cross the cut
// behind the row's start diagonal c of ((F(u) + w) + Bk(v)), minus F(end).  svx_slack.hip evaluates it from a stored
// [A][T][B] cost array, one row at a time.  A wide band keeps no cost array, and the scan would price maxstep * B * (T + 2)
// edges per row from 1024-wide dot products nobody kept.  Here the computation is turned round: a backward tile sweep holds,
// for every edge it relaxes, w (the tile's own cost plane, the fp32 value the forward sweep used), Bk(v) (just computed)
// and F(u) (the forward csum, complete by now) in LDS at the same moment.  An edge u -> v crosses the cuts
// a(u) <= c < a(v) and the returned path crosses every cut exactly once, so
//     cutmin[c] = min over the edges crossing cut c, the returned path's own edge left out, of ((F(u) + w) + Bk(v))
//     slack[r]  = cutmin[x_start + y_start] - F(end)
// and cutmin is a per-diagonal minimum that the sweep folds while it runs.  A minimum does not depend on the order it is
// taken in and every candidate is the same two float64 additions as in svx_slack.hip: on equal cost bits the result is
// svx_row_slack's bits (tests/slack_wide_ref.py restates the scheme in numpy).
//
//   k_bwd_table       per pair: the returned path's node on each diagonal, (y, x_len | y_len << 8), from the level-0 rows
//   k_band_tiles_bwd  persistent workgroups, one per CU, tickets in REVERSE order of the forward sweep (reverse ticket k is
//                     forward ticket total - 1 - k).  A tile owns the edges LEAVING its 32 x 32 nodes; it needs Bk of the
//                     tiles (I+1, J), (I, J+1), (I+1, J+1), whose forward tickets are larger, hence whose reverse tickets
//                     are smaller: claimed by running workgroups, no deadlock under any dispatch order (the argument of
//                     svx_tiles.hip with the order turned round).  Costs phase: the SlabRing of svx_slab.h with the slot of
//                     layer k shifted by k rows, so that plane t at [xloc][yloc] is the weight of the move out of that node.
//                     DP phase: thread = (node column, move slot), diagonals 62 .. 0, Bk in the csum tile with the halo
//                     BELOW and to the RIGHT, merged over a node's eight lanes by a plain minimum (Bk has no back-pointer).
//                     Cut fold: every thread keeps 16 running minima for the cuts c .. c + 15 (a candidate of step st from
//                     diagonal a feeds cuts a .. a + st - 1, st <= 16); the cut that no later diagonal of the tile can feed
//                     is reduced over the wave and parked in LDS, and at the end of the tile one 64-bit atomic minimum per
//                     (tile, cut) on a monotone integer image of the double goes to cutmin.
//   k_slack_wide      per pair: slack[r] = cutmin[c] - total for the rows that are edges, NaN otherwise; the summary.
// The tile plan (t_lo, t_cnt, t_pref, the ticket table) is the forward call's, still in its arena; flags are an array of
// this call's own.  Claim, wait, halo fill and publish are the scaffold of svx_tile_plan.h with BWD = true; this file holds
// the cost phase, the F and path fill, the node-diagonal loop with the cut fold, and the cut minima.  Plain C++ and vector
// stores only.
#include <stdio.h>
#include <stdlib.h>

#include "svx_plane.h"
#include "svx_tile_plan.h"

namespace {

__device__ __forceinline__ unsigned long long cut_image(double v) {   // order-preserving: a < b <=> image(a) < image(b)
    const long long b = __double_as_longlong(v);
    return b < 0 ? ~(unsigned long long)b : ((unsigned long long)b | 0x8000000000000000ull);
}
__device__ __forceinline__ double cut_value(unsigned long long k) {   // all ones (the initial value): no candidate
    if (k == ~0ull) return __builtin_inf();
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

__device__ __forceinline__ double min_f64(double a, double b) { return b < a ? b : a; }
// minimum over a node's eight lanes (every lane ends with it)
__device__ __forceinline__ double node_min(double v) {
    v = min_f64(v, dpp_f64<DPP_QUAD_1032>(v));
    v = min_f64(v, dpp_f64<DPP_QUAD_2301>(v));
    v = min_f64(v, dpp_f64<DPP_HALF_MIRROR>(v));
    return v;
}
// minimum over the wave (every lane ends with it): the exchanges of wave_max (svx_common.h) on the two halves of a double
__device__ __forceinline__ double wave_min_f64(double v, int lane) {
    v = node_min(v);
    v = min_f64(v, dpp_f64<DPP_ROW_MIRROR>(v));
    {
        const unsigned long long u = __double_as_longlong(v);
        const unsigned lo = xchg16_u32((unsigned)u, lane), hi = xchg16_u32((unsigned)(u >> 32), lane);
        v = min_f64(v, __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo)));
    }
    {
        const unsigned long long u = __double_as_longlong(v);
        const unsigned lo = xchg32_u32((unsigned)u, lane), hi = xchg32_u32((unsigned)(u >> 32), lane);
        v = min_f64(v, __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo)));
    }
    return v;
}

constexpr int CUT_RING = 16;            // cuts a candidate can feed: steps are at most 2 * TT_HALO
constexpr int CUT_SPAN = 2 * TL + CUT_RING;   // cuts a tile can feed: its 63 diagonals + 15, rounded up
static_assert(2 * TT_HALO <= CUT_RING, "a step feeds at most CUT_RING cuts");

// The returned path's node on every diagonal: tab[2 a] = y of the node, tab[2 a + 1] = x_len | y_len << 8 of the row that
// starts there; -1 (the table's initial fill) on a diagonal no row starts on.  Rows that cannot be edges are left out.
__global__ __launch_bounds__(256) void k_bwd_table(const SvxPairDev* __restrict__ pairs, const BwdPair* __restrict__ bw) {
    const SvxPairDev& P = pairs[blockIdx.x];
    const BwdPair Q = bw[blockIdx.x];
    const SvxLevel& Lv = P.lev[0];
    if (!Q.slack || gld(P.status) != 0) return;
    const int A = gld(Lv.path_len), cap = Lv.n[0] + Lv.n[1] + 2;
    const int cnt = gld(Lv.n_align);
    if (A <= 0 || cnt < 0 || cnt > cap) return;
    for (int r = threadIdx.x; r < cnt; r += 256) {
        const uint4 rv = gld16(Lv.align + 4 * (size_t)r);
        const long long x0 = (int)rv.x, xl = (int)rv.y, y0 = (int)rv.z, yl = (int)rv.w;
        if (x0 < 0 || y0 < 0 || xl < 0 || yl < 0 || xl > 127 || yl > 127 || xl + yl < 1 || x0 + y0 >= (long long)A + 2) continue;
        const size_t c = (size_t)(x0 + y0);
        gst(Q.tab + 2 * c, (int)y0);
        gst(Q.tab + 2 * c + 1, (int)(xl | (yl << 8)));
    }
}

template <typename E, int NSLOT, int UPW, int S>
__global__ __launch_bounds__(TT_THREADS) void k_band_tiles_bwd(const SvxPairDev* __restrict__ pairs, const BwdPair* __restrict__ bw,
                                                               int n_pairs, SvxTypes ty, TilePlan plan, int W, int max_nd,
                                                               const int* __restrict__ gpref, int* ticket, unsigned long long* prof) {
    using C = TileCfg<E, NSLOT, UPW, S>;
    using St = typename E::storage;
    using R = typename C::Ring;
    __shared__ __attribute__((aligned(1024))) char st0[R::STAGE];
    __shared__ __attribute__((aligned(1024))) char st1[R::STAGE];
    __shared__ __attribute__((aligned(1024))) char st2[S >= 3 ? R::STAGE : 16];
    __shared__ __attribute__((aligned(1024))) char st3[S >= 4 ? R::STAGE : 16];
    __shared__ __attribute__((aligned(1024))) char st4[S >= 5 ? R::STAGE : 16];
    __shared__ __attribute__((aligned(16))) float planes[C::TPP * TL * TL];   // [type][x row][y row]: the move OUT of the node
    __shared__ __attribute__((aligned(16))) double cs[CS_W * CS_W + 2];       // Bk of the tile's nodes and halo; [CS_W^2] = +inf
    __shared__ __attribute__((aligned(16))) double fs[TL * TL];               // F of the tile's nodes, +inf for a non-node
    __shared__ __attribute__((aligned(16))) double cmw[TT_WAVES][CUT_SPAN];   // per wave: the retired cut minima of the tile
    __shared__ float snrm[NSLOT * TL], sinv[NSLOT * TL];
    __shared__ int bo_l[2 * TL + 2 * TT_HALO + 2];
    __shared__ int pth[2 * 64];                                               // the path's node of the tile's diagonals
    __shared__ int tpk[TT_MAXT + 2];
    __shared__ int sh_ticket;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int B = 2 * W, T = ty.n, NTt = T + 2, H = plan.halo, maxstep = ty.maxstep;
    const long long nent = (long long)max_nd * n_pairs;
    const int total = gpref[nent];
    for (int t = tid; t < NTt; t += TT_THREADS) tpk[t] = (int)ty.x[t] | ((int)ty.y[t] << 8);
    const double inf = __builtin_inf();
    long long ecur = nent - 1;

    TileStamp stamp(prof);
    for (;;) {
        const TileAt at = tile_claim<true>(pairs, n_pairs, gpref, nent, total, ticket, &sh_ticket, ecur, stamp);
        if (at.p < 0) break;
        const int s = at.s, I = at.I, J = at.J;
        const SvxPairDev& P = pairs[at.p];
        const BwdPair Q = bw[at.p];
        if (!Q.slack) continue;   // (uniform) a skipped pair: none of its tiles waits for another
        const SvxLevel& Lv = P.lev[0];
        const int xs = Lv.n[0], ys = Lv.n[1], d = P.d;
        const int rowbytes = d * (int)sizeof(St);
        const int NK = (rowbytes + TT_SLAB - 1) / TT_SLAB;
        const int A = *Lv.path_len;
        const double pen = *Lv.pen;

        stamp(0);
        // ---- phase 1: cost planes of the moves out of the tile's nodes.  Edge u -> u + (p, q) is priced from rows
        // x_u + p - 1 of layer p - 1 and y_u + q - 1 of layer q - 1: the slot of layer k stages rows 32 I + k ... (svx_slab.h)
        const SlabSide sx{P.v[0], Lv.nrm[0], Lv.inv[0], TL * I, TL, xs}, sy{P.v[1], Lv.nrm[1], Lv.inv[1], TL * J, TL, ys};
        auto slot_of = [&](int slot) {
            return slot < plan.nslot ? SlabSlot{plan.slot_info[slot] >> 8, plan.slot_info[slot] & 255, plan.slot_info[slot] & 255}
                                     : SlabSlot{-1, 0, 0};
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
        // band offsets of the node diagonals this tile and its halo touch: a in [32 s, 32 s + 62 + 2 H]
        const int abase = TL * s;
        tile_band_offsets(bo_l, Lv.boff_out, abase, 2 * TL + 2 * H, A);
        __syncthreads();
        tile_cost_planes<UPW, 1>(acc, nunits, wave, lane, snrm, sinv, [&](int tl) {
            return TilePlane{tpk[tl] & 255, tpk[tl] >> 8, (plan.type_slots[tl] & 255) * TL, (plan.type_slots[tl] >> 8) * TL, planes + tl * TL * TL};
        });
        stamp(1);
        // ---- phase 2: wait for the neighbours below and to the right (all three, when they exist, have smaller reverse
        // tickets), then their halo into the Bk tile: position (i, j) <-> node (32 I + i, 32 J + j), i, j in [0, 32 + H)
        // (the hand-off: svx_tile_plan.h)
        const TileBand band{xs, ys, B, abase, bo_l};
        const TileGeo geo{H, H, CS_W, 0, 0};
        tile_wait<true>(P, Q.flag, I, J, 1, 1);
        stamp(2);
        // F of the tile's own nodes (plain loads: the forward sweep is complete), the path's node of its diagonals
        // (in front of the halo fill, whose barriers cover these writes too)
        for (int e = tid; e < TL * TL; e += TT_THREADS) {
            size_t o;
            fs[e] = band.cell(TL * I + e / TL, TL * J + e % TL, &o) ? gld(Lv.csum + o) : inf;
        }
        if (tid < 64) {
            const int a = abase + tid;
            const bool has = tid < 2 * TL - 1 && a < A + 2;
            pth[2 * tid] = has ? gld(Q.tab + 2 * (size_t)a) : -1;
            pth[2 * tid + 1] = has ? gld(Q.tab + 2 * (size_t)a + 1) : -1;
        }
        tile_halo_fill<true, 3>(cs, CS_W * CS_W + 2, geo, band, Q.bsum, I, J);
        stamp(3);
        // ---- phase 3: the tile's 63 node anti-diagonals from the last to the first, all four waves: thread = (node j = tid >> 3,
        // move slot = tid & 7); a slot relaxes the moves t = slot, slot + 8, ... OUT of its node.  Successors outside the
        // lattice or the band, and the moves a slot does not have, read +inf.  The loop is unrolled 16 times so that the ring
        // of cut minima is indexed by constants (it stays in registers).
        {
            constexpr int MS = (C::TPP + 2 + 7) / 8;
            const int j = tid >> 3, slot = tid & 7;
            int m_off[MS], m_pk[MS], m_plb[MS], m_st[MS];
            bool use_cv[MS];
            double cconst[MS];
#pragma unroll
            for (int m = 0; m < MS; m++) {
                const int t = slot + 8 * m;
                const bool ok = t < NTt;
                const int pk = ok ? tpk[t] : 0;
                m_off[m] = (pk & 255) * CS_W + (pk >> 8);      // Bk position of the successor, relative (0: any valid cell)
                m_pk[m] = ok ? pk : 0x7fffffff;                 // (never the move of a row)
                m_st[m] = (pk & 255) + (pk >> 8);               // cuts the move crosses; 0 for a move the slot does not have
                use_cv[m] = t < T;
                cconst[m] = ok ? pen : inf;                     // a deletion costs `pen`; a missing move never wins
                m_plb[m] = t < T ? t * TL * TL : 0;
            }
            // the slot's moves by falling step (a minimum does not mind the order): the moves that cross a given cut are then a
            // prefix of them, and the cut fold below selects one prefix minimum per cut instead of every move
#pragma unroll
            for (int a2 = 0; a2 < MS - 1; a2++) {
#pragma unroll
                for (int b2 = 0; b2 < MS - 1 - a2; b2++) {
                    if (m_st[b2] < m_st[b2 + 1]) {
                        const int o_ = m_off[b2], k_ = m_pk[b2], s_ = m_st[b2], l_ = m_plb[b2];
                        const bool u_ = use_cv[b2];
                        const double c_ = cconst[b2];
                        m_off[b2] = m_off[b2 + 1]; m_pk[b2] = m_pk[b2 + 1]; m_st[b2] = m_st[b2 + 1]; m_plb[b2] = m_plb[b2 + 1];
                        use_cv[b2] = use_cv[b2 + 1]; cconst[b2] = cconst[b2 + 1];
                        m_off[b2 + 1] = o_; m_pk[b2 + 1] = k_; m_st[b2 + 1] = s_; m_plb[b2 + 1] = l_;
                        use_cv[b2 + 1] = u_; cconst[b2 + 1] = c_;
                    }
                }
            }
            const int yy = TL * J + j;
            const bool y_in = yy <= ys;
            const int xrel_max = xs - TL * I;
            const int bo_mine = bo_l[lane];                     // abase is the tile's first diagonal
            const int py_mine = pth[2 * lane], pm_mine = pth[2 * lane + 1];
            const bool end_tile = (xs / TL == I) && (ys / TL == J);
            double rg[CUT_RING];
#pragma unroll
            for (int e = 0; e < CUT_RING; e++) rg[e] = inf;
            for (int dq = 2 * TL / CUT_RING - 1; dq >= 0; dq--) {
#pragma unroll
                for (int k = CUT_RING - 1; k >= 0; k--) {
                    const int dd = dq * CUT_RING + k;           // (dd = 63 holds no node: it only keeps the unrolling even)
                    const int i = dd - j;
                    const bool inside = (unsigned)i < (unsigned)TL;
                    const int ic = inside ? i : 0;
                    const int cpos = ic * CS_W + j, ppos = ic * TL + j;
                    double pv[MS];
                    float cv[MS];
#pragma unroll
                    for (int m = 0; m < MS; m++) {
                        pv[m] = cs[cpos + m_off[m]];
                        cv[m] = planes[m_plb[m] + ppos];
                        asm volatile("" : "+v"(cv[m]));
                    }
                    const double fu_raw = fs[ppos];
                    const double fu = inside ? fu_raw : inf;    // F(u); +inf for a non-node: its candidates vanish
                    const int bo = __builtin_amdgcn_readlane(bo_mine, dd);
                    const int py = __builtin_amdgcn_readlane(py_mine, dd), pm = __builtin_amdgcn_readlane(pm_mine, dd);
                    const int b = yy - bo;
                    const bool node = inside & (ic <= xrel_max) & y_in & ((unsigned)b < (unsigned)B);
                    const bool on_path = yy == py;              // (u is the path's node of its diagonal)
                    double best = inf, cand[MS];
#pragma unroll
                    for (int m = 0; m < MS; m++) {
                        const double w = use_cv[m] ? (double)cv[m] : cconst[m];
                        const double tot = w + pv[m];
                        best = tot < best ? tot : best;
                        const double c2 = (fu + w) + pv[m];
                        cand[m] = (on_path & (m_pk[m] == pm)) ? inf : c2;   // the returned row's own edge (and duplicates of its move)
                    }
                    best = node_min(best);
                    double v = node ? best : inf;
                    if (end_tile && node && TL * I + ic == xs && yy == ys) v = 0.0;   // the end node
                    if (inside && slot == 0) cs[cpos] = v;
                    // a candidate of step st from this diagonal feeds the cuts dd .. dd + st - 1: cut dd + e gets the minimum of
                    // the moves with st > e, a prefix of the slot's moves
#pragma unroll
                    for (int m = 1; m < MS; m++) cand[m] = cand[m] < cand[m - 1] ? cand[m] : cand[m - 1];
#pragma unroll
                    for (int e = 0; e < CUT_RING; e++) {
                        if (e < maxstep) {   // (uniform)
                            double c2 = inf;
#pragma unroll
                            for (int m = 0; m < MS; m++) c2 = e < m_st[m] ? cand[m] : c2;
                            const double x = rg[(k + e) & (CUT_RING - 1)];
                            rg[(k + e) & (CUT_RING - 1)] = c2 < x ? c2 : x;
                        }
                    }
                    // cut dd + 15 is fed by no earlier diagonal of the tile: retire it
                    {
                        const double r = wave_min_f64(rg[(k + CUT_RING - 1) & (CUT_RING - 1)], lane);
                        rg[(k + CUT_RING - 1) & (CUT_RING - 1)] = inf;
                        if (lane == 0) cmw[wave][dd + CUT_RING - 1] = r;
                    }
                    __syncthreads();   // the diagonal is complete before any wave reads it
                }
            }
            // the cuts 0 .. 14 of the tile are still in the ring (dd = 0 left cut e in slot e)
#pragma unroll
            for (int e = 0; e < CUT_RING - 1; e++) {
                const double r = wave_min_f64(rg[e], lane);
                if (lane == 0) cmw[wave][e] = r;
            }
        }
        __syncthreads();
        stamp(4);
        // the tile's cut minima: one atomic minimum per cut that got a candidate
        if (tid < 2 * TL - 1 + CUT_RING - 1) {
            double m = cmw[0][tid];
#pragma unroll
            for (int w2 = 1; w2 < TT_WAVES; w2++) m = min_f64(m, cmw[w2][tid]);
            const int c = abase + tid;
            if (m < inf && c < A + 2)
                __hip_atomic_fetch_min(Q.cutmin + c, cut_image(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // ---- phase 4: Bk into the plane; the neighbours read the first H rows and columns
        tile_publish<true>(cs, geo, band, Q.bsum, Q.flag + tile_flag_at(P, s, I), I, J, stamp, [](size_t, int) {});
    }
}

// slack[r] = cutmin[start diagonal of row r] - total for the rows that are edges of the search space (plane_is_edge: the
// test of k_path_slack), NaN otherwise; the summary of svx_row_slack.
__global__ __launch_bounds__(256) void k_slack_wide(const SvxPairDev* __restrict__ pairs, const BwdPair* __restrict__ bw, SvxTypes ty, int B) {
    __shared__ int scnt[2];
    const SvxPairDev& P = pairs[blockIdx.x];
    const BwdPair Q = bw[blockIdx.x];
    if (!Q.slack) return;   // (uniform) a skipped pair: nothing of it is written
    const SvxLevel& Lv = P.lev[0];
    PlanePair pp{};
    pp.boff_in = Lv.boff; pp.path_len = Lv.path_len; pp.pen_dev = Lv.pen; pp.status = P.status; pp.csum = Lv.csum;
    pp.n_rows = Lv.n_align; pp.summary = Q.summary;
    pp.xs = Lv.n[0]; pp.ys = Lv.n[1]; pp.cap = Lv.n[0] + Lv.n[1] + 2;
    PlaneGeo g;
    const bool ok_pair = plane_geo(pp, ty, B, 1, &g);
    int cnt;
    if (!plane_row_count(pp, ok_pair, &cnt)) return;   // (uniform) a failed pair
    const int tid = threadIdx.x;
    if (tid < 2) scnt[tid] = 0;
    __syncthreads();
    const double inf = __builtin_inf();
    const double total = plane_total(g);
    int n_zero = 0, n_inf = 0;
    for (int r = tid; r < cnt; r += 256) {
        const uint4 rv = gld16(Lv.align + 4 * (size_t)r);
        int t_own, bui, bvi;
        double sl = __builtin_nan("");
        if (plane_is_edge(g, ty, rv, &t_own, &bui, &bvi)) sl = cut_value(gld(Q.cutmin + ((int)rv.x + (int)rv.z))) - total;
        gst(Q.slack + r, sl);
        n_zero += sl == 0.0 ? 1 : 0;
        n_inf += sl == inf ? 1 : 0;
    }
    if (n_zero) atomicAdd(&scnt[0], n_zero);
    if (n_inf) atomicAdd(&scnt[1], n_inf);
    __syncthreads();
    if (tid == 0) gst16(Q.summary, (uint32_t)cnt, (uint32_t)scnt[0], (uint32_t)scnt[1], 0u);
}

}  // namespace

// The node table, the reverse sweep, the slack kernel.  gpref is the forward call's ticket table; `ticket` is this call's
// own counter (zero).  The descriptors' cutmin and tab are filled with ones, their flags with zeros, by the caller.
int svxl_band_tiles_bwd(svx_ctx* ctx, const SvxPairDev* pairs, const BwdPair* bw, int n_pairs, const SvxTypes& types, int W, int dtype,
                        int max_nd, const int* gpref, int* ticket) {
    hipStream_t st = ctx->stream;
    const int shape = svxl_band_tiles_shape(types);
    TilePlan plan;
    if (shape < 0 || shape > 1 || !make_tile_plan(types, shape == 0 ? 10 : 16, shape == 0 ? 8 : 12, &plan))
        return svx_fail(ctx, SVX_ERR_ARG, "svx_row_slack_wide: %d alignment types take the general tile shape, which has no backward sweep", types.n);
    hipLaunchKernelGGL(k_bwd_table, dim3(n_pairs), dim3(256), 0, st, pairs, bw);
    SVX_LAUNCH_CHECK(ctx, "k_bwd_table");
    dim3 grid((unsigned)tile_cu_count());   // one persistent workgroup per CU, all resident (> 100 KB of LDS each)
    TileProf tp;
    if (const int rc = tp.begin(ctx, st, "svx_row_slack_wide")) return rc;
    unsigned long long* prof = tp.dev;
#define TILES(E)                                                                                                                   \
    do {                                                                                                                           \
        if (shape == 0) hipLaunchKernelGGL((k_band_tiles_bwd<E, 8, 5, 5>), grid, dim3(TT_THREADS), 0, st, pairs, bw, n_pairs, types, plan, W, max_nd, gpref, ticket, prof); \
        else hipLaunchKernelGGL((k_band_tiles_bwd<E, 12, 8, 2>), grid, dim3(TT_THREADS), 0, st, pairs, bw, n_pairs, types, plan, W, max_nd, gpref, ticket, prof); \
    } while (0)
    SVX_TILE_BY_DTYPE(dtype, TILES);
#undef TILES
    hipError_t le = hipGetLastError();
    if (le == hipSuccess) {
        hipLaunchKernelGGL(k_slack_wide, dim3(n_pairs), dim3(256), 0, st, pairs, bw, types, 2 * W);
        le = hipGetLastError();
    }
    le = tp.end(st, le);
    if (le != hipSuccess) return svx_fail(ctx, SVX_ERR_HIP, "svx_row_slack_wide: backward tile sweep: %s", hipGetErrorString(le));
    if (prof) {
        static const char* const nm[7] = {"ticket+lookup", "costs", "wait", "F+halo", "dp+cuts", "cutmin+store+flag", "interior-store+loop"};
        tp.print("svx backward tile sweep", grid.x, nm);
        fprintf(stderr, "\n");
    }
    return SVX_OK;
}
