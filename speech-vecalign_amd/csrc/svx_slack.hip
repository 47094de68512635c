// svx_slack.hip -- row slack: the backward band DP and, per returned row, the best path of the same search space that
// avoids the row (include/svx.h: svx_sparse_dp_backward, svx_path_slack, svx_row_slack; gfx950 only).
//
// The search space is what the forward band DP of svx_dp.hip relaxes: an edge u -> v by move (xo, yo) exists when u and v
// are lattice nodes (0 <= x <= xs, 0 <= y <= ys) that are band cells of their diagonals.  (Spelled out per node kind in
// include/svx.h; the kinds collapse to this because a type move ends at x, y >= 1 and a deletion into a border node can
// only come from along that border.)  Bk(u) is the cheapest way from u to the end node, Bk = min(w + Bk(v)).
//
//   k_bk_fast      B <= 64, one workgroup of four waves per pair, the forward fast kernel turned round.  Diagonals run
//                  from A+1 down to 0.  Waves 1-3 turn the next chunk of CH diagonals into three LDS tables -- the cost
//                  of every (diagonal, type, cell), the ring slot of its successor (or the slot that holds +inf) and one
//                  word per node with its kind and the lanes of its two deletion successors -- and write the chunk
//                  before to memory; wave 0 carries the chain: lanes are cells, diagonal a+1 stays in a register and
//                  its two neighbours come through a lane shuffle, the type moves (which reach at least two diagonals
//                  ahead) of diagonal a-1 are gathered from the ring of maxstep+1 diagonals before diagonal a is closed.
//                  Wave 0 does no index arithmetic and waits on no global load.
//   k_bk_wide      any B: cells strided over the workgroup, per-(diagonal, move) shifts and ring slots tabulated 32
//                  diagonals at a time, costs from global memory; RING keeps maxstep+1 diagonals of Bk in LDS, otherwise
//                  they are re-read from the output plane (the workgroup's own stores), as k_sparse_dp<RING> does.
//   k_path_slack   one workgroup per pair over a stored Bk plane; a wave takes a row at a time: the cut scan of svx_plane.h
//                  (cut_scan<false>: the minimum of (F(u) + w) + Bk(v) over the edges that cross the cut behind the row's
//                  start diagonal, the row's own left out), then slack = alt - total.  A row that fails the range checks
//                  forms no address.  The counts of the summary are reduced through LDS.
// The descriptor of a pair (PlanePair), its geometry and the helpers that read a plane are svx_plane.h's, shared with
// svx_alt.hip.  svx_row_slack lays out the post-processing scratch as [descriptors] uploaded, then one Bk plane per pair that
// is not skipped.  Both cost layouts are read: [T][A][B] (per-op) and [A][T][B] (fused pipeline).  Plain C++, vector stores only.
#include "svx_plane.h"

namespace {

// ------------------------------------------------------------------------------ backward sweep, any band width
constexpr int BKW_CH = 32;
__host__ __device__ inline size_t bkw_tab_bytes(int NTt) { return (size_t)BKW_CH * (2 * NTt + 1) * sizeof(int) + (size_t)NTt * sizeof(int); }

template <bool RING>
__device__ void bk_block(const PlaneGeo& g, const SvxTypes& ty, double* ring, int* tab) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int B = g.B, Aout = g.A + 2;
    const int T = ty.n, NTt = ty.n + 2;
    const int RD = ty.maxstep + 1;
    int* tpk = tab;                      // [NTt] xo | yo << 8 | step << 16
    int* shs = tab + NTt;                // [BKW_CH][NTt] cell shift of move t from diagonal a0 + i
    int* sls = shs + BKW_CH * NTt;       // [BKW_CH][NTt] ring slot (RING) of diagonal a + step
    int* bos = sls + BKW_CH * NTt;       // [BKW_CH] b_offset_out
    for (int t = tid; t < NTt; t += nt) tpk[t] = (int)ty.x[t] | ((int)ty.y[t] << 8) | (((int)ty.x[t] + (int)ty.y[t]) << 16);
    __syncthreads();
    const double inf = __builtin_inf();
    for (int a0 = ((Aout - 1) / BKW_CH) * BKW_CH; a0 >= 0; a0 -= BKW_CH) {
        for (int e = tid; e < BKW_CH * NTt; e += nt) {
            const int i = e / NTt, t = e - i * NTt;
            const int a = a0 + i, st = tpk[t] >> 16, yo = (tpk[t] >> 8) & 255;
            const int av = a + st;
            int v = 1 << 24, sl = 0;  // no successor diagonal: the shift pushes the cell out of the band
            if (av < Aout) {
                v = plane_bout(g.boff_in, a) + yo - plane_bout(g.boff_in, av);
                sl = av % RD;
            }
            shs[e] = v;
            sls[e] = sl;
        }
        for (int i = tid; i < BKW_CH; i += nt) bos[i] = a0 + i < Aout ? plane_bout(g.boff_in, a0 + i) : 0;
        __syncthreads();
        const int a_end = a0 + BKW_CH < Aout ? a0 + BKW_CH : Aout;
        for (int a = a_end - 1; a >= a0; a--) {
            const int i = a - a0;
            const int bo = bos[i];
            const int* sh = shs + i * NTt;
            const int* sl = sls + i * NTt;
            for (int b = tid; b < B; b += nt) {
                const int yy = b + bo;
                const int xx = a - yy;
                const bool lattice = 0 <= xx && xx <= g.xs && 0 <= yy && yy <= g.ys;
                double best = inf;
#pragma unroll 6
                for (int t = 0; t < NTt; t++) {
                    const int pk = tpk[t];
                    const int xo = pk & 255, yo = (pk >> 8) & 255, st = pk >> 16;
                    const int bv = b + sh[t];
                    const bool ok = lattice && xx + xo <= g.xs && yy + yo <= g.ys && 0 <= bv && bv < B;
                    const size_t ci = (ok && t < T) ? plane_cost_index(g, t, a + st - 2, bv) : 0;
                    const double w = t < T ? (double)g.costs[ci] : g.pen;
                    const double nxt = RING ? ring[ok ? sl[t] * B + bv : 0] : g.bsum[ok ? (size_t)(a + st) * B + bv : 0];
                    const double tot = w + nxt;
                    if (ok && tot < best) best = tot;
                }
                if (xx == g.xs && yy == g.ys) best = 0.0;   // the end node
                if (RING) ring[(size_t)(a % RD) * B + b] = best;
                g.bsum[(size_t)a * B + b] = best;
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------ backward sweep, B <= 64
constexpr int BKF_THREADS = 256;   // wave 0 sweeps, the others stage the next chunk's tables and write the last one's results

__host__ __device__ inline size_t bkf_align16(size_t v) { return (v + 15) & ~(size_t)15; }
__host__ __device__ inline size_t bkf_chunk_bytes(int T, int B, int CH) {
    const size_t cells = (size_t)CH * (T > 0 ? T : 1) * B;
    return bkf_align16(cells * sizeof(float)) + bkf_align16(cells * sizeof(unsigned short)) + bkf_align16((size_t)CH * B * sizeof(unsigned));
}
__host__ __device__ inline size_t bkf_out_bytes(int B, int CH) { return bkf_align16((size_t)CH * B * sizeof(double)); }
__host__ __device__ inline size_t bkf_smem_bytes(int T, int B, int RD, int CH) {
    return bkf_align16(((size_t)RD * B + 1) * sizeof(double))        // Bk ring + the +inf slot
           + bkf_align16((size_t)(SVX_MAX_TYPES + 2) * sizeof(int))  // packed moves
           + 2 * bkf_chunk_bytes(T, B, CH) + 2 * bkf_out_bytes(B, CH)
           + bkf_align16((size_t)4 * (CH + RD) * sizeof(int));       // per-wave band-offset tables of the staging code
}

// node word: kind (2 bits: 0 lattice node, 1 the end node, 3 outside) | lane of the (0,1) successor (7 bits, 127 = none)
// << 2 | lane of the (1,0) successor << 9.
// Stage chunk q (diagonals a0 = q * CH .. a0 + CH - 1) into buffer q & 1.  Every staging wave first copies the band offsets
// of diagonals a0 .. a0 + CH + RD - 1 into its own small LDS table.  wboff: [4 waves][CH + RD] ints.
__device__ __forceinline__ void bkf_stage(const PlaneGeo& g, const int* tpk, int T, int RD, int CH, int q, char* bufs, int* wboff,
                                          int tsub, int nsub) {
    const int B = g.B, Aout = g.A + 2;
    const int a0 = q * CH;
    const int Tn = T > 0 ? T : 1;
    char* base = bufs + (size_t)(q & 1) * bkf_chunk_bytes(T, B, CH);
    float* cost = reinterpret_cast<float*>(base);
    unsigned short* idx = reinterpret_cast<unsigned short*>(base + bkf_align16((size_t)CH * Tn * B * sizeof(float)));
    unsigned* node = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(idx) + bkf_align16((size_t)CH * Tn * B * sizeof(unsigned short)));
    const int dummy = RD * B;
    const int TB = T * B;
    const int lim = Aout - 1;
    int* wb = wboff + ((threadIdx.x >> 6) & 3) * (CH + RD);
    for (int k = threadIdx.x & 63; k < CH + RD; k += 64) {
        const int a = a0 + k;
        wb[k] = plane_bout(g.boff_in, a > lim ? lim : a);   // (past the last diagonal: never used, the moves are cut at lim)
    }
    wave_lds_sync();
    // one thread per column -- a (type, cell) pair or, past those, a node cell -- walking the chunk's diagonals; with fewer
    // columns than staging threads the diagonals are split over thread groups
    const int ncols = TB + B;
    const int ngroups = nsub / ncols > 0 ? nsub / ncols : 1;
    for (int cg = tsub; cg < ncols * ngroups; cg += nsub) {
        const int col = cg % ncols, grp = cg / ncols;
        const bool is_node = col >= TB;
        const int t = is_node ? 0 : col / B;
        const int b = is_node ? col - TB : col - t * B;
        const int pk = is_node ? (1 << 16) : tpk[t];
        const int xo = pk & 255, yo = (pk >> 8) & 255, st = pk >> 16;
        for (int i = grp; i < CH; i += ngroups) {
            const int a = a0 + i;
            const int boa = wb[i];
            const int yy = b + boa, xx = a - yy;
            const bool lattice = a <= lim && 0 <= xx && xx <= g.xs && 0 <= yy && yy <= g.ys;
            if (is_node) {
                const int bop = wb[i + 1];
                const int b01 = yy + 1 - bop, b10 = yy - bop;
                unsigned w = 3u | (127u << 2) | (127u << 9);
                if (lattice) {
                    const bool next = a + 1 <= lim;
                    const unsigned s01 = (next && yy + 1 <= g.ys && 0 <= b01 && b01 < B) ? (unsigned)b01 : 127u;
                    const unsigned s10 = (next && xx + 1 <= g.xs && 0 <= b10 && b10 < B) ? (unsigned)b10 : 127u;
                    w = ((xx == g.xs && yy == g.ys) ? 1u : 0u) | (s01 << 2) | (s10 << 9);
                }
                node[i * B + b] = w;
            } else {
                const int av = a + st;
                const int bv = yy + yo - wb[i + st];
                const bool ok = lattice && av <= lim && xx + xo <= g.xs && yy + yo <= g.ys && 0 <= bv && bv < B;
                float cv = 0.f;
                if (ok) cv = gld(g.costs + plane_cost_index(g, t, av - 2, bv));
                cost[i * TB + col] = cv;
                idx[i * TB + col] = (unsigned short)(ok ? (av % RD) * B + bv : dummy);
            }
        }
    }
}

__device__ __forceinline__ void bkf_flush(const PlaneGeo& g, const char* obuf, int B, int a0, int a_end, int tsub, int nsub) {
    const double* ob = reinterpret_cast<const double*>(obuf);
    const int n = (a_end - a0) * B;
    for (int e = tsub; e < n; e += nsub) gst(g.bsum + ((size_t)a0 * B + e), ob[e]);
}

__device__ void bk_fast(const PlaneGeo& g, const SvxTypes& ty, int CH, char* smem) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int A = __builtin_amdgcn_readfirstlane(g.A), B = g.B, Aout = A + 2, T = ty.n, NTt = ty.n + 2, RD = ty.maxstep + 1;
    const int Tn = T > 0 ? T : 1;
    double* ring = reinterpret_cast<double*>(smem);
    int* tpk = reinterpret_cast<int*>(smem + bkf_align16(((size_t)RD * B + 1) * sizeof(double)));
    char* bufs = reinterpret_cast<char*>(tpk) + bkf_align16((size_t)(SVX_MAX_TYPES + 2) * sizeof(int));
    const size_t chunk_bytes = bkf_chunk_bytes(T, B, CH);
    char* obufs = bufs + 2 * chunk_bytes;
    const size_t out_bytes = bkf_out_bytes(B, CH);
    int* wboff = reinterpret_cast<int*>(obufs + 2 * out_bytes);
    const size_t idx_off = bkf_align16((size_t)CH * Tn * B * sizeof(float));
    const size_t node_off = idx_off + bkf_align16((size_t)CH * Tn * B * sizeof(unsigned short));
    const double inf = __builtin_inf();
    for (int t = tid; t < NTt; t += BKF_THREADS) tpk[t] = (int)ty.x[t] | ((int)ty.y[t] << 8) | (((int)ty.x[t] + (int)ty.y[t]) << 16);
    for (int e = tid; e <= RD * B; e += BKF_THREADS) ring[e] = inf;
    __syncthreads();
    const int nchunks = (Aout + CH - 1) / CH;
    bkf_stage(g, tpk, T, RD, CH, nchunks - 1, bufs, wboff, tid, BKF_THREADS);
    __syncthreads();
    const double pen = g.pen;
    const int bb = lane < B ? lane : 0;   // idle lanes shadow cell 0 (they never store)
    const int TB = T * B;
    int slot = (Aout - 1) % RD;           // a % RD of the diagonal being closed (wave 0 only)
    double cur = inf;                     // Bk of this lane's cell on diagonal a + 1
    for (int q = nchunks - 1; q >= 0; q--) {
        const int a0 = q * CH;
        const int a_end = (a0 + CH) < Aout ? (a0 + CH) : Aout;
        if (wave >= 1) {
            if (q > 0) bkf_stage(g, tpk, T, RD, CH, q - 1, bufs, wboff, tid - 64, BKF_THREADS - 64);
            if (q + 1 < nchunks) {
                const int p0 = a0 + CH;
                bkf_flush(g, obufs + (size_t)((q + 1) & 1) * out_bytes, B, p0, (p0 + CH) < Aout ? (p0 + CH) : Aout, tid - 64, BKF_THREADS - 64);
            }
        } else {
            const char* base = bufs + (size_t)(q & 1) * chunk_bytes;
            const float* cost = reinterpret_cast<const float*>(base);
            const unsigned short* idx = reinterpret_cast<const unsigned short*>(base + idx_off);
            const unsigned* node = reinterpret_cast<const unsigned*>(base + node_off);
            double* obest = reinterpret_cast<double*>(obufs + (size_t)(q & 1) * out_bytes);
            // the type moves out of diagonal a0 + i: they reach diagonals >= a + 2, which are closed when a + 1 is being closed
            auto partial = [&](int i) {
                double r = inf;
#pragma unroll 4
                for (int t = 0; t < T; t++) {
                    const int o = i * TB + t * B + bb;
                    const double tot = (double)cost[o] + ring[idx[o]];
                    r = tot < r ? tot : r;
                }
                return r;
            };
            const int nrows = a_end - a0;
            double part = partial(nrows - 1);
            unsigned nw = node[(nrows - 1) * B + bb];
            for (int i = nrows - 1; i >= 0; i--) {
                const int inext = i > 0 ? i - 1 : 0;   // (the last diagonal re-reads itself: no branch)
                const unsigned nnw = node[inext * B + bb];
                const double npart = partial(inext);
                const int kind = nw & 3, s01 = (nw >> 2) & 127, s10 = (nw >> 9) & 127;
                const double p01 = __shfl(cur, s01 < B ? s01 : bb, SVX_WAVE);
                const double p10 = __shfl(cur, s10 < B ? s10 : bb, SVX_WAVE);
                double best = part;
                const double t01 = pen + p01, t10 = pen + p10;
                if (s01 < B && t01 < best) best = t01;
                if (s10 < B && t10 < best) best = t10;
                best = kind == 0 ? best : (kind == 1 ? 0.0 : inf);
                if (lane < B) {
                    ring[slot * B + lane] = best;
                    obest[i * B + lane] = best;
                }
                cur = best;
                part = npart;
                nw = nnw;
                slot = __builtin_amdgcn_readfirstlane(slot == 0 ? RD - 1 : slot - 1);
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
    }
    bkf_flush(g, obufs, B, 0, CH < Aout ? CH : Aout, tid, BKF_THREADS);   // chunk 0 sits in buffer 0
}

__global__ __launch_bounds__(BKF_THREADS) void k_bk_fast(const PlanePair* __restrict__ pairs, PlanePair one, int use_one, SvxTypes ty,
                                                         int B, int atb, int CH) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PlanePair P = use_one ? one : pairs[blockIdx.x];
    PlaneGeo g;
    if (!P.bsum || !plane_geo(P, ty, B, atb, &g)) return;   // (uniform) a skipped or failed pair
    bk_fast(g, ty, CH, smem);
}

template <bool RING>
__global__ __launch_bounds__(1024) void k_bk_wide(const PlanePair* __restrict__ pairs, PlanePair one, int use_one, SvxTypes ty, int B,
                                                  int atb) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PlanePair P = use_one ? one : pairs[blockIdx.x];
    PlaneGeo g;
    if (!P.bsum || !plane_geo(P, ty, B, atb, &g)) return;   // (uniform) a skipped or failed pair
    const size_t ring_bytes = RING ? (((size_t)(ty.maxstep + 1) * B * sizeof(double) + 15) & ~(size_t)15) : 0;
    bk_block<RING>(g, ty, reinterpret_cast<double*>(smem), reinterpret_cast<int*>(smem + ring_bytes));
}

// ------------------------------------------------------------------------------ slack of the rows of a path
constexpr int SK_THREADS = 512;
constexpr int SK_WAVES = SK_THREADS / SVX_WAVE;

__global__ __launch_bounds__(SK_THREADS) void k_path_slack(const PlanePair* __restrict__ pairs, PlanePair one, int use_one, SvxTypes ty,
                                                           int B, int atb) {
    __shared__ int scnt[SK_WAVES][2];
    __shared__ int sbo[SK_WAVES][2 * MAXSTEP];   // per wave: b_offset_out of diagonals c - maxstep + 1 .. c + maxstep of its row
    const PlanePair P = use_one ? one : pairs[blockIdx.x];
    if (!P.slack) return;   // (uniform) a skipped pair: nothing of it is written
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    PlaneGeo g;
    const bool ok_pair = P.bsum && plane_geo(P, ty, B, atb, &g);
    int cnt;
    if (!plane_row_count(P, ok_pair, &cnt)) return;   // (uniform) a failed pair
    const double inf = __builtin_inf();
    const double total = plane_total(g);
    int n_zero = 0, n_inf = 0;   // lane 0 of the wave counts
    for (int r = w; r < cnt; r += SK_WAVES) {
        const uint4 rv = gld16(P.rows + 4 * (size_t)r);
        int t_own, bui, bvi;
        double s = __builtin_nan("");
        if (plane_is_edge(g, ty, rv, &t_own, &bui, &bvi))   // (uniform over the wave)
            s = cut_scan<false>(g, ty, sbo[w], (int)rv.x + (int)rv.z, bui, (int)rv.y, (int)rv.w, nullptr) - total;
        if (lane == 0) {
            gst(P.slack + r, s);
            n_zero += s == 0.0 ? 1 : 0;
            n_inf += s == inf ? 1 : 0;
        }
    }
    if (P.summary) plane_summary(scnt, P.summary, cnt, n_zero, n_inf, 0);
}

inline int bk_threads(int B) {
    int t = ((B + 63) / 64) * 64;
    return t < 64 ? 64 : (t > 1024 ? 1024 : t);
}

// chunk length of the fast sweep, 0: the strided kernel (as dpf_choose_ch of svx_dp.hip: a workgroup should leave room for
// three more on its CU)
int bkf_choose_ch(int T, int B, int maxstep) {
    if (B > 64 || maxstep > 120) return 0;   // ring slots are 16-bit table entries
    const int opts[8] = {64, 48, 32, 24, 16, 12, 8, 4};
    const size_t budgets[3] = {36 * 1024, 52 * 1024, 150 * 1024};
    for (int k = 0; k < 3; k++)
        for (int i = 0; i < 8; i++)
            if (bkf_smem_bytes(T, B, maxstep + 1, opts[i]) <= budgets[k]) return opts[i];
    return 0;
}

// the backward sweep of n pairs: `dev` descriptors, or the one descriptor `one` when dev is null
int launch_backward(svx_ctx* ctx, const PlanePair* dev, const PlanePair& one, int n, const SvxTypes& types, int B, int atb) {
    const int use_one = dev ? 0 : 1;
    const int CH = bkf_choose_ch(types.n, B, types.maxstep);
    if (CH > 0) {
        const size_t smem = bkf_smem_bytes(types.n, B, types.maxstep + 1, CH);
        if (smem > 64 * 1024)
            SVX_HIP(ctx, hipFuncSetAttribute((const void*)k_bk_fast, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        hipLaunchKernelGGL(k_bk_fast, dim3(n), dim3(BKF_THREADS), smem, ctx->stream, dev, one, use_one, types, B, atb, CH);
        SVX_LAUNCH_CHECK(ctx, "k_bk_fast");
        return SVX_OK;
    }
    const size_t ring = (((size_t)(types.maxstep + 1) * B * sizeof(double)) + 15) & ~(size_t)15;
    const size_t tabs = bkw_tab_bytes(types.n + 2);
    const int nt = bk_threads(B);
    if (ring + tabs <= 150 * 1024) {
        const size_t smem = ring + tabs;
        if (smem > 64 * 1024)
            SVX_HIP(ctx, hipFuncSetAttribute((const void*)k_bk_wide<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        hipLaunchKernelGGL(k_bk_wide<true>, dim3(n), dim3(nt), smem, ctx->stream, dev, one, use_one, types, B, atb);
    } else {
        hipLaunchKernelGGL(k_bk_wide<false>, dim3(n), dim3(nt), tabs, ctx->stream, dev, one, use_one, types, B, atb);
    }
    SVX_LAUNCH_CHECK(ctx, "k_bk_wide");
    return SVX_OK;
}

}  // namespace

int svxl_sparse_dp_backward(svx_ctx* ctx, const float* costs, const int* boff_in, int A, int B, const SvxTypes& types, double pen,
                            int xs, int ys, double* bsum) {
    PlanePair one{};
    one.costs = costs; one.boff_in = boff_in; one.bsum = bsum;
    one.pen = pen; one.A = A; one.xs = xs; one.ys = ys;
    return launch_backward(ctx, nullptr, one, 1, types, B, 0);
}

int svxl_path_slack(svx_ctx* ctx, const float* costs, const int* boff_in, int A, int B, const SvxTypes& types, double pen, int xs,
                    int ys, const double* csum, const double* bsum, const int* rows, const int* n_rows, int cap, double* slack) {
    PlanePair one{};
    one.costs = costs; one.boff_in = boff_in; one.csum = csum; one.bsum = const_cast<double*>(bsum);   // (read only here)
    one.rows = rows; one.n_rows = n_rows; one.slack = slack;
    one.pen = pen; one.A = A; one.xs = xs; one.ys = ys; one.cap = cap;
    hipLaunchKernelGGL(k_path_slack, dim3(1), dim3(SK_THREADS), 0, ctx->stream, (const PlanePair*)nullptr, one, 1, types, B, 0);
    SVX_LAUNCH_CHECK(ctx, "k_path_slack");
    return SVX_OK;
}

int svxl_backward_batch(svx_ctx* ctx, const PlanePair* dev, int n, const SvxTypes& types, int B, int atb) {
    return launch_backward(ctx, dev, PlanePair{}, n, types, B, atb);
}

// What both batch entries put into a pair's descriptor from the aligner's own record of it.
void svxl_plane_pair(PlanePair& r, const SvxPairDev& P, int32_t* summary) {
    const SvxLevel& Lv = P.lev[0];
    r = PlanePair{};
    r.costs = Lv.costs;
    r.boff_in = Lv.boff;
    r.path_len = Lv.path_len;
    r.pen_dev = Lv.pen;
    r.status = P.status;
    r.csum = Lv.csum;
    r.xp = Lv.xp; r.yp = Lv.yp; r.bpk = Lv.bpk;
    r.rows = Lv.align;
    r.n_rows = Lv.n_align;
    r.summary = summary;
    r.xs = Lv.n[0];
    r.ys = Lv.n[1];
    r.cap = Lv.n[0] + Lv.n[1] + 2;
}

extern "C" int svx_row_slack(svx_ctx* ctx, double* const* slack, int32_t* summary, int n_pairs) {
    if (!ctx) return svx_fail(nullptr, SVX_ERR_ARG, "svx_row_slack: ctx is NULL");
    NEED(ctx, slack && summary, "svx_row_slack: null argument");
    NEED(ctx, aligned16(summary), "svx_row_slack: summary must be 16-byte aligned");
    NEED(ctx, n_pairs >= 0, "svx_row_slack: negative n_pairs");
    SvxLastCall lc;
    int rc = svxl_last_call(ctx, "svx_row_slack", n_pairs, "row slack needs", &lc);
    if (rc) return rc;
    // ---- scratch: [descriptors] uploaded, then one Bk plane per pair that is not skipped
    const size_t b_desc = up256((size_t)n_pairs * sizeof(PlanePair));
    size_t b_all = b_desc;
    for (int p = 0; p < n_pairs; p++)
        if (slack[p]) b_all += up256(((size_t)lc.pair(p).lev[0].path_cap + 2) * lc.band * sizeof(double));
    char *pin, *dev;
    rc = svxl_scratch_begin(ctx, "svx_row_slack", b_desc, b_all, &pin, &dev);
    if (rc) return rc;
    PlanePair* hp = reinterpret_cast<PlanePair*>(pin);
    size_t at = b_desc;
    for (int p = 0; p < n_pairs; p++) {
        svxl_plane_pair(hp[p], lc.pair(p), summary + 4 * (size_t)p);
        hp[p].slack = slack[p];
        if (slack[p]) {
            hp[p].bsum = reinterpret_cast<double*>(dev + at);
            at += up256(((size_t)lc.pair(p).lev[0].path_cap + 2) * lc.band * sizeof(double));
        }
    }
    rc = svxl_scratch_upload(ctx, (size_t)n_pairs * sizeof(PlanePair));
    if (rc) return rc;
    const PlanePair* dp = reinterpret_cast<const PlanePair*>(dev);
    rc = launch_backward(ctx, dp, PlanePair{}, n_pairs, *lc.types, lc.band, 1);
    if (rc) return rc;
    hipLaunchKernelGGL(k_path_slack, dim3(n_pairs), dim3(SK_THREADS), 0, ctx->stream, dp, PlanePair{}, 0, *lc.types, lc.band, 1);
    SVX_LAUNCH_CHECK(ctx, "k_path_slack");
    return SVX_OK;
}
