// svx_alt.hip -- row alternatives: per returned row the best competing edge of its cut, the detour of the best path through
// that edge, and the regret of caller-given rows (include/svx.h: svx_path_alternatives, svx_row_alternatives; DESIGN.md 6e;
// gfx950 only).
//
// Everything is read off the two planes the library already has: F, the stored forward csum, and Bk, the backward plane of
// svx_slack.hip (k_bk_fast / k_bk_wide, run again into the post-processing scratch by svx_row_alternatives).
//
//   k_row_alt       one workgroup per pair, one wave per row.
//                   Phase 1 fills a per-diagonal table in scratch: the band cell of the returned path's node on that diagonal
//                   and the number i of that node P_i (the start of row i; P_R is the end of the last row), or (-1, -1).  One
//                   workgroup barrier.
//                   Phase 2, per row, is the cut scan of k_path_slack carrying (cand, order key) instead of cand alone: lanes
//                   take (diagonal, cell) targets v in ascending order and loop over the moves in list order, so a lane's first
//                   strictly smaller candidate is its smallest key; a wave arg-min on (cand, key) follows.  The per-wave
//                   band-offset table stays in LDS.
//                   Phase 3, for a measured row, are the two walks, on wave-uniform state.  Backward from u: a chain of
//                   dependent loads (table entry, back-pointer) per step, rows staged in the wave's LDS slots in walk order.
//                   Forward from v: the lanes take the moves, each tests its edge and w + Bk(s) == Bk(node), the first match in
//                   list order comes out of a ballot; rows staged from the other end of the same slots.  A walk that fails or
//                   grows past K writes nothing but the span.  Otherwise the lanes write the detour in document order, one
//                   16-byte store per row, and price each row from its cost cell.
//   k_given_regret  one thread per given row: ((F(u) + w) + Bk(v)) - total from three resident reads behind the validity checks.
// A row that fails the range checks forms no address.  Both cost layouts are read: [T][A][B] (per-op) and [A][T][B] (fused
// pipeline); back-pointers come as packed bytes or as two int32 planes.  Plain C++, vector stores only.
#include "svx_common.h"

namespace {

struct AltPair {
    const float* costs;
    const int* boff_in;         // [A]
    const int* path_len;        // device A (the pipeline), or null: A below
    const double* pen_dev;      // device penalty (the pipeline), or null: pen below
    const int* status;          // the aligner's info[1] of the pair, or null
    const double* csum;         // [A+2][B] forward plane
    const double* bsum;         // [A+2][B] backward plane
    const int* xp;              // int32 back-pointers, or null when bpk is given
    const int* yp;
    const unsigned char* bpk;   // packed back-pointers xp << 4 | yp, 0xFF = none
    const int* rows;            // [cap][4]
    const int* n_rows;          // [1]
    int* table;                 // [A+2][2] scratch: (cell, node number) of the path node on each diagonal
    double* slack;              // [cap] or null
    int* edge;                  // [cap][4]; null: the pair is skipped
    int* span;                  // [cap][4]
    int* detour;                // [cap][K][4] or null: edges only
    double* dscores;            // [cap][K] or null
    const int* given;           // [given_cap][4] or null
    const int* given_info;      // [2]
    double* regret;             // [given_cap]
    int* summary;               // [4] or null (per-op entry)
    double pen;
    int A, xs, ys, cap, given_cap, pad;
};

struct AltGeo {
    const float* costs;
    const int* boff_in;
    int A, B, T, atb, xs, ys;
    double pen;
};

__device__ __forceinline__ bool alt_geo(const AltPair& P, const SvxTypes& ty, int B, int atb, AltGeo* g) {
    if (P.status && gld(P.status) != 0) return false;
    g->A = P.path_len ? gld(P.path_len) : P.A;
    if (g->A <= 0) return false;
    g->costs = P.costs;
    g->boff_in = P.boff_in;
    g->B = B;
    g->T = ty.n;
    g->atb = atb;
    g->xs = P.xs;
    g->ys = P.ys;
    g->pen = P.pen_dev ? gld(P.pen_dev) : P.pen;
    return true;
}

__device__ __forceinline__ size_t alt_cost_index(const AltGeo& g, int t, int a, int b) {
    return g.atb ? ((size_t)a * g.T + t) * g.B + b : ((size_t)t * g.A + a) * g.B + b;
}
// b_offset_out[a], 0 <= a < A + 2
__device__ __forceinline__ int alt_bout(const int* boff_in, int a) { return a < 2 ? gld(boff_in) : gld(boff_in + (a - 2)) + 1; }

// total = F(end); +inf when the end node is no band cell
__device__ __forceinline__ double alt_total(const AltPair& P, const AltGeo& g) {
    const long long xs = g.xs, ys = g.ys, Aout = (long long)g.A + 2;
    if (xs >= 0 && ys >= 0 && xs + ys < Aout) {
        const long long be = ys - alt_bout(g.boff_in, (int)(xs + ys));
        if (be >= 0 && be < g.B) return gld(P.csum + ((size_t)(xs + ys) * g.B + be));
    }
    return __builtin_inf();
}

// Is the row an edge of the search space?  Range checks, the move is in the list (-> *t, its first index), both nodes are
// band cells (-> *bu, *bv).  No address is formed before the ranges are known to hold.
__device__ __forceinline__ bool alt_is_edge(const AltGeo& g, const SvxTypes& ty, uint4 rv, int* t, int* bu, int* bv) {
    const long long x0 = (int)rv.x, xl = (int)rv.y, y0 = (int)rv.z, yl = (int)rv.w;
    const long long Aout = (long long)g.A + 2, c = x0 + y0;
    if (!(x0 >= 0 && xl >= 0 && y0 >= 0 && yl >= 0 && x0 + xl <= g.xs && y0 + yl <= g.ys && xl + yl >= 1 && c + xl + yl < Aout)) return false;
    int tt = -1;
    for (int k = ty.n + 1; k >= 0; k--)
        if (ty.x[k] == xl && ty.y[k] == yl) tt = k;
    if (tt < 0) return false;
    const long long b0 = y0 - alt_bout(g.boff_in, (int)c);
    const long long b1 = y0 + yl - alt_bout(g.boff_in, (int)(c + xl + yl));
    if (!(b0 >= 0 && b0 < g.B && b1 >= 0 && b1 < g.B)) return false;
    *t = tt; *bu = (int)b0; *bv = (int)b1;
    return true;
}

// Is node (x, y) -> (x + xo, y + yo) by move t an edge of E or E_b?  (x, y) is a band cell of diagonal a = x + y; -> the
// successor's diagonal and cell.
__device__ __forceinline__ bool alt_out_edge(const AltGeo& g, int x, int y, int t, int xo, int yo, int* av_out, int* bv_out) {
    const int a = x + y, av = a + xo + yo;
    if (av >= g.A + 2) return false;
    const int vx = x + xo, vy = y + yo;
    const int bv = vy - alt_bout(g.boff_in, av);
    if (bv < 0 || bv >= g.B) return false;
    const bool bx = x == 0 && 0 <= y && y <= g.ys;
    const bool by = !bx && y == 0 && 0 <= x && x <= g.xs;
    const bool gen = !bx && !by && 1 <= x && x <= g.xs && 1 <= y && y <= g.ys && a - 2 < g.A;
    bool ok = (bx || by || gen) && 1 <= vx && vx <= g.xs && 1 <= vy && vy <= g.ys && av - 2 < g.A;
    if (t == g.T) ok = ok || (bx && vy <= g.ys);
    else if (t == g.T + 1) ok = ok || ((by || (bx && y == 0)) && vx <= g.xs);
    *av_out = av; *bv_out = bv;
    return ok;
}

constexpr int AL_THREADS = 512;
constexpr int AL_WAVES = AL_THREADS / SVX_WAVE;
constexpr int AL_MAXSTEP = 200;   // make_types: type sizes are at most 100 a side
// dynamic LDS: per wave K staged rows (16 bytes) and K move indices
__host__ __device__ inline size_t al_smem_bytes(int K) { return (size_t)AL_WAVES * K * (4 * sizeof(int) + sizeof(int)); }

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(AL_THREADS) void k_row_alt(const AltPair* __restrict__ pairs, AltPair one, int use_one, SvxTypes ty, int B,
                                                        int atb, int K, double max_slack) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int scnt[AL_WAVES][3];
    __shared__ int sbo[AL_WAVES][2 * AL_MAXSTEP];   // per wave: b_offset_out of diagonals c - maxstep + 1 .. c + maxstep of its row
    const AltPair P = use_one ? one : pairs[blockIdx.x];
    if (!P.edge) return;   // (uniform) a skipped pair: nothing of it is written
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    AltGeo g;
    const bool ok_pair = alt_geo(P, ty, B, atb, &g);
    int cnt = ok_pair ? gld(P.n_rows) : -1;
    if (P.summary) {
        if (cnt < 0 || cnt > P.cap) {   // (uniform) a failed pair
            if (tid == 0) gst16(P.summary, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
            return;
        }
    } else {
        if (!ok_pair) return;
        cnt = cnt < 0 ? 0 : (cnt > P.cap ? P.cap : cnt);
    }
    const int T = ty.n, NTt = ty.n + 2;
    const int Aout = g.A + 2;
    const long long xs = g.xs, ys = g.ys;
    const double inf = __builtin_inf();
    const double total = alt_total(P, g);
    const bool walks = P.detour != nullptr;
    // ---- phase 1: the path's node on every diagonal
    if (walks) {
        for (int a = tid; a < Aout; a += AL_THREADS) {
            gst(P.table + 2 * (size_t)a, -1);
            gst(P.table + 2 * (size_t)a + 1, -1);
        }
        __syncthreads();
        for (int i = tid; i <= cnt && cnt > 0; i += AL_THREADS) {
            const uint4 rv = gld16(P.rows + 4 * (size_t)(i < cnt ? i : cnt - 1));
            long long x = (int)rv.x, y = (int)rv.z;
            if (i == cnt) { x += (int)rv.y; y += (int)rv.w; }
            if (x < 0 || x > xs || y < 0 || y > ys || x + y >= Aout) continue;
            const long long b = y - alt_bout(g.boff_in, (int)(x + y));
            if (b < 0 || b >= B) continue;
            gst(P.table + 2 * (size_t)(x + y), (int)b);
            gst(P.table + 2 * (size_t)(x + y) + 1, i);
        }
        __syncthreads();
    }
    int4* stage = reinterpret_cast<int4*>(smem) + (size_t)w * K;                               // this wave's K row slots
    int* stage_t = reinterpret_cast<int*>(smem + (size_t)AL_WAVES * K * sizeof(int4)) + (size_t)w * K;
    int n_edge = 0, n_written = 0, n_long = 0;   // lane 0 of the wave counts
    const int items = ty.maxstep * B;
    for (int r = w; r < cnt; r += AL_WAVES) {
        const uint4 rv = gld16(P.rows + 4 * (size_t)r);
        int t_own, bui, bvi;
        const bool valid = alt_is_edge(g, ty, rv, &t_own, &bui, &bvi);   // (uniform over the wave)
        double s = __builtin_nan("");
        bool has_edge = false;
        int e_ux = -1, e_xo = -1, e_uy = -1, e_yo = -1, e_t = 0;
        if (valid) {
            const int ci = (int)rv.x + (int)rv.z, xli = (int)rv.y, yli = (int)rv.w;
            // the band offsets of every diagonal an edge across this cut can touch, once per row
            const int ms = ty.maxstep, dbase = ci - ms + 1;
            int* bo = sbo[w];
            __builtin_amdgcn_wave_barrier();   // (the row before may still be reading the table)
            for (int k = lane; k < 2 * ms; k += SVX_WAVE) {
                const long long a = (long long)dbase + k;
                bo[k] = (a >= 0 && a < Aout) ? alt_bout(g.boff_in, (int)a) : 0;
            }
            wave_lds_sync();
            // ---- phase 2: the cut scan with the order key (diagonal of v, cell of v, move index)
            double alt = inf;
            unsigned long long key = ~0ull;
            for (int it = lane; it < items; it += SVX_WAVE) {
                const int dv = it / B + 1, bv = it - (dv - 1) * B;
                const long long avl = (long long)ci + dv;
                if (avl >= Aout) continue;
                const int av = (int)avl;
                const int vy = bv + bo[av - dbase], vx = av - vy;
                if (vx < 0 || vx > xs || vy < 0 || vy > ys) continue;
                const double bk = gld(P.bsum + ((size_t)av * B + bv));
                for (int t = 0; t < NTt; t++) {
                    const int xo = ty.x[t], yo = ty.y[t], st = xo + yo;
                    if (st < dv) continue;             // the edge starts behind the cut
                    const int au = av - st, ux = vx - xo, uy = vy - yo;
                    if (au < 0 || ux < 0 || uy < 0) continue;
                    const int bp = uy - bo[au - dbase];
                    if (bp < 0 || bp >= B) continue;
                    if (au == ci && bp == bui && xo == xli && yo == yli) continue;   // the row's own edge
                    const double wgt = t < T ? (double)gld(g.costs + alt_cost_index(g, t, av - 2, bv)) : g.pen;
                    const double cand = (gld(P.csum + ((size_t)au * B + bp)) + wgt) + bk;
                    if (cand < alt) {   // (a lane meets its keys in ascending order)
                        alt = cand;
                        key = (unsigned long long)it * (unsigned)NTt + (unsigned)t;
                    }
                }
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const double oa = __shfl_xor(alt, o, SVX_WAVE);
                const unsigned long long ok = __shfl_xor(key, o, SVX_WAVE);
                if (oa < alt || (oa == alt && ok < key)) { alt = oa; key = ok; }
            }
            s = alt - total;
            has_edge = alt < inf;
            if (has_edge) {
                e_t = (int)(key % (unsigned)NTt);
                const int it = (int)(key / (unsigned)NTt);
                const int dv = it / B + 1, bv = it - (dv - 1) * B;
                const int av = ci + dv;
                const int vy = bv + bo[av - dbase], vx = av - vy;
                e_xo = ty.x[e_t]; e_yo = ty.y[e_t];
                e_ux = vx - e_xo; e_uy = vy - e_yo;
            }
        }
        if (lane == 0) {
            if (P.slack) gst(P.slack + r, s);
            gst16(P.edge + 4 * (size_t)r, (uint32_t)e_ux, (uint32_t)e_xo, (uint32_t)e_uy, (uint32_t)e_yo);
            n_edge += has_edge ? 1 : 0;
        }
        int status = 2, lo = -1, hi = -1, nd = -1;
        if (has_edge && walks && s <= max_slack) {
            // ---- phase 3: the two walks (every value wave-uniform)
            status = 0;
            int nb = 0, nf = 0;
            int x = __builtin_amdgcn_readfirstlane(e_ux), y = __builtin_amdgcn_readfirstlane(e_uy);
            __builtin_amdgcn_wave_barrier();   // (the row before may still be reading the slots)
            for (;;) {   // backward: the stored back-pointers, until a node of the returned path
                const int a = x + y;
                const int b = y - alt_bout(g.boff_in, a);
                if (gld(P.table + 2 * (size_t)a) == b) { lo = gld(P.table + 2 * (size_t)a + 1); break; }
                if (nb == K - 1) { status = 1; break; }
                const size_t o = (size_t)a * B + b;
                int px, py;
                if (P.bpk) {
                    const int v = gld(P.bpk + o);
                    px = v == 0xFF ? -42 : (v >> 4);
                    py = v == 0xFF ? -42 : (v & 15);
                } else {
                    px = gld(P.xp + o);
                    py = gld(P.yp + o);
                }
                if (px < 0 || py < 0 || px + py < 1 || px > x || py > y) { status = 3; break; }
                int tt = -1;
                for (int k = NTt - 1; k >= 0; k--)
                    if (ty.x[k] == px && ty.y[k] == py) tt = k;
                const int bpre = (y - py) - alt_bout(g.boff_in, a - px - py);
                if (tt < 0 || bpre < 0 || bpre >= B) { status = 3; break; }
                if (lane == 0) {
                    stage[nb] = make_int4(x - px, px, y - py, py);
                    stage_t[nb] = tt;
                }
                x -= px; y -= py;
                nb++;
            }
            if (status == 0) {   // forward: the first move in list order that keeps Bk exact, until a node of the returned path
                x = __builtin_amdgcn_readfirstlane(e_ux + e_xo);
                y = __builtin_amdgcn_readfirstlane(e_uy + e_yo);
                for (;;) {
                    const int a = x + y;
                    const int b = y - alt_bout(g.boff_in, a);
                    if (gld(P.table + 2 * (size_t)a) == b) { hi = gld(P.table + 2 * (size_t)a + 1); break; }
                    if (nb + 1 + nf == K) { status = 1; break; }
                    const double here = gld(P.bsum + ((size_t)a * B + b));
                    int tt = -1;
                    for (int t0 = 0; t0 < NTt && tt < 0; t0 += SVX_WAVE) {
                        const int t = t0 + lane;
                        bool match = false;
                        if (t < NTt) {
                            int av, bv;
                            if (alt_out_edge(g, x, y, t, ty.x[t], ty.y[t], &av, &bv)) {
                                const double wgt = t < T ? (double)gld(g.costs + alt_cost_index(g, t, av - 2, bv)) : g.pen;
                                match = wgt + gld(P.bsum + ((size_t)av * B + bv)) == here;
                            }
                        }
                        const unsigned long long m = __ballot(match);
                        if (m) tt = t0 + __builtin_ctzll(m);
                    }
                    if (tt < 0) { status = 3; break; }
                    const int mxo = ty.x[tt], myo = ty.y[tt];
                    if (lane == 0) {
                        stage[K - 1 - nf] = make_int4(x, mxo, y, myo);
                        stage_t[K - 1 - nf] = tt;
                    }
                    x += mxo; y += myo;
                    nf++;
                }
            }
            if (status == 0) {
                nd = nb + 1 + nf;
                wave_lds_sync();
                for (int j = lane; j < nd; j += SVX_WAVE) {   // document order: the backward rows reversed, the edge, the forward rows
                    int4 row;
                    int tt;
                    if (j < nb) { row = stage[nb - 1 - j]; tt = stage_t[nb - 1 - j]; }
                    else if (j == nb) { row = make_int4(e_ux, e_xo, e_uy, e_yo); tt = e_t; }
                    else { row = stage[K - 1 - (j - nb - 1)]; tt = stage_t[K - 1 - (j - nb - 1)]; }
                    gst16(P.detour + 4 * ((size_t)r * K + j), (uint32_t)row.x, (uint32_t)row.y, (uint32_t)row.z, (uint32_t)row.w);
                    if (P.dscores) {
                        double sc = 0.0;
                        if (tt < T) {   // max(cost cell, 0) / (xo yo); a deletion scores 0
                            const int av = row.x + row.y + row.z + row.w;
                            const int bv = row.z + row.w - alt_bout(g.boff_in, av);
                            const double cst = (double)gld(g.costs + alt_cost_index(g, tt, av - 2, bv));
                            sc = (cst < 0.0 ? 0.0 : cst) / (double)(row.y * row.w);
                        }
                        gst(P.dscores + ((size_t)r * K + j), sc);
                    }
                }
            } else {
                lo = hi = -1;
            }
        }
        if (lane == 0) {
            gst16(P.span + 4 * (size_t)r, (uint32_t)lo, (uint32_t)hi, (uint32_t)nd, (uint32_t)status);
            n_written += status == 0 ? 1 : 0;
            n_long += status == 1 ? 1 : 0;
        }
    }
    if (!P.summary) return;
    if (lane == 0) { scnt[w][0] = n_edge; scnt[w][1] = n_written; scnt[w][2] = n_long; }
    __syncthreads();
    if (tid == 0) {
        int e = 0, d = 0, l = 0;
        for (int u = 0; u < AL_WAVES; u++) { e += scnt[u][0]; d += scnt[u][1]; l += scnt[u][2]; }
        gst16(P.summary, (uint32_t)cnt, (uint32_t)e, (uint32_t)d, (uint32_t)l);
    }
}

constexpr int GR_THREADS = 256;

__global__ __launch_bounds__(GR_THREADS) void k_given_regret(const AltPair* __restrict__ pairs, AltPair one, int use_one, SvxTypes ty, int B,
                                                             int atb) {
    const AltPair P = use_one ? one : pairs[blockIdx.y];
    if (!P.edge || !P.given) return;   // (uniform)
    AltGeo g;
    if (!alt_geo(P, ty, B, atb, &g)) return;
    if (gld(P.given_info + 1) != 0) return;
    int cnt = gld(P.given_info);
    cnt = cnt < 0 ? 0 : (cnt > P.given_cap ? P.given_cap : cnt);
    const int i = blockIdx.x * GR_THREADS + threadIdx.x;
    if (i >= cnt) return;
    const uint4 rv = gld16(P.given + 4 * (size_t)i);
    int t, bu, bv;
    double out = __builtin_nan("");
    if (alt_is_edge(g, ty, rv, &t, &bu, &bv)) {
        const int c = (int)rv.x + (int)rv.z, av = c + (int)rv.y + (int)rv.w;
        const double wgt = t < ty.n ? (double)gld(g.costs + alt_cost_index(g, t, av - 2, bv)) : g.pen;
        out = ((gld(P.csum + ((size_t)c * B + bu)) + wgt) + gld(P.bsum + ((size_t)av * B + bv))) - alt_total(P, g);
    }
    gst(P.regret + i, out);
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

int launch_alt(svx_ctx* ctx, const AltPair* dev, const AltPair& one, int n, const SvxTypes& types, int B, int atb, int K, double max_slack,
               int max_given) {
    const int use_one = dev ? 0 : 1;
    const size_t smem = al_smem_bytes(K);   // at most 40 KB (K <= 256), beside 6.5 KB of static tables
    hipLaunchKernelGGL(k_row_alt, dim3(n), dim3(AL_THREADS), smem, ctx->stream, dev, one, use_one, types, B, atb, K, max_slack);
    SVX_LAUNCH_CHECK(ctx, "k_row_alt");
    if (max_given > 0) {
        hipLaunchKernelGGL(k_given_regret, dim3((max_given + GR_THREADS - 1) / GR_THREADS, n), dim3(GR_THREADS), 0, ctx->stream, dev, one,
                           use_one, types, B, atb);
        SVX_LAUNCH_CHECK(ctx, "k_given_regret");
    }
    return SVX_OK;
}

// the argument rules svx_path_alternatives and svx_row_alternatives share for one svx_alt record
int check_alt(svx_ctx* ctx, const char* who, const svx_alt& a) {
    NEED(ctx, a.edge && a.span, "%s: null edge / span", who);
    NEED(ctx, aligned16(a.edge) && aligned16(a.span) && aligned16(a.detour) && aligned16(a.given),
         "%s: edge, span, detour and given must be 16-byte aligned", who);
    NEED(ctx, !a.given || (a.regret && a.given_info && a.given_cap >= 0), "%s: given rows need regret, given_info and a capacity >= 0", who);
    return SVX_OK;
}

int check_limits(svx_ctx* ctx, const char* who, int max_detour, double max_slack) {
    NEED(ctx, max_detour >= 1 && max_detour <= SVX_ALT_MAX_DETOUR, "%s: max_detour %d outside [1, %d]", who, max_detour, SVX_ALT_MAX_DETOUR);
    NEED(ctx, max_slack == max_slack, "%s: max_slack is NaN", who);
    return SVX_OK;
}

void fill_outputs(AltPair& r, const svx_alt& a) {
    r.slack = a.slack; r.edge = a.edge; r.span = a.span; r.detour = a.detour; r.dscores = a.detour_scores;
    r.given = a.given; r.given_info = a.given_info; r.regret = a.regret; r.given_cap = a.given ? a.given_cap : 0;
}

}  // namespace

int svxl_path_alternatives(svx_ctx* ctx, const float* costs, const int* boff_in, int A, int B, const SvxTypes& types, double pen, int xs,
                           int ys, const double* csum, const double* bsum, const int* xp, const int* yp, const int* rows, const int* n_rows,
                           int cap, const svx_alt* alt, int max_detour, double max_slack) {
    int rc = check_alt(ctx, "svx_path_alternatives", *alt);
    if (rc) return rc;
    rc = check_limits(ctx, "svx_path_alternatives", max_detour, max_slack);
    if (rc) return rc;
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    char *pin, *dev;
    rc = svxl_scratch_begin(ctx, "svx_path_alternatives", 0, up256(((size_t)A + 2) * 2 * sizeof(int)), &pin, &dev);
    if (rc) return rc;
    AltPair one{};
    one.costs = costs; one.boff_in = boff_in; one.csum = csum; one.bsum = bsum; one.xp = xp; one.yp = yp;
    one.rows = rows; one.n_rows = n_rows; one.table = reinterpret_cast<int*>(dev);
    one.pen = pen; one.A = A; one.xs = xs; one.ys = ys; one.cap = cap;
    fill_outputs(one, *alt);
    return launch_alt(ctx, nullptr, one, 1, types, B, 0, max_detour, max_slack, one.given_cap);
}

extern "C" int svx_row_alternatives(svx_ctx* ctx, const svx_alt* alt, int max_detour, double max_slack, int32_t* summary, int n_pairs) {
    if (!ctx) return svx_fail(nullptr, SVX_ERR_ARG, "svx_row_alternatives: ctx is NULL");
    NEED(ctx, alt && summary, "svx_row_alternatives: null argument");
    NEED(ctx, aligned16(summary), "svx_row_alternatives: summary must be 16-byte aligned");
    NEED(ctx, n_pairs >= 0, "svx_row_alternatives: negative n_pairs");
    int rc = check_limits(ctx, "svx_row_alternatives", max_detour, max_slack);
    if (rc) return rc;
    const SvxPairDev* host[2] = {nullptr, nullptr};
    int np[2] = {0, 0}, band = 0, dtype = 0, d = 0;
    const SvxTypes* types = nullptr;
    const bool have = svxl_last_batch(ctx, host, np, &band) && svxl_last_batch_types(ctx, &dtype, &d, &types);
    NEED(ctx, have && np[0] + np[1] > 0, "svx_row_alternatives: no earlier svx_align_batch / svx_align_around call on this context");
    NEED(ctx, n_pairs == np[0] + np[1], "svx_row_alternatives: %d pairs given, the last call had %d", n_pairs, np[0] + np[1]);
    for (int h = 0; h < 2; h++)
        for (int i = 0; i < np[h]; i++)
            NEED(ctx, host[h][i].lev[0].costs,
                 "svx_row_alternatives: the last call ran the tile sweep, which keeps no cost array (a_b_costs is NULL): row "
                 "alternatives need a band of at most 64 cells in the straight and around-wide modes");
    int max_given = 0;
    for (int p = 0; p < n_pairs; p++) {
        if (!alt[p].edge) continue;   // a skipped pair
        rc = check_alt(ctx, "svx_row_alternatives", alt[p]);
        if (rc) return rc;
        if (alt[p].given && alt[p].given_cap > max_given) max_given = alt[p].given_cap;
    }
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    rc = svx_flush(ctx);  // with the software pipeline on, the call's second half is complete only behind this
    if (rc) return rc;
    // ---- scratch: [sweep descriptors][alt descriptors] uploaded, then per pair that is not skipped one Bk plane and one
    //      node table of (path capacity + 2) entries
    const size_t b_sweep = up256((size_t)n_pairs * sizeof(SlackPair));
    const size_t b_desc = b_sweep + up256((size_t)n_pairs * sizeof(AltPair));
    size_t b_all = b_desc;
    {
        int p = 0;
        for (int h = 0; h < 2; h++)
            for (int i = 0; i < np[h]; i++, p++)
                if (alt[p].edge) {
                    const size_t diag = (size_t)host[h][i].lev[0].path_cap + 2;
                    b_all += up256(diag * band * sizeof(double)) + up256(diag * 2 * sizeof(int));
                }
    }
    char *pin, *dev;
    rc = svxl_scratch_begin(ctx, "svx_row_alternatives", b_desc, b_all, &pin, &dev);
    if (rc) return rc;
    SlackPair* hs = reinterpret_cast<SlackPair*>(pin);
    AltPair* hp = reinterpret_cast<AltPair*>(pin + b_sweep);
    size_t at = b_desc;
    int p = 0;
    for (int h = 0; h < 2; h++) {
        for (int i = 0; i < np[h]; i++, p++) {
            const SvxPairDev& P = host[h][i];
            const SvxLevel& Lv = P.lev[0];
            SlackPair& s = hs[p];
            AltPair& r = hp[p];
            s = SlackPair{};
            r = AltPair{};
            s.costs = r.costs = Lv.costs;
            s.boff_in = r.boff_in = Lv.boff;
            s.path_len = r.path_len = Lv.path_len;
            s.pen_dev = r.pen_dev = Lv.pen;
            s.status = r.status = P.status;
            s.xs = r.xs = Lv.n[0];
            s.ys = r.ys = Lv.n[1];
            r.csum = Lv.csum;
            r.xp = Lv.xp; r.yp = Lv.yp; r.bpk = Lv.bpk;
            r.rows = Lv.align;
            r.n_rows = Lv.n_align;
            r.summary = summary + 4 * (size_t)p;
            r.cap = Lv.n[0] + Lv.n[1] + 2;
            if (alt[p].edge) {
                fill_outputs(r, alt[p]);
                const size_t diag = (size_t)Lv.path_cap + 2;
                s.bsum = reinterpret_cast<double*>(dev + at);
                r.bsum = s.bsum;
                at += up256(diag * band * sizeof(double));
                r.table = reinterpret_cast<int*>(dev + at);
                at += up256(diag * 2 * sizeof(int));
            }
        }
    }
    rc = svxl_scratch_upload(ctx, b_desc);
    if (rc) return rc;
    rc = svxl_backward_batch(ctx, reinterpret_cast<const SlackPair*>(dev), n_pairs, *types, band, 1);
    if (rc) return rc;
    return launch_alt(ctx, reinterpret_cast<const AltPair*>(dev + b_sweep), AltPair{}, n_pairs, *types, band, 1, max_detour, max_slack, max_given);
}
