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
//                   Phase 2, per row, is the cut scan k_path_slack runs (svx_plane.h), here cut_scan<true>: it carries
//                   (cand, order key) instead of cand alone.  The per-wave band-offset table stays in LDS.
//                   Phase 3, for a measured row, are the two walks, on wave-uniform state.  Backward from u: a chain of
//                   dependent loads (table entry, back-pointer) per step, rows staged in the wave's LDS slots in walk order.
//                   Forward from v: the lanes take the moves, each tests its edge and w + Bk(s) == Bk(node), the first match in
//                   list order comes out of a ballot; rows staged from the other end of the same slots.  A walk that fails or
//                   grows past K writes nothing but the span.  Otherwise the lanes write the detour in document order, one
//                   16-byte store per row, and price each row from its cost cell.
//   k_given_regret  one thread per given row: ((F(u) + w) + Bk(v)) - total from three resident reads behind the validity checks.
// The descriptor of a pair (PlanePair), its geometry and the helpers that read a plane are svx_plane.h's, shared with
// svx_slack.hip: the backward sweep, k_row_alt and k_given_regret read the same records.  svx_row_alternatives lays out the
// post-processing scratch as [descriptors] uploaded, then per pair that is not skipped one Bk plane and one node table.
// A row that fails the range checks forms no address.  Both cost layouts are read: [T][A][B] (per-op) and [A][T][B] (fused
// pipeline); back-pointers come as packed bytes or as two int32 planes.  Plain C++, vector stores only.
#include "svx_plane.h"

namespace {

// Is node (x, y) -> (x + xo, y + yo) by move t an edge of E or E_b?  (x, y) is a band cell of diagonal a = x + y; -> the
// successor's diagonal and cell.
__device__ __forceinline__ bool alt_out_edge(const PlaneGeo& g, int x, int y, int t, int xo, int yo, int* av_out, int* bv_out) {
    const int a = x + y, av = a + xo + yo;
    if (av >= g.A + 2) return false;
    const int vx = x + xo, vy = y + yo;
    const int bv = vy - plane_bout(g.boff_in, av);
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
// dynamic LDS: per wave K staged rows (16 bytes) and K move indices
__host__ __device__ inline size_t al_smem_bytes(int K) { return (size_t)AL_WAVES * K * (4 * sizeof(int) + sizeof(int)); }

__global__ __launch_bounds__(AL_THREADS) void k_row_alt(const PlanePair* __restrict__ pairs, PlanePair one, int use_one, SvxTypes ty, int B,
                                                        int atb, int K, double max_slack) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int scnt[AL_WAVES][3];
    __shared__ int sbo[AL_WAVES][2 * MAXSTEP];   // per wave: b_offset_out of diagonals c - maxstep + 1 .. c + maxstep of its row
    const PlanePair P = use_one ? one : pairs[blockIdx.x];
    if (!P.edge) return;   // (uniform) a skipped pair: nothing of it is written
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    PlaneGeo g;
    const bool ok_pair = plane_geo(P, ty, B, atb, &g);
    int cnt;
    if (!plane_row_count(P, ok_pair, &cnt)) return;   // (uniform) a failed pair
    const int T = ty.n, NTt = ty.n + 2;
    const int Aout = g.A + 2;
    const long long xs = g.xs, ys = g.ys;
    const double inf = __builtin_inf();
    const double total = plane_total(g);
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
            const long long b = y - plane_bout(g.boff_in, (int)(x + y));
            if (b < 0 || b >= B) continue;
            gst(P.table + 2 * (size_t)(x + y), (int)b);
            gst(P.table + 2 * (size_t)(x + y) + 1, i);
        }
        __syncthreads();
    }
    int4* stage = reinterpret_cast<int4*>(smem) + (size_t)w * K;                               // this wave's K row slots
    int* stage_t = reinterpret_cast<int*>(smem + (size_t)AL_WAVES * K * sizeof(int4)) + (size_t)w * K;
    int n_edge = 0, n_written = 0, n_long = 0;   // lane 0 of the wave counts
    for (int r = w; r < cnt; r += AL_WAVES) {
        const uint4 rv = gld16(P.rows + 4 * (size_t)r);
        int t_own, bui, bvi;
        const bool valid = plane_is_edge(g, ty, rv, &t_own, &bui, &bvi);   // (uniform over the wave)
        double s = __builtin_nan("");
        bool has_edge = false;
        int e_ux = -1, e_xo = -1, e_uy = -1, e_yo = -1, e_t = 0;
        if (valid) {
            const int ci = (int)rv.x + (int)rv.z;
            int* bo = sbo[w];
            // ---- phase 2: the cut scan with the order key (diagonal of v, cell of v, move index)
            unsigned long long key;
            const double alt = cut_scan<true>(g, ty, bo, ci, bui, (int)rv.y, (int)rv.w, &key);
            s = alt - total;
            has_edge = alt < inf;
            if (has_edge) {
                e_t = (int)(key % (unsigned)NTt);
                const int it = (int)(key / (unsigned)NTt);
                const int dv = it / B + 1, bv = it - (dv - 1) * B;
                const int av = ci + dv;
                const int vy = bv + bo[av - (ci - ty.maxstep + 1)], vx = av - vy;
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
                const int b = y - plane_bout(g.boff_in, a);
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
                const int bpre = (y - py) - plane_bout(g.boff_in, a - px - py);
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
                    const int b = y - plane_bout(g.boff_in, a);
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
                                const double wgt = t < T ? (double)gld(g.costs + plane_cost_index(g, t, av - 2, bv)) : g.pen;
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
                            const int bv = row.z + row.w - plane_bout(g.boff_in, av);
                            const double cst = (double)gld(g.costs + plane_cost_index(g, tt, av - 2, bv));
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
    if (P.summary) plane_summary(scnt, P.summary, cnt, n_edge, n_written, n_long);
}

constexpr int GR_THREADS = 256;

__global__ __launch_bounds__(GR_THREADS) void k_given_regret(const PlanePair* __restrict__ pairs, PlanePair one, int use_one, SvxTypes ty, int B,
                                                             int atb) {
    const PlanePair P = use_one ? one : pairs[blockIdx.y];
    if (!P.edge || !P.given) return;   // (uniform)
    PlaneGeo g;
    if (!plane_geo(P, ty, B, atb, &g)) return;
    if (gld(P.given_info + 1) != 0) return;
    int cnt = gld(P.given_info);
    cnt = cnt < 0 ? 0 : (cnt > P.given_cap ? P.given_cap : cnt);
    const int i = blockIdx.x * GR_THREADS + threadIdx.x;
    if (i >= cnt) return;
    const uint4 rv = gld16(P.given + 4 * (size_t)i);
    int t, bu, bv;
    double out = __builtin_nan("");
    if (plane_is_edge(g, ty, rv, &t, &bu, &bv)) {
        const int c = (int)rv.x + (int)rv.z, av = c + (int)rv.y + (int)rv.w;
        const double wgt = t < ty.n ? (double)gld(g.costs + plane_cost_index(g, t, av - 2, bv)) : g.pen;
        out = ((gld(P.csum + ((size_t)c * B + bu)) + wgt) + gld(P.bsum + ((size_t)av * B + bv))) - plane_total(g);
    }
    gst(P.regret + i, out);
}

int launch_alt(svx_ctx* ctx, const PlanePair* dev, const PlanePair& one, int n, const SvxTypes& types, int B, int atb, int K, double max_slack,
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

void fill_outputs(PlanePair& r, const svx_alt& a) {
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
    PlanePair one{};
    one.costs = costs; one.boff_in = boff_in; one.csum = csum; one.bsum = const_cast<double*>(bsum); one.xp = xp; one.yp = yp;
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
    int max_given = 0;
    for (int p = 0; p < n_pairs; p++) {
        if (!alt[p].edge) continue;   // a skipped pair
        rc = check_alt(ctx, "svx_row_alternatives", alt[p]);
        if (rc) return rc;
        if (alt[p].given && alt[p].given_cap > max_given) max_given = alt[p].given_cap;
    }
    SvxLastCall lc;
    rc = svxl_last_call(ctx, "svx_row_alternatives", n_pairs, "row alternatives need", &lc);
    if (rc) return rc;
    // ---- scratch: [descriptors] uploaded, then per pair that is not skipped one Bk plane and one node table of
    //      (path capacity + 2) entries
    const size_t b_desc = up256((size_t)n_pairs * sizeof(PlanePair));
    size_t b_all = b_desc;
    for (int p = 0; p < n_pairs; p++)
        if (alt[p].edge) {
            const size_t diag = (size_t)lc.pair(p).lev[0].path_cap + 2;
            b_all += up256(diag * lc.band * sizeof(double)) + up256(diag * 2 * sizeof(int));
        }
    char *pin, *dev;
    rc = svxl_scratch_begin(ctx, "svx_row_alternatives", b_desc, b_all, &pin, &dev);
    if (rc) return rc;
    PlanePair* hp = reinterpret_cast<PlanePair*>(pin);
    size_t at = b_desc;
    for (int p = 0; p < n_pairs; p++) {
        PlanePair& r = hp[p];
        svxl_plane_pair(r, lc.pair(p), summary + 4 * (size_t)p);
        if (!alt[p].edge) continue;
        fill_outputs(r, alt[p]);
        const size_t diag = (size_t)lc.pair(p).lev[0].path_cap + 2;
        r.bsum = reinterpret_cast<double*>(dev + at);
        at += up256(diag * lc.band * sizeof(double));
        r.table = reinterpret_cast<int*>(dev + at);
        at += up256(diag * 2 * sizeof(int));
    }
    rc = svxl_scratch_upload(ctx, (size_t)n_pairs * sizeof(PlanePair));
    if (rc) return rc;
    const PlanePair* dp = reinterpret_cast<const PlanePair*>(dev);
    rc = svxl_backward_batch(ctx, dp, n_pairs, *lc.types, lc.band, 1);
    if (rc) return rc;
    return launch_alt(ctx, dp, PlanePair{}, n_pairs, *lc.types, lc.band, 1, max_detour, max_slack, max_given);
}
