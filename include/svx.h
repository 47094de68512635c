/*
 * svx.h -- C ABI of libsvx: the MI355X (gfx950) implementation of Speech-Vecalign's
 * segment-alignment hot path (svecalign/vecalign + svecalign/seg_align).
 *
 * The reference has exactly one native module on this path, svecalign/vecalign/dp_core.pyx
 * (Cython, 5 functions), called from svecalign/vecalign/dp_utils.py:vecalign().  Each entry
 * point below names the reference interface it replaces (paths relative to the reference
 * repository).  All array arguments are DEVICE pointers (HIP) unless marked "host"; the caller
 * owns every input and output buffer, the library owns only scratch inside the context.
 * Everything is asynchronous on the context's stream; call svx_synchronize() (or synchronise
 * the stream yourself) before reading results.  No function falls back to the CPU.
 *
 * Return value: 0 (SVX_OK) or an SVX_ERR_* code; svx_last_error() has the message.
 */
#ifndef SVX_H
#define SVX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svx_ctx svx_ctx;

enum svx_dtype { SVX_F32 = 0, SVX_F16 = 1, SVX_BF16 = 2 };

enum svx_status {
    SVX_OK = 0,
    SVX_ERR_ARG = 1,       /* bad shape / null pointer / unsupported size (asserts of dp_core.pyx:48-60,186-190,216) */
    SVX_ERR_OVERLAPS = 2,  /* "%d x overlaps requrested (via alignment_types), but vecs0 only has %d" dp_core.pyx:204-209 */
    SVX_ERR_HIP = 3,       /* a HIP runtime call failed */
    SVX_ERR_TRACEBACK = 4, /* 'traceback bug' dp_utils.py:123-124 / walked off the band */
    SVX_ERR_NOMEM = 5,     /* scratch allocation failed */
    SVX_ERR_EXTEND = 6,    /* 'asked to extend alignments but already bigger than requested' dp_utils.py:242-243 */
    SVX_ERR_PATH = 7,      /* search path is not a unit-step lattice path from (0,0) */
    SVX_ERR_BP = 8         /* 'got unknown value' dp_utils.py:166-167 */
};

#define SVX_MAX_LEVELS 16 /* pyramid depth limit (N*M <= max_size_full_dp^2 * 4^15) */
#define SVX_MAX_TYPES 128 /* alignment types per call (a=10 -> 45) */
#define SVX_MAX_DIM 2048  /* embedding dimension limit; d must be a multiple of 8 */

/* ---- context -------------------------------------------------------------------------- */
/* One context per (process, device): owns a HIP stream reference and a grow-only scratch arena.
 * Replaces nothing in the reference (its module is stateless); see SURVEY.md section 8(b). */
int svx_create(int device_id, svx_ctx **out);
int svx_destroy(svx_ctx *ctx);
/* Use an existing HIP stream (e.g. torch.cuda.current_stream().cuda_stream); NULL = default stream.
 * The context carries state from call to call -- the arena, the post-processing scratch, the costs, sums and tile plan
 * the "last call" entries read, the half-batches the pipeline holds back -- so a change of stream orders it: everything
 * the context did under the old binding (a held-back half included: svx_flush runs first, under the old binding, so the
 * stream a batch was launched on also sees its outputs complete) is ordered in front of the first work under the new
 * one, by an event the new stream waits for; the host does not wait.  The handle that is already bound returns at once.
 * A bound stream must stay alive until the context is bound elsewhere or destroyed.  What the caller still orders
 * themselves: their own buffers across their own streams (inputs written on another stream than the one the call is
 * bound to, outputs read on another one). */
int svx_set_stream(svx_ctx *ctx, void *hip_stream);
int svx_synchronize(svx_ctx *ctx);
/* Message of the last failure on this context (ctx may be NULL for svx_create failures). */
const char *svx_last_error(const svx_ctx *ctx);
const char *svx_version(void);
/* Bytes of device scratch currently held by the context: the arena and the post-processing scratch.
 * The post-processing scratch is what svx_alignment_rows, svx_concat_rows, svx_knn_search_groups, svx_time_prior,
 * svx_prior_width, svx_band_contact and svx_align_widen work in: one grow-only device buffer of the context's own, not in the arena -- the views of svx_debug_level stay valid --,
 * shared by these calls (they are ordered on the context's stream) and filled through two pinned staging buffers
 * taken in turn, like svx_align_batch's descriptors.  It grows with 25 % slack behind one stream synchronisation and is
 * released by svx_destroy. */
int64_t svx_scratch_bytes(const svx_ctx *ctx);

/* ---- the five native functions of dp_core.pyx (float32 buffers, like the reference) ----- */

/* make_dense_costs(vecs0, vecs1, norm0, norm1, offset0, offset1) -> costs      dp_core.pyx:36-77
 * vecs0 [k0][s0][d], vecs1 [k1][s1][d], norm0 [k0][s0], norm1 [k1][s1]; costs [s0][s1]. */
int svx_dense_costs(svx_ctx *ctx, const float *vecs0, int k0, int s0, const float *vecs1, int k1, int s1, int d,
                    const float *norm0, const float *norm1, int offset0, int offset1, float *costs);

/* dense_dp(alignment_cost, pen) -> (csum, bp)                                   dp_core.pyx:79-141
 * cost [s0][s1]; csum [s0+1][s1+1] float64 (may be NULL); bp [s0+1][s1+1] int32. */
int svx_dense_dp(svx_ctx *ctx, const float *cost, int s0, int s1, float pen, double *csum, int32_t *bp);

/* score_path(xx, yy, norm1, norm2, vecs1, vecs2, out)                            dp_core.pyx:143-161
 * xx,yy [n] int32; norm1 [rows1], norm2 [rows2]; vecs1 [rows1][d], vecs2 [rows2][d]; out [n]. */
int svx_score_path(svx_ctx *ctx, const int32_t *xx, const int32_t *yy, int64_t n, const float *norm1,
                   const float *norm2, const float *vecs1, int rows1, const float *vecs2, int rows2, int d, float *out);

/* make_sparse_costs(vecs0, vecs1, norms0, norms1, x_y_path, alignment_types, width_over2)
 *   -> (a_b_feats, b_offset)                                                    dp_core.pyx:165-267
 * path [A][2] int32 (device), types [T][2] int32 (HOST); costs [T][A][2W]; b_offset [A]. */
int svx_sparse_costs(svx_ctx *ctx, const float *vecs0, int k0, int xsize, const float *vecs1, int k1, int ysize,
                     int d, const float *norms0, const float *norms1, const int32_t *path, int A,
                     const int32_t *types_host, int T, int width_over2, float *costs, int32_t *b_offset);

/* sparse_dp(a_b_costs, b_offset_in, alignment_types, del_penalty, x_in_size, y_in_size)
 *   -> (a_b_csum, a_b_xp, a_b_yp, b_offset_out)                                 dp_core.pyx:269-404
 * costs [T][A][B]; csum [A+2][B] float64; xp, yp [A+2][B] int32; b_offset_out [A+2]. */
int svx_sparse_dp(svx_ctx *ctx, const float *costs, const int32_t *b_offset_in, int A, int B,
                  const int32_t *types_host, int T, double del_penalty, int x_in_size, int y_in_size,
                  double *csum, int32_t *xp, int32_t *yp, int32_t *b_offset_out);

/* ---- device versions of the numpy-side hot spots of dp_utils.py ------------------------ */

/* make_norm1(vecs): rows /= (||row|| + 1e-5), in place                          dp_utils.py:32-40 */
int svx_make_norm1(svx_ctx *ctx, float *vecs, int64_t rows, int d);

/* downsample_vectors(vecs) -> half [k][n/2][d]                                  dp_utils.py:362-378 */
int svx_downsample(svx_ctx *ctx, const float *vecs, int k, int n, int d, float *half);

/* compute_norms(vecs0, vecs1, num_samples) -> norms0 [k0][n0]                   dp_utils.py:326-359
 * The random row indices (one np.random.choice per overlap layer of vecs1, dp_utils.py:345-348)
 * are drawn by the caller: idx [k1][samples_per_overlap] int32, indices into vecs1's rows. */
int svx_compute_norms(svx_ctx *ctx, const float *vecs0, int k0, int n0, const float *vecs1, int k1, int n1, int d,
                      const int32_t *idx, int samples_per_overlap, float *norms0);

/* DeletionKnob(samp, 0, max(samp)).percentile_frac_to_del_penalty(frac)  dp_utils.py:43-79,312-313,321
 * scores [n] float32 -> *del_penalty (device double). */
int svx_del_penalty(svx_ctx *ctx, const float *scores, int64_t n, double frac, double *del_penalty);

/* The counting sort in front of the sampled scores (the samples of dp_utils.py:301-308, grouped by source row so that
 * the scoring pass reads every source row once).  kx, ky [kn] int32 sample rows on the two sides, clamped to [0, n) and
 * [0, m); kstart [n + 1]: kstart[x] = samples with a clamped source row below x, kstart[n] = kn; korder [kn]: the sample
 * ids 0..kn-1 grouped by clamped source row (the order inside one row is unspecified); kys [kn]: kys[p] = clamped
 * ky[korder[p]].  One workgroup; the same device code as svx_align_batch runs per (pair, level).  The scatter is staged
 * in LDS while (n + 1 + kn) * 4 bytes fit SVX_KNOB_SORT_STAGE_LDS and goes straight to memory otherwise; n is limited
 * by the LDS histogram ((n + 1) * 4 <= 150 KB), kn >= 0. */
#define SVX_KNOB_SORT_STAGE_LDS (150 * 1024)
int svx_knob_sort(svx_ctx *ctx, const int32_t *kx, const int32_t *ky, int kn, int n, int m, int32_t *korder,
                  int32_t *kys, int32_t *kstart);

/* dense_traceback(bp) -> alignments                                           dp_utils.py:146-174
 * bp [s0+1][s1+1]; align [s0+s1][4] int32 rows (x_start, x_len, y_start, y_len) in document
 * order; *count = number of rows, or -SVX_ERR_* on failure.
 * SVX_ERR_BP: a value other than 0 / 1 / 2 at a node of the walk, or a move that would leave the lattice (0 or 2 at
 * x == 0, 0 or 1 at y == 0).  The reference wraps around through a negative numpy index on such a move; that is not
 * mirrored.  No cell outside bp is ever addressed, whatever the table holds. */
int svx_dense_traceback(svx_ctx *ctx, const int32_t *bp, int s0, int s1, int32_t *align, int32_t *count);

/* sparse_traceback(csum, xp, yp, b_offset, xsize, ysize) -> (alignments, scores)  dp_utils.py:105-143
 * (+ process_scores :89-102).  align [xsize+ysize+2][4], scores [xsize+ysize+2] float64 (both are also
 * used as scratch by the walk: rows past *count are unspecified), *count as above.
 * csum, xp, yp [a_out][B], b_offset_out [a_out]; the tables may hold anything.  Rule: no cell outside
 * [0, a_out) x [0, B) is ever addressed.  A node (x, y) of the walk lives at [x + y][y - b_offset_out[x + y]]; the end
 * node (xsize, ysize), every node the back-pointers lead to and the origin (0, 0) -- whose csum the first score is taken
 * from -- must lie inside that rectangle, a back-pointer must be a step (px, py) >= 0, not (0, 0), with px <= x and
 * py <= y, and a_out >= 1, B >= 1, xsize, ysize >= 0: anything else is SVX_ERR_TRACEBACK ('traceback bug') and no score
 * is computed. */
int svx_sparse_traceback(svx_ctx *ctx, const double *csum, const int32_t *xp, const int32_t *yp,
                         const int32_t *b_offset_out, int a_out, int B, int xsize, int ysize, int32_t *align,
                         double *scores, int32_t *count);

/* upsample_alignment + extend_alignments + alignment_to_search_path  dp_utils.py:261-275,228-258,199-225
 * align [*n_align][4] rows of the coarser level (upsample != 0; size0/size1 = finer sizes) or of
 * the same level (upsample == 0, dp_utils.py:485-486).  path [size0+size1+4][2]; *path_len =
 * number of points or -SVX_ERR_*. */
int svx_search_path(svx_ctx *ctx, const int32_t *align, const int32_t *n_align, int upsample, int size0,
                    int size1, int32_t *path, int32_t *path_len);

/* make_doc_embedding's gather (svecalign/utils/embedding_utils.py:164-201): out[r][:] = table[idx[r]][:],
 * or zeros where idx[r] < 0 (PAD / ignored / missing candidate) or where the source row holds a NaN
 * (embedding_utils.py:183-190).  table [n_rows][d], out [n_out][d] of `dtype`; idx [n_out] int32 is the
 * flattened [overlaps][segments] row table (svx_candidate_table, or the Python mirror of make_overlap). */
int svx_gather_rows(svx_ctx *ctx, const void *table, int64_t n_rows, int d, int dtype, const int32_t *idx, int64_t n_out,
                    void *out);

/* ---- host-side helpers (HOST pointers, no device work, callable from any thread) ---------
 * What a driver needs besides the kernels to keep a GPU fed: the random row indices, the candidate index
 * table of a document and the text of an alignment file. */

/* np.random.RandomState.choice(n, size, replace=True) (the call of dp_utils.py:301-302,346), bit for bit: MT19937
 * 32-bit outputs with masked rejection.  key[624] / *pos are RandomState.get_state()[1] / [2], advanced in place. */
int svx_mt19937_choice(uint32_t *key, int32_t *pos, int64_t n, int64_t size, int32_t *out);

/* Lengths of svx_pair.norm_idx / svx_pair.knob_idx for a pair of these sizes. */
int64_t svx_norm_index_count(int n, int m, int k0, int k1, int max_size_full_dp, int num_samps_for_norm, int have_norms0,
                             int have_norms1);
int64_t svx_knob_index_count(int n, int m, int max_size_full_dp, int costs_sample_size);

/* All random row indices of one vecalign() call, in the reference's draw order (dp_utils.py:423-444 then
 * :450-456), laid out as svx_pair.norm_idx / knob_idx document.  have_norms0/1: the depth-0
 * normalisers of that side are given (dp_utils.py:428-444), so its draws are skipped. */
int svx_draw_indices(uint32_t *key, int32_t *pos, int n, int m, int k0, int k1, int max_size_full_dp, int costs_sample_size,
                     int num_samps_for_norm, int have_norms0, int have_norms1, int32_t *norm_idx, int32_t *knob_idx);

/* make_doc_embedding's table for speech segments (overlap_segments=True; embedding_utils.py:106-132, 164-201,
 * read_in_embeddings :93-99, load_ignore_index_file vecalign.py:187-195): table[o][i] = first line of `cat_path`
 * equal to "<start of segment i-o> <end of segment i>", or -1 (slot i < o, ignored from that overlap on, or no
 * such candidate).  table [max_overlaps][cap_lines] (NULL: only *n_lines / *n_candidates are returned).
 * ignore_path may be NULL.  err: optional message buffer. */
int svx_candidate_table(const char *seg_path, const char *cat_path, const char *ignore_path, int max_overlaps, int32_t *table,
                        int cap_lines, int32_t *n_lines, int64_t *n_candidates, char *err, int err_cap);

/* print_alignments (vecalign.py:174-184): "[x ids]:[y ids]:%.6f\n" per row (x_start, x_len, y_start, y_len), Python
 * list syntax; scores may be NULL ("[..]:[..]\n").  Returns the number of bytes needed; they are written to out
 * when they fit in cap. */
int64_t svx_format_alignments(const int32_t *rows, const double *scores, int64_t n, char *out, int64_t cap);

/* ---- global margin scoring of the mined alignments (next row after the alignment path) ---
 * svecalign/postprocess/score_align.py:118-161 (compute_sim_with_nonflat_idx) and the index side of
 * svecalign/postprocess/prep_index.py:153-185 (populate_index), for an exact ("Flat") database held in
 * HBM as unit-norm fp16 / bf16 rows -- the storage of the reference's faiss GPU index with gpu_type
 * "fp16-shard" (score_align.py:48-50). */

#define SVX_MARGIN_RATIO 0
#define SVX_MARGIN_DISTANCE 1
#define SVX_MARGIN_ABSOLUTE 2 /* score = similarity; accepted by svx_margin_candidates only */

/* populate_index: out[i] = rows[i] / |rows[i]| (faiss.normalize_L2, prep_index.py:180) stored as
 * out_dtype (SVX_F16 | SVX_BF16).  rows [n][d] of `dtype`; d a multiple of 32, at most 1024. */
int svx_unit_rows(svx_ctx *ctx, const void *rows, int dtype, int64_t n, int d, void *out, int out_dtype);

/* index.search(x, k) + the mean over the k neighbours (score_align.py:137-148), exact search:
 * mean_sim[i] = mean of the k largest <q_i / |q_i|, db_j>, j < n_db  (= (2 - mean L2^2) / 2 of the
 * reference for unit rows).  queries [n][d] of q_dtype are normalised on the fly (not in place) and
 * rounded to db_dtype for the MFMA, accumulation in fp32.  db [n_db][d] fp16 / bf16, n_db >= k,
 * 1 <= k <= 64. */
int svx_knn_mean_sim(svx_ctx *ctx, const void *queries, int q_dtype, int64_t n, const void *db, int db_dtype,
                     int64_t n_db, int d, int k, float *mean_sim);

/* The same search with the database arriving shard by shard (one rank's rows at a time on a ring of GPUs, or a
 * corpus larger than one allocation): topk [n][k] floats holds every query's k largest similarities so far, in no
 * particular order (-inf = none yet).  first != 0: the lists start empty; otherwise they continue from `topk`.
 * After the call `topk` covers the shards seen so far; mean_sim (nullable) receives their mean, which after the
 * last shard is svx_knn_mean_sim's result over the concatenated database (score_align.py:137-148, where the
 * reference searches one index holding the whole corpus).  n_db may be smaller than k, or 0. */
int svx_knn_topk_merge(svx_ctx *ctx, const void *queries, int q_dtype, int64_t n, const void *db, int db_dtype,
                       int64_t n_db, int d, int k, float *topk, int first, float *mean_sim);

/* index.search(x, k) itself (score_align.py:139-141), exact, with the neighbours' row ids: what svx_knn_mean_sim averages
 * and svx_knn_topk_merge keeps, plus which database rows they are.  sims [n][k] float32 = <q_i / |q_i|, db_j> as defined
 * above, ids [n][k] int64 = id_base + row number.  The k results of a query are the first k of the total order
 * (similarity descending, id ascending) over all rows seen, in that order: equal similarities come out by ascending id,
 * and of rows that tie at the k-th place the lowest ids are kept.  A query that has seen fewer than k rows carries
 * trailing (-inf, -1) entries.
 * first != 0: the lists start empty; otherwise they continue from (sims, ids) as an earlier call left them (database
 * arriving shard by shard; with distinct ids the result does not depend on the order of the shards).  n_db may be
 * smaller than k, or 0 (db may then be NULL).  d a multiple of 32, at most 1024; 1 <= k <= 64; rows and queries finite.
 * A separate kernel (csrc/svx_search.hip); asynchronous on the context's stream, no scratch. */
int svx_knn_search(svx_ctx *ctx, const void *queries, int q_dtype, int64_t n, const void *db, int db_dtype,
                   int64_t n_db, int d, int k, int64_t id_base, float *sims, int64_t *ids, int first);

/* The same search over GROUPS: query rows [q_off[g], q_off[g+1]) search database rows [db_off[g], db_off[g+1]) and nothing
 * else, for g < n_groups, in one launch (csrc/svx_groupsearch.hip) -- the two documents of every parallel pair of a corpus
 * (Local Mining), or any "neighbours from the same document only" normalisation.  q_off, db_off: HOST arrays of
 * n_groups + 1 entries that start at 0 and never decrease; they are copied before the call returns and may be freed then.
 * queries [n][d] with n = q_off[n_groups]; db holds at least db_off[n_groups] rows.
 * sims [n][k] float32, ids [n][k] int64 = GLOBAL database row numbers (db_off[g] + the row inside the group).  For the rows
 * of group g the result is, bit for bit in values and ids, what
 *   svx_knn_search(queries + q_off[g] * d, n_g, db + db_off[g] * d, N_g, d, k, id_base = db_off[g], ..., first = 1)
 * writes on the same build: the same total order, the same tie rule, trailing (-inf, -1) entries where the group has fewer
 * than k database rows.  Empty groups are legal on either side, and so is n_groups = 0.  There is no continuation mode.
 * d, k, the dtypes and finite rows: the rules of svx_knn_search.  A violation, a null argument, an offset array that does not
 * start at 0 or decreases, a negative n_groups, or offsets that need 2^31 or more workgroups (a group of n_g queries takes
 * ceil(n_g / 64)) return SVX_ERR_ARG with text and queue nothing.  Asynchronous on the context's stream, no host
 * synchronisation.  Scratch (the two offset arrays and 8 bytes per workgroup) is the context's post-processing scratch
 * (svx_scratch_bytes). */
int svx_knn_search_groups(svx_ctx *ctx, const void *queries, int q_dtype, const void *db, int db_dtype, int d, int k,
                          const int64_t *q_off, const int64_t *db_off, int n_groups, float *sims, int64_t *ids);

/* score_align.py:151-160: scores[i] = <x_i/|x_i|, y_i/|y_i|> / ((mean_xy[i] + mean_yx[i]) / 2)
 * (SVX_MARGIN_RATIO) or minus it (SVX_MARGIN_DISTANCE).  x, y [n][d] of `dtype`. */
int svx_margin_scores(svx_ctx *ctx, const void *x, const void *y, int dtype, int64_t n, int d, const float *mean_xy,
                      const float *mean_yx, int margin, float *scores);

/* ---- margin-based mining over two Flat databases (csrc/svx_mine.hip) ----------------------
 * Artetxe & Schwenk, https://aclanthology.org/P19-1309 sec. 3, as LASER's mine_bitexts.py runs it: every row of one
 * side is searched in the other (svx_knn_search), its k neighbours are re-scored with the margin and the best one is
 * taken.  The operation order below is part of the contract: the results are defined bit for bit. */

/* mean[i] = (((s[i][0] + s[i][1]) + ...) + s[i][k-1]) / (float)k, fp32, j ascending: the mean similarity of a
 * query to its k neighbours from the lists svx_knn_search left (sims [n][k]).  -inf entries propagate.  1 <= k <= 64.
 * Asynchronous on the context's stream, no scratch. */
int svx_knn_list_means(svx_ctx *ctx, const float *sims, int64_t n, int k, float *mean);

/* Candidate scoring of margin-based mining (P19-1309 sec. 3; LASER score_candidates + argmax):
 *   b = (mean_q[i] + mean_db[ids[i][j] - id_base]) * 0.5f
 *   scores[i][j] = sims[i][j] / b   (SVX_MARGIN_RATIO)
 *                | sims[i][j] - b   (SVX_MARGIN_DISTANCE)
 *                | sims[i][j]       (SVX_MARGIN_ABSOLUTE; mean_q and mean_db are not read and may be NULL)
 * each operation rounded to fp32 on its own, the division correctly rounded.  sims, ids [n][k] as svx_knn_search left
 * them; mean_q [n], mean_db [n_db] = svx_knn_list_means of the lists of the two directions.
 * An id of -1, or one outside [id_base, id_base + n_db), is never dereferenced and scores -inf.
 * best starts as (-inf, -1); candidate j replaces it when scores[i][j] > best_score, j ascending.
 * So ties go to the lowest j (= higher similarity, then lower id), and NaN / -inf never win.
 * best_id [n] int64 (the id as it stands in ids), best_score [n]; scores [n][k] may be NULL.  1 <= k <= 64.
 * Asynchronous on the context's stream, no scratch. */
int svx_margin_candidates(svx_ctx *ctx, const float *sims, const int64_t *ids, int64_t n, int k, const float *mean_q,
                          const float *mean_db, int64_t n_db, int64_t id_base, int margin, float *scores, int64_t *best_id,
                          float *best_score);

/* The sequential greedy pass of LASER's `max` retrieval (mine_bitexts.py: seen_src / seen_trg).  HOST pointers, no device
 * work, callable from any thread.  order[p], p < n_cand: candidate indices in output order; src[], tgt[] [n_cand]: their
 * rows, src[c] < n_src, tgt[c] < n_tgt.  Keeps candidate c = order[p] iff neither src[c] nor tgt[c] was kept before;
 * writes the kept c's to out [n_cand] in order.  Returns the count, or -SVX_ERR_ARG (null pointer, negative count, an
 * index out of range). */
int64_t svx_mine_greedy(const int64_t *order, int64_t n_cand, const int64_t *src, const int64_t *tgt, int64_t n_src,
                        int64_t n_tgt, int64_t *out);

/* ---- the whole of dp_utils.vecalign() for a batch of document pairs -------------------- */

typedef struct svx_align_params {
    int32_t dtype;            /* svx_dtype of vecs0/vecs1 */
    int32_t d;                /* embedding dimension */
    int32_t n_types;          /* final_alignment_types, in the order of vecalign.py:154-162 */
    int32_t types[2 * SVX_MAX_TYPES];
    int32_t width_over2;      /* dp_utils.py:391-393: values < 3 are raised to 3 */
    int32_t max_size_full_dp; /* dp_utils.py:403-408 */
    int32_t costs_sample_size;
    int32_t num_samps_for_norm;
    double del_percentile_frac;
    int32_t search_mode;      /* SVX_SEARCH_* (0 = the reference's coarse-to-fine recursion) */
    int32_t reserved0;
} svx_align_params;

/* search_mode.  COARSE_TO_FINE: dp_utils.vecalign() as the reference runs it.  STRAIGHT: the same recurrence
 * (make_sparse_costs + sparse_dp + sparse_traceback, final alignment types, depth-0 normalisers and deletion
 * penalty, same random draws as a vecalign() call without pyramid levels) in a band of half-width width_over2
 * around the straight line from (0,0) to (N,M) (append_slant, dp_utils.py:177-196) instead of around an up-sampled
 * coarse alignment: Sakoe-Chiba search (BASELINE configs[3]), and with width_over2 > max(N, M) every cell of
 * the lattice (what vecalign() evaluates with max_size_full_dp = infinity; SURVEY.md 8a, Modes B / C).  Bands wider
 * than 64 cells run as a wavefront of 32 x 32 tiles over all CUs, the costs of a tile computed on the matrix cores
 * (no [T][A][B] cost tensor in memory).  Every band width takes the type sets COARSE_TO_FINE takes (<= 128 types,
 * sizes <= 100): up to 16 types on up to 12 overlap layers with steps <= 8 keep a tile's costs in LDS; larger sets
 * stream them through a per-CU plane buffer of ceil(T/8)*8 x 4 KB (counted in svx_scratch_bytes). */
#define SVX_SEARCH_COARSE_TO_FINE 0
#define SVX_SEARCH_STRAIGHT 1

typedef struct svx_pair {
    const void *vecs0, *vecs1; /* [k0][n][d], [k1][m][d] of params.dtype; NOT modified */
    int32_t n, m, k0, k1;
    /* Random row indices in the reference's draw order.  norm_idx: for each depth
     * 0..L: [k1][S1] indices into side 1 (used for n0), then [k0][S0] into side 0 (used for n1),
     * S1 = ceil(num_samps/k1), S0 = ceil(num_samps/k0); a side whose norms are overridden at depth 0
     * contributes no indices at depth 0.  knob_idx: for each depth: x[c] then y[c], c =
     * svx_knob_count(n_l, m_l, costs_sample_size) (full enumeration when n_l*m_l < sample size). */
    const int32_t *norm_idx;
    const int32_t *knob_idx;
    const float *norms0, *norms1; /* optional depth-0 overrides [k0][n], [k1][m] (dp_utils.py:428-444) */
    /* outputs */
    int32_t *align;   /* [n+m+2][4] rows (x_start, x_len, y_start, y_len) */
    double *scores;   /* [n+m+2] */
    int32_t *info;    /* [2]: info[0] = number of alignments, info[1] = 0 or SVX_ERR_* */
    double *del_pen;  /* optional [L+1]: deletion penalty per depth */
} svx_pair;

/* Number of halvings dp_utils.py:403-408 performs (max_depth). */
int svx_num_levels(int n, int m, int max_size_full_dp);
/* Length of each of the two knob index arrays at a level of sizes (n_l, m_l): dp_utils.py:286-302. */
int64_t svx_knob_count(int n_l, int m_l, int costs_sample_size);

/* vecalign(vecs0, vecs1, final_alignment_types, del_percentile_frac, width_over2,
 *          max_size_full_dp, costs_sample_size, num_samps_for_norm, norms0, norms1) -> stack
 *                                                                              dp_utils.py:381-537
 * for n_pairs independent document pairs (pairs: HOST array).  Produces stack[0]
 * ['final_alignments'] and ['alignment_scores'] per pair. */
int svx_align_batch(svx_ctx *ctx, const svx_align_params *params, const svx_pair *pairs, int n_pairs);

/* ---- margin from candidate rows: the alignment rows of a batch -> the inputs of the margin half -------------
 * svecalign/postprocess/embed_align.py embeds the audio span of every mined alignment again, from the start of its first
 * segment to the end of its last (svecalign/utils/file_utils.py:158-163).  For an alignment of at most k0 x k1 segments
 * that span is the line "<start> <end>" of the candidate file and its embedding is the candidate row
 * vecs0[x_len-1][x_start+x_len-1] the DP has just read, so the two row matrices svx_unit_rows / svx_knn_mean_sim /
 * svx_margin_scores expect are gathered on the device, with no encoder and no host round trip (csrc/svx_alignrows.hip).
 *
 * Read per pair (pairs: HOST array): vecs0, vecs1, n, m, k0, k1, align, scores, info -- as an earlier svx_align_batch on this
 * context's stream left them, or as any caller filled them; nothing else of svx_pair is read.  align and scores hold
 * n + m + 2 rows; rows past that are never read.  vecs0 / vecs1 and the row buffers below are 16-byte aligned.
 *
 * Row r of pair p is KEPT iff  info[1] == 0 and 0 <= r < info[0];  1 <= x_len <= k0 and 1 <= y_len <= k1 (deletions and
 * anything wider than a candidate go);  0 <= x_start, x_start + x_len <= n, 0 <= y_start, y_start + y_len <= m;  and
 * scores[r] <= max_score as a plain double comparison (NaN fails; max_score = +inf keeps every non-deletion).  A row that
 * is not kept is never used to form an address: a failed pair may hold garbage.
 *
 * Kept rows are numbered j = 0, 1, ... in (pair ascending, r ascending) order.  At j:
 *   x_rows[j] = vecs0[x_len-1][x_start+x_len-1][:], y_rows[j] = vecs1[y_len-1][y_start+y_len-1][:], copied bit for bit
 *               ([cap][d] of `dtype`);
 *   src[j]    = (p, r)                                                   ([cap][2] int32);
 *   x_unit[j], y_unit[j] = bit for bit what svx_unit_rows(..., unit_dtype) writes for that row, a zero row stays zero
 *               ([cap][d] fp16 | bf16; both pointers or neither).
 * *count (device, [1]) = the number of kept rows, also when it exceeds cap; only j < cap is written and nothing else of
 * the output buffers is touched.  cap = 0 or n_pairs = 0 is legal, the buffers may then be NULL.
 * d: with unit rows a multiple of 32, at most 1024 (the margin entries' rule); without them a multiple of 8, at most
 * SVX_MAX_DIM.  A violation, a null argument or an unknown dtype returns SVX_ERR_ARG with text and queues nothing.
 * Asynchronous on the context's stream, no host synchronisation; it calls svx_flush first, so with the software pipeline
 * on it still sees complete outputs.  Scratch (a copy of the descriptors, a chunk table, per-chunk counts and offsets)
 * is the context's post-processing scratch (svx_scratch_bytes). */
int svx_alignment_rows(svx_ctx *ctx, int dtype, int d, const svx_pair *pairs, int n_pairs, double max_score, int64_t cap,
                       void *x_rows, void *y_rows, void *x_unit, void *y_unit, int unit_dtype, int32_t *src, int64_t *count);

/* ---- margin rows for concatenated alignments: the post-filter chain on the device ---------------------------
 * Between alignment and margin scoring the reference runs filter_by_cost --max_cost, concat_aligns and filter_by_dur
 * (example/voxpopuli/run.sh steps 6.1, 6.3, 6.4; the audio-based filter_untrans_align of 6.2 is NOT part of this entry).
 * concat_aligns only joins alignments that are directly connected on both sides, so a joined alignment is a contiguous run
 * of segments on each side, and while that run is at most k0 x k1 segments its embedding is the candidate row
 * vecs0[x_len-1][x_start+x_len-1] as for svx_alignment_rows.  svx_concat_rows applies the chain to the alignment rows of a
 * batch and gathers the rows of every output that fits (csrc/svx_alignrows.hip).
 *
 * pairs: as svx_alignment_rows reads them.  frames (HOST array of n_pairs): per pair the device arrays [n][2] and [m][2] of
 * (start, end) sample positions of the segments (svecalign/utils/file_utils.py read_segments); may be NULL only when
 * max_num_align == 1 and min_frames <= 0, and is then not read.
 *
 * BASE ROWS (filter_by_cost.py:39-87).  Row r of pair p is a base row iff  info[1] == 0 and 0 <= r < min(info[0], n+m+2);
 * x_len >= 1 and y_len >= 1;  0 <= x_start, x_start + x_len <= n, 0 <= y_start, y_start + y_len <= m;  scores[r] <=
 * max_score as a plain double comparison (NaN fails).  There is no width limit.  A row that is not a base row is never used
 * to form an address.  c_0 < c_1 < ... are the base rows of the pair.
 *
 * JOINING (concat_aligns.py:56-110).  For every i the output e = 0 is c_i alone; outputs e = 1 .. max_num_align-1 follow
 * while c_{i+e} exists IN THE SAME PAIR and passes, against the run so far (first row f = c_i, last row l = c_{i+e-1}, with
 * xs/xl/ys/yl the row's fields, xend = xs + xl - 1, F0 / F1 the frames of the two sides), in this order:
 *   (double)(F0[xend(nx)][1] - F0[xs(f)][0]) / sample_rate <= max_dur;  if both_sides, the same with F1 / y;
 *   xs(nx) == xs(l) + xl(l) and ys(nx) == ys(l) + yl(l);
 *   (double)(F0[xs(nx)][0] - F0[xend(l)][1]) / sample_rate <= max_sil, and the same with F1 / y.
 * The first failure ends the run of that i.  Differences are taken in int64, divisions in double.
 * The span of (i, e): x_start = xs(c_i), x_len = xs(c_{i+e}) + xl(c_{i+e}) - xs(c_i); likewise y.
 *
 * DURATION FILTER (filter_by_dur.py:62-63), when min_frames > 0: an output is dropped unless
 * min_frames <= F0[x_start+x_len-1][1] - F0[x_start][0] and the same on the target side.
 *
 * FIT.  An output that passes is numbered and gathered only if x_len <= k0 and y_len <= k1; otherwise it is counted in
 * counts[1] ("wide": the reference embeds it with the encoder) and nothing is written for it.
 *
 * Fitting outputs are numbered j = 0, 1, ... in (pair, i, e) ascending order, the line order of the reference's files.  At j:
 *   x_rows[j], y_rows[j], x_unit[j], y_unit[j]: what svx_alignment_rows defines for a row with that span;
 *   meta[j] = (p, c_i, c_{i+e}, e + 1, x_start, x_len, y_start, y_len)              ([cap][8] int32).
 * counts (device, [2]): counts[0] = the number of fitting outputs, also when it exceeds cap, counts[1] = the wide ones.  Only
 * j < cap is written and nothing else of the output buffers is touched.  cap = 0 or n_pairs = 0 is legal.
 * d, alignment, dtypes, null arguments: the rules of svx_alignment_rows; max_num_align outside 1 .. SVX_CONCAT_MAX, a
 * non-positive sample_rate or NaN limits where frames are needed, and missing frames return SVX_ERR_ARG with text and queue
 * nothing.  Asynchronous on the context's stream, no host synchronisation, svx_flush first.  Seven launches (count, scan
 * and write of the base rows; count, scan and write of the outputs; gather) with no host round trip in between.  Scratch
 * is the context's post-processing scratch (svx_scratch_bytes; here also the compacted base rows, 24 bytes per alignment
 * row, and 16 bytes per output up to cap). */
#define SVX_CONCAT_MAX 8
typedef struct svx_frames { const int32_t *src, *tgt; } svx_frames;
typedef struct svx_concat_params {
    double  max_score;        /* cost filter, as svx_alignment_rows' max_score */
    int32_t max_num_align;    /* 1 .. SVX_CONCAT_MAX; 1 = no joining */
    int32_t sample_rate;      /* > 0 (16000) */
    double  max_sil, max_dur; /* seconds */
    int32_t both_sides;       /* apply max_dur to the target span too */
    int32_t pad;
    int64_t min_frames;       /* duration filter; <= 0 keeps everything */
} svx_concat_params;
int svx_concat_rows(svx_ctx *ctx, int dtype, int d, const svx_pair *pairs, const svx_frames *frames, int n_pairs,
                    const svx_concat_params *params, int64_t cap, void *x_rows, void *y_rows, void *x_unit, void *y_unit,
                    int unit_dtype, int32_t *meta, int64_t *counts);

/* ---- band search around a prior alignment (csrc/svx_prior.hip) ---------------------------------------------
 * At max_depth == 0 dp_utils.vecalign() refines around the same-level alignment it has just made (dp_utils.py:485-489:
 * alignment_to_search_path, make_sparse_costs, sparse_dp, sparse_traceback).  svx_align_around is that step started from
 * an alignment the CALLER supplies: an earlier run, a cheap 1-1 pass, or the segments' timestamps (svx_time_prior).
 *
 * It is svx_align_batch in SVX_SEARCH_STRAIGHT -- the same random draws (depth 0 only, the index layout
 * svx_norm_index_count / svx_knob_index_count give for max_size_full_dp = 1 << 30), normalisers, deletion penalty, final
 * types, outputs, svx_debug_level view, stage timers and software pipeline -- except that the level-0 alignment the search
 * path is made from is the prior instead of the one block covering both documents.  params->search_mode must be
 * SVX_SEARCH_AROUND (svx_align_batch keeps rejecting that value).  priors: HOST array parallel to pairs; typically another
 * call's svx_pair.align / .info with cap = n + m + 2, with no host round trip in between, or what svx_time_prior wrote.
 * The call flushes the software pipeline first (svx_flush), so a prior that an earlier pipelined call on this context
 * produces is complete when it is read; prior buffers must stay alive until svx_flush, like every input.
 *
 * The prior is taken in on the device, one workgroup per pair, with no host synchronisation, in this order:
 *   info[1] != 0                                  the pair fails with that code;
 *   count = info[0] outside [0, cap]              SVX_ERR_ARG;
 *   a row with a negative length or both 0        SVX_ERR_PATH;
 *   sum of x_len > n or sum of y_len > m          SVX_ERR_EXTEND;
 *   sums smaller than n / m                       one final row (n - sum x_len, m - sum y_len) is appended, so count = 0 is
 *                                                 exactly the straight search; a remainder with one side 0 is a deletion
 *                                                 run, which alignment_to_search_path walks as a slant.
 * Only the two lengths of a row are read.  A pair that fails gets the code in its info[1] (info[0] = 0) and the ingest
 * writes nothing else for it; it never forms an address from its rows and does not disturb the other pairs of the batch.
 * Returned at once with SVX_ERR_ARG and text, nothing queued: a null argument, cap < 0, a prior buffer that is the pair's
 * own align / info output (in-place refinement is not supported), a band (2 * width_over2) above 64 cells under
 * SVX_SEARCH_AROUND (wider bands are SVX_SEARCH_AROUND_WIDE's).
 *
 * SVX_SEARCH_AROUND_WIDE is SVX_SEARCH_AROUND without the limit on the band: the same prior, ingest rules, draws,
 * normalisers, penalty, outputs and flush-first behaviour (svx_align_batch rejects this value too).  A band of at most 64
 * cells runs the very kernels of SVX_SEARCH_AROUND: outputs and svx_debug_level views are equal bit for bit.  A wider band
 * runs the tile sweep of SVX_SEARCH_STRAIGHT around the prior's search path: every type set the wide straight sweep takes
 * (SVX_ERR_ARG with the same text for a set no tile shape takes), never pipelined, and a svx_level_view like the wide
 * straight sweep's (no a_b_costs; csum and back-pointers on lattice nodes only).  Time and scratch of the sweep grow with
 * the band, not with n x m: a prior that follows the drift needs a band as wide as its blocks (svx_prior_width). */
#define SVX_SEARCH_AROUND 2
#define SVX_SEARCH_AROUND_WIDE 3
typedef struct svx_prior {
    const int32_t *rows;   /* device [cap][4] rows (x_start, x_len, y_start, y_len); only the two lengths are read */
    const int32_t *info;   /* device [2]: info[0] = number of rows, info[1] = 0 or SVX_ERR_* (layout of svx_pair.info) */
    int32_t cap, pad;
} svx_prior;
int svx_align_around(svx_ctx *ctx, const svx_align_params *params, const svx_pair *pairs,
                     const svx_prior *priors, int n_pairs);

/* A prior from the segments' timestamps: parallel speech is time-synchronous up to a lag while segment indices drift apart
 * wherever one side has a stretch the other lacks.  pairs: n and m are read; frames (HOST array of n_pairs) as
 * svx_concat_rows reads it, F0 = frames[p].src [n][2], F1 = frames[p].tgt [m][2]; out (HOST array of n_pairs): rows / info
 * are WRITTEN (device), cap >= n + m.
 *   window of source segment i = floor(F0[i][0] / window), of target segment j = floor(max(F1[j][0] - lag, 0) / window),
 *   in int64; window > 0, lag may be negative (|lag| < 2^62).
 * One row per window value present on either side, windows ascending: x_start = source segments in earlier windows,
 * x_len = source segments in this window, likewise y; info = (number of rows, 0).  The lengths always sum to n and m.
 * Segment starts that decrease on a side give info = (0, SVX_ERR_PATH) and no rows.
 * A null argument, window <= 0, negative sizes or cap < n + m return SVX_ERR_ARG with text and queue nothing.
 * Asynchronous on the context's stream, no host synchronisation.  Scratch (the descriptors and 4 bytes per segment + 8 per
 * pair) is the context's post-processing scratch (svx_scratch_bytes). */
int svx_time_prior(svx_ctx *ctx, const svx_pair *pairs, const svx_frames *frames, int n_pairs,
                   int64_t window, int64_t lag, const svx_prior *out);

/* The width_over2 from which the band around a prior holds every node of every block of that prior.  pairs (n and m are
 * read) and priors: HOST arrays as svx_align_around takes them; width: DEVICE int32 [n_pairs], written.  One workgroup per
 * pair applies the ingest rules of svx_align_around in their order and writes
 *   1 + max over the ingested rows, the appended remainder row included, of min(x_len, y_len), and never less than 3
 *   (the width svx_align_around raises smaller ones to);   0 for a prior the ingest would fail.
 * Covering property: with that width_over2 every lattice node (x, y) of every ingested block -- x and y inside the
 * block's two spans, ends included -- satisfies 0 <= y - new_b_offset[x + y] < 2 * width_over2, so the search can reach
 * every alignment that stays inside the prior's blocks.  This rests on a check on the CPU oracle (tests/
 * test_around_wide_cpu.py: block priors of 1 .. 15 blocks, deletion rows, a remainder), not on a proof; a deletion row
 * counts with min = 0 because alignment_to_search_path merges deletion runs into the slant that follows.
 * A null argument, negative sizes or cap, or a null prior buffer return SVX_ERR_ARG with text and queue nothing.
 * Asynchronous on the context's stream, no host synchronisation.  Scratch: the descriptors only, in the context's
 * post-processing scratch (svx_scratch_bytes). */
int svx_prior_width(svx_ctx *ctx, const svx_pair *pairs, const svx_prior *priors, int n_pairs, int32_t *width);

/* ---- band-edge contact and band doubling (csrc/svx_contact.hip) ------------------------------------------------
 * Every search here is a banded DP: 2 * width_over2 cells per diagonal around a search path that something else chose (the
 * up-sampled coarser alignment, the straight line, the caller's prior).  Where the best alignment wants to leave that band
 * the DP returns the best path INSIDE it: a search error.  svx_band_contact reports the classical symptom -- nodes of the
 * returned path on the outermost cells of their diagonals -- and svx_align_widen applies the classical remedy, band
 * doubling: search again around the path just found, in twice the band, until the path clears the edge.  Widening removes
 * search errors, not model errors: on noisy data a lower-cost path need not hold more of the true pairs,
 * so the report is always available and the re-search is the caller's choice.
 *
 * svx_band_contact covers the pairs of the LAST svx_align_batch / svx_align_around call on the context -- the pairs
 * svx_debug_level addresses, both halves of a pipelined call -- at pyramid level `level` of that call.  It calls svx_flush
 * first and is asynchronous on the context's stream, with no host synchronisation.  It reads integers only: the level's
 * alignment rows and their count, its new_b_offset, the level's sizes, the band B = 2 * width_over2 of that call and the
 * pair's info.
 *   Nodes of a level: (0, 0) and, for every alignment row in order, (x_start + x_len, y_start + y_len).
 *   For a node (x, y): a = x + y, o = new_b_offset[a], b = y - o.  The cell just outside the band is (a - (o - 1), o - 1) on
 *   the low side and (a - (o + B), o + B) on the high side; a side is REAL iff that cell is a lattice node of the level,
 *   0 <= x' <= size0 and 0 <= y' <= size1.  The node's clearance is the minimum over its real sides of b (low) and
 *   B - 1 - b (high), INT32_MAX when neither side is real: document borders never count, and in a band that covers the
 *   whole lattice nothing touches.  A node TOUCHES iff its clearance is <= guard.
 * out (device, [n_pairs][4] int32, 16-byte aligned): out[p] = (touch, run, clearance, nodes) = the number of touching
 * nodes, the longest run of consecutive touching nodes, the minimum clearance over all nodes, the node count; or
 * (-1, -1, -1, -1) for a pair whose info[1] != 0 and for a level the pair did not refine (level > L, and the dense coarsest
 * level when L > 0).
 * A null argument, level < 0, guard < 0 or no earlier (successful) call return SVX_ERR_ARG with text and queue nothing.
 * One workgroup per pair; scratch (the descriptors) is the context's post-processing scratch (svx_scratch_bytes). */
int svx_band_contact(svx_ctx *ctx, int level, int guard, int32_t *out);

/* Band doubling.  SYNCHRONOUS: every round ends with a read-back of the contact report, and the entry returns with all
 * outputs complete.
 *   Round 0 is exactly svx_align_batch(params, pairs) when priors == NULL (SVX_SEARCH_COARSE_TO_FINE or
 *   SVX_SEARCH_STRAIGHT) or svx_align_around(params, pairs, priors) otherwise, followed by svx_band_contact(0, guard).
 *   Round r >= 1: the pairs that touch (touch > 0, info[1] == 0) are searched again in ONE svx_align_around call in
 *   SVX_SEARCH_AROUND_WIDE with width_over2 = min(W0 * 2^r, max_width_over2), W0 = params->width_over2 raised to 3.  The
 *   prior of a pair is its current result, which the library first copies into the post-processing scratch (rows up to
 *   the count read on the device, and info), since a prior may not be the pair's own output; the results go into the
 *   pair's own align / scores / info (and del_pen).  Every other field of svx_pair is passed unchanged, the norm_idx /
 *   knob_idx pointers included: the depth-0 draws are the leading entries of both arrays in either layout, so every round
 *   uses the depth-0 normaliser and penalty draws of round 0.  svx_band_contact(0, guard) follows.
 *   It stops when nothing touches, after max_rounds rounds, or when the width has reached max_width_over2.
 * report (HOST, [n_pairs][4]): (rounds run for this pair, its final width_over2, touch after round 0, touch after its last
 * round); touch is -1 for a failed pair.  max_rounds = 0 is round 0 plus the report.
 * Outputs and report equal, bit for bit, those of that sequence of public calls.  A non-zero return of an internal call
 * is returned as is.  Afterwards svx_debug_level, svx_band_contact and the stage timers see the LAST internal call: with
 * r >= 1 that is the batch of the pairs searched again in the last round, in their order.
 * A null argument, a negative field of wp, or max_width_over2 < W0 return SVX_ERR_ARG with text and queue nothing.
 * svx_pair, svx_align_params and svx_prior are what the other entries take. */
typedef struct svx_widen_params { int32_t guard, max_width_over2, max_rounds, reserved; } svx_widen_params;
int svx_align_widen(svx_ctx *ctx, const svx_align_params *params, const svx_pair *pairs, const svx_prior *priors /* nullable */,
                    int n_pairs, const svx_widen_params *wp, int32_t *report /* HOST [n_pairs][4] */);

/* ---- given alignments at the aligner's prices: search error or model error (csrc/svx_given.hip) ------------------
 * svx_band_contact reports a symptom.  The test itself (search-error analysis) prices a path the caller believes in --
 * gold, the timestamps' path, an earlier run, another tool's output -- with the normalisers and the deletion penalty the
 * DP used, and compares its total with the total of the path the DP returned: a given path that is cheaper was missed by
 * the search; one that is dearer is not what the model prefers, and no band width will find it.
 *
 * svx_score_alignments covers the pairs of the LAST svx_align_batch / svx_align_around call on the context, exactly as
 * svx_band_contact does: both halves of a pipelined call, in the pair order of svx_debug_level; n_pairs must equal that
 * call's pair count.  It calls svx_flush first and is asynchronous on the context's stream, with no host synchronisation.
 * It reads level 0 of that call only: the caller's vectors, their dtype and d, k0 and k1, the level's n0 / n1, the inverse
 * row norms 1/(||row|| + 1e-5) of the level-0 pass (the call's arena holds them until the next call: they are read, not
 * formed again), the deletion penalty, new_b_offset, the search path's length, the band B = 2 * width_over2 and the call's
 * type set.
 * given (HOST [n_pairs]): rows / info as svx_pair.align / info and svx_prior.rows / info, 16-byte aligned, read only; they
 * may be the pair's own align / info output, which is how a caller gets the total of the found path.  rows == NULL skips
 * the pair: nothing of it is written.
 *
 * Row r < info[0], with p = x_len and q = y_len, n and m the sizes of the pair:
 *   DELETION  exactly one of p, q is 1 and the other is 0, 0 <= x_start, x_start + p <= n, 0 <= y_start, y_start + q <= m.
 *             Cost: the penalty.  scores[r] = 0.0 (process_scores, dp_utils.py:94-96).
 *   PRICED    1 <= p <= k0, 1 <= q <= k1, in range as above.  With xe = x_start + p - 1, ye = y_start + q - 1:
 *               dot = <V0[p-1][xe], V1[q-1][ye]> in fp32 x inv0[p-1][xe] x inv1[q-1][ye]
 *               c   = fp32( 2 p q (1 - dot) / (1e-6 + (double) n0[p-1][xe] + (double) n1[q-1][ye]) )
 *             -- the expression of the level-0 band-cost kernel.  scores[r] = max(c, 0) / (p q) as a double.
 *             The row is OFF_TYPE as well when (p, q) is not in the call's type set.
 *   WIDE      p, q >= 1 and in range, but p > k0 or q > k1: there is no candidate row.  scores[r] = NaN.
 *   INVALID   anything else: a negative field, out of range, p = q = 0, a deletion of more than one segment.
 *             scores[r] = NaN.
 * A WIDE or INVALID row is never used to form an address: it may hold anything.
 *   Nodes: node 0 is (0, 0), node i the end (x_start + p, y_start + q) of row i - 1.  Node (x, y) is OUTSIDE iff it is no
 *   lattice node (0 <= x <= n, 0 <= y <= m), or a = x + y has no diagonal (a >= path_len + 2), or b = y - new_b_offset[a]
 *   is not in [0, B).  The cost cell of a transition into a node has the node's b, so a path with no OUTSIDE node and no
 *   OFF_TYPE, WIDE or INVALID row is one the DP could have returned.
 *   COMPLETE: row 0 starts at (0, 0), every row starts where its predecessor ended, the last row ends at (n, m), and no
 *   row is INVALID (a path without rows is not complete).
 * report (device [8] int32, 16-byte aligned) = (rows, priced, deletions, wide, invalid, off_type, outside nodes, complete).
 * total  (device [2] double): total[0] = sum of (double) c over the PRICED rows + penalty x deletions, total[1] = the
 *   penalty.  The sum is formed in float64 in a fixed order -- row order inside a chunk of 256 rows, chunk order inside the
 *   pair, the deletions' product last -- so it is the same from run to run.
 * scores (device [cap] double, nullable): rows < info[0] as above, nothing past them.
 * A pair with info[1] != 0, with info[0] outside [0, cap], or that failed in the aligner's call gets report = (-1 x 8) and
 * total = (NaN, NaN); its scores are untouched.
 * A null `given`, a negative n_pairs, a count that differs from the last call's, no earlier successful call, a null info /
 * total / report beside non-null rows, a negative cap, or rows / report that are not 16-byte aligned return SVX_ERR_ARG
 * with text and queue nothing.
 * Two launches: one workgroup per chunk of 256 rows (a chunk never spans two pairs; per priced row two candidate rows are
 * read, nothing else of that size), then one workgroup per pair.  Scratch (descriptors, the chunk table, per-chunk
 * partial sums) is the context's post-processing scratch (svx_scratch_bytes). */
typedef struct svx_given {
    const int32_t *rows;   /* device [cap][4]: (x_start, x_len, y_start, y_len) */
    const int32_t *info;   /* device [2]: info[0] = row count, info[1] != 0 -> the pair gets the -1 report */
    int32_t cap, pad;
    double *scores;        /* device [cap], nullable */
    double *total;         /* device [2] */
    int32_t *report;       /* device [8], 16-byte aligned */
} svx_given;
int svx_score_alignments(svx_ctx *ctx, const svx_given *given /* HOST [n_pairs] */, int n_pairs);

/* ---- row slack: how decided is each returned row? (csrc/svx_slack.hip) ------------------------------
 * The entries above judge a whole path.  The slack of a returned row is the min-marginal of the band DP: the total of the
 * best path of the SAME search space that does not contain the row, minus the total of the returned path.  0: there is a
 * second optimum and the row was picked by the tie rule (first strictly smaller candidate, dp_core.pyx); small: the row is
 * ambiguous; several deletion penalties: the row is solid.  ("Margin" is the k-NN ratio margin in this library; this
 * figure is called slack.)
 *
 * Notation of svx_sparse_dp (dp_core.pyx:269-404): A rows of the cost tensor, B cells per diagonal, bout = b_offset_out
 * (bout[0] = bout[1] = b_offset_in[0], bout[a] = b_offset_in[a-2] + 1), xs / ys = x_in_size / y_in_size, moves in list
 * order = the T types (xo, yo), then (0,1), then (1,0), st = xo + yo.
 * Cells.  Cell (a, b), 0 <= a < A+2, 0 <= b < B, is the node (x, y) = (a - y, b + bout[a]); its kind, tested in this order:
 *   border-x  x == 0 and 0 <= y <= ys;   border-y  y == 0 and 0 <= x <= xs;
 *   general   1 <= x <= xs, 1 <= y <= ys and a - 2 < A;   outside  anything else.
 * Edges E: exactly what the forward loop relaxes.  For every general cell v = (a, b) and move t, with ap = a - st and the
 *   predecessor (x - xo, y - yo): when ap >= 0, x - xo >= 0, y - yo >= 0 and bp = (y - yo) - bout[ap] is in [0, B) there is
 *   an edge (ap, bp) -> (a, b) of weight (double) costs[t][a-2][b] for t < T and del_penalty for the two deletions.
 * Border edges E_b: what the traceback walks along the closed-form borders, weight del_penalty: (0, y) -> (0, y+1) when
 *   both are band cells of kind border-x, (x, 0) -> (x+1, 0) when both are band cells of kind border-y, and (0,0) -> (1,0)
 *   from the border-x cell (0,0) to a border-y cell.
 * Forward value F(cell): the csum the forward DP stored (borders closed form, +inf unreachable); nothing is recomputed.
 * Backward value Bk: Bk(end) = 0 for the end cell (xs + ys, ys - bout[xs + ys]); every other border or general cell u has
 *   Bk(u) = min over the edges u -> v of E and E_b of (w + Bk(v)), each candidate ONE float64 addition, +inf when there is no
 *   edge; outside cells are +inf; when the end cell is no band cell every value is +inf.  A minimum of singly rounded sums
 *   does not depend on the order of evaluation: Bk is the same bits from run to run and kernel to kernel.
 * Slack of row r = (x_start, x_len, y_start, y_len): its edge e* goes from u* = (x_start, y_start) to v* = (x_start + x_len,
 *   y_start + y_len) by move (x_len, y_len).  With c = x_start + y_start, the edges with a(u) <= c < a(v) cross the cut
 *   behind diagonal c, and every path crosses it by exactly one of them.
 *     alt[r]   = min over the crossing edges e != e* of ((F(u) + w) + Bk(v)), in that order; +inf when there is none
 *     slack[r] = alt[r] - total,   total = F(end) (+inf when the end cell is no band cell: the difference is then NaN)
 *   Not clamped.  In exact arithmetic slack >= 0; in float64 it may be negative by rounding, by at most
 *   2 (A+2) 2^-53 max|finite csum|.  A row that is no edge of E or E_b -- a negative field, a node off the lattice or off
 *   the band, a move that is neither a type of the list nor a deletion -- gets NaN and is never used to form an address:
 *   row fields may hold anything.  (The DP's own rows are always edges.)
 * A known corner: a border cell keeps its closed-form F even when its border predecessor is no band cell; the reference's
 *   traceback fails on such a path ('traceback bug').  Slack uses the stored F as it is.
 *
 * svx_sparse_dp_backward: the arguments and limits of svx_sparse_dp (costs [T][A][B], A, B >= 1, T <= SVX_MAX_TYPES, type
 *   sizes 1..100; sizes >= 0); writes bsum [A+2][B] = Bk.  One launch, one workgroup: B <= 64 and steps <= 120 take the
 *   LDS-staged sweep, anything else the strided kernel (Bk ring in LDS while it fits 150 KB, else re-read from bsum).
 * svx_path_slack: the slack kernel of svx_row_slack on caller-supplied planes csum, bsum [A+2][B] (device), any B.
 *   rows (device [cap][4], 16-byte aligned), n_rows (device [1]; clamped to [0, cap]); slack[r] is written for r < n_rows,
 *   nothing past that.  One launch.  Reads costs, b_offset_in, the two planes and the rows.
 * Both return SVX_ERR_ARG with text for a null argument, A or B < 1, a negative size, a bad type list, rows not 16-byte
 * aligned, a negative cap; asynchronous on the context's stream. */
int svx_sparse_dp_backward(svx_ctx *ctx, const float *costs, const int32_t *b_offset_in, int A, int B,
                           const int32_t *types_host, int T, double del_penalty, int x_in_size, int y_in_size,
                           double *bsum /* [A+2][B] */);
int svx_path_slack(svx_ctx *ctx, const float *costs, const int32_t *b_offset_in, int A, int B, const int32_t *types_host,
                   int T, double del_penalty, int x_in_size, int y_in_size, const double *csum, const double *bsum,
                   const int32_t *rows /* [n_rows][4] */, const int32_t *n_rows /* device [1] */, int cap,
                   double *slack /* [cap] */);

/* svx_row_slack: the slack of every returned row at level 0 of the LAST svx_align_batch / svx_align_around call on the
 * context, under the rules of svx_band_contact and svx_score_alignments: both halves of a pipelined call, in the pair
 * order of svx_debug_level; n_pairs must equal that call's pair count; svx_flush first; asynchronous on the context's
 * stream, no host synchronisation.  It reads what the call's arena still holds of level 0 and svx_debug_level exposes --
 * the level's own rows and their count, a_b_costs, a_b_csum, b_offset / new_b_offset, the penalty, the sizes, the band and
 * the call's type set -- fp32 costs and fp64 sums that are resident; no embedding row is read again.
 * slack (HOST [n_pairs] of device [n + m + 2] double): slack[p][r] is written for r < the pair's row count, nothing past
 *   that.  slack[p] == NULL skips the pair: nothing of it is written.
 * summary (device [n_pairs][4] int32, 16-byte aligned) = (rows, rows with slack == 0, rows with slack == +inf, 0).
 * A pair with info[1] != 0 gets summary = (-1, -1, -1, -1); its slack is untouched.
 * SVX_ERR_ARG with text, nothing queued: a call that ran the tile sweep, which keeps no cost array (a_b_costs is NULL: a
 * band above 64 cells in the straight and around-wide modes); no earlier successful call; a pair count that differs; a
 * null slack / summary; summary not 16-byte aligned; a negative n_pairs.
 * Two launches, one workgroup per pair each: the backward sweep into a Bk plane, then the slack kernel over it.  The
 * scratch -- the descriptors and one plane of (path capacity + 2) x B doubles per pair -- is the context's
 * post-processing scratch (svx_scratch_bytes). */
int svx_row_slack(svx_ctx *ctx, double *const *slack /* HOST [n_pairs] of device [n+m+2] */,
                  int32_t *summary /* device [n_pairs][4], 16-byte aligned */, int n_pairs);

/* svx_row_slack_wide: svx_row_slack for a last call that ran the tile sweep -- a band above 64 cells in the straight, dense
 * and around-wide modes (csrc/svx_tiles_bwd.hip).  The definition above is unchanged: cells, kinds, E, E_b, F,
 * Bk, the cut, the row's own edge and any duplicate of its move in the list excluded, NaN for a row that is no edge, not
 * clamped.  The one new statement: w is the tile sweep's own cost, the fp32 value its LDS planes hold (the forward sweep
 * keeps no cost array; the value is recomputed from the same rows by the same code).  Every candidate is still one
 * (Bk) or two (the cut) singly rounded float64 additions in the order w + Bk(v), (F(u) + w) + Bk(v), and a minimum does not
 * depend on its order: on equal cost bits the result is svx_path_slack's bits.
 * How: a backward tile sweep over the forward call's tile plan, tickets reversed, computes Bk tile by tile and, for every
 * edge u -> v it relaxes, folds ((F(u) + w) + Bk(v)) into the cuts a(u) <= c < a(v) unless the edge is the returned path's
 * own; cutmin[c] is a per-diagonal minimum (64-bit atomic minimum per (tile, cut)), slack[r] = cutmin[x_start + y_start] -
 * F(end).  One more tile sweep, no cost tensor.
 * sw (HOST [n_pairs]): slack (device [n + m + 2] double; NULL skips the pair: nothing of it is written) and bsum (device
 *   [A+2][B] double, A the level's path length, at least (n + m + 6) rows; NULL: the plane lives in the post-processing
 *   scratch).  A given bsum receives Bk on the lattice nodes that are band cells; its other cells are unspecified.
 * summary, failed pairs, the rules (LAST call on the context, svx_flush first, asynchronous): as svx_row_slack.
 * SVX_ERR_ARG with text, nothing queued: the last call did not run the tile sweep (svx_row_slack measures it); its type set
 * takes the general tile shape (k_band_tiles_gen; no backward sweep yet); no earlier successful call; a pair count that
 * differs; a null sw / summary; summary not 16-byte aligned; slack or bsum not 8-byte aligned; a negative n_pairs.
 * Launches: the node table, the persistent sweep (one workgroup per CU), the slack kernel.  The scratch -- descriptors, per
 * pair cutmin and node table of (path capacity + 2) entries, tile flags, and the plane when it is not the caller's -- is the
 * context's post-processing scratch (svx_scratch_bytes).  Stage name for svx_stage_ms: "tiles_bwd". */
typedef struct svx_slack_wide {
    double *slack;             /* device [n+m+2], NULL: skip the pair */
    double *bsum;              /* device [A+2][B], nullable */
} svx_slack_wide;
int svx_row_slack_wide(svx_ctx *ctx, const svx_slack_wide *sw /* HOST [n_pairs] */,
                       int32_t *summary /* device [n_pairs][4], 16-byte aligned */, int n_pairs);

/* ---- row alternatives: what would the DP have done instead? (csrc/svx_alt.hip) ----------------------
 * Slack says how decided a row is.  These entries name the competitor: the edge that wins the row's cut when the row is
 * forbidden, and the rows of the best path through that edge that replace returned rows (its detour).  For rows the
 * caller believes in they give the regret: how much dearer the best path containing the row is than the returned one.
 * Notation, cells, kinds, the edge sets E and E_b, F, Bk, total and the move list are those of the slack section above.
 * The definitions apply to the rows 0 .. R-1 of one pair, which form a path: their nodes are P_0, P_1, .., P_R, P_i the
 * start of row i and P_R the end of row R-1 (for the DP's own rows P_0 = (0,0) and P_R = (xs, ys)).  A node that is no
 * lattice node or no band cell is not a P_i; when rows that are no path put several nodes on one diagonal, one of them
 * counts, unspecified which (nothing out of range is read or written either way).
 * A row IS AN EDGE under the rule of svx_path_slack: 0 <= x_start, x_len, y_start, y_len; x_start + x_len <= xs;
 *   y_start + y_len <= ys; x_len + y_len >= 1; its end diagonal is below A+2; (x_len, y_len) is a move of the list (its
 *   move index t is the first such entry); both of its nodes are band cells.  No address is formed before that is known.
 *
 * Alternative edge of row r with cut c = x_start + y_start.  The candidates are the crossing edges e = u -> v by move t,
 *   e != e* (an edge from u* by the row's move is e*, whichever list entry it uses), cand(e) = (F(u) + w) + Bk(v) exactly
 *   as in the slack definition.
 *     alt[r] = min cand, slack[r] = alt[r] - total (the bits svx_path_slack / svx_row_slack write).
 *   The alternative edge is the candidate with cand == alt[r] that comes first by diagonal of v ascending, then cell b of
 *   v ascending, then move index t ascending.  There is none when alt[r] = +inf or the row is no edge.
 *     edge[r] = (x_u, xo, y_u, yo), or (-1, -1, -1, -1) without one.
 * Detour of row r: computed when r has an alternative edge, `detour` is not NULL and slack[r] <= max_slack (a plain double
 *   comparison: NaN fails it, +inf measures every row).  With K = max_detour, nb and nf the rows taken so far:
 *   Backward part.  Start from u.  While the node is none of the P_i: when nb == K - 1 the status is 1; else take the
 *     stored back-pointer (xp, yp) of the node's cell -- the step svx_sparse_traceback takes, under its conditions: xp, yp
 *     >= 0, xp + yp >= 1, xp <= x, yp <= y; the step must also be a move of the list and the predecessor a band cell, or
 *     the status is 3 -- and prepend the row (x - xp, xp, y - yp, yp).  The walk stops at L = P_lo.
 *   Forward part.  Start from v.  While the node is none of the P_i: when nb + 1 + nf == K the status is 1; else take the
 *     first move t in list order whose edge node -> s is in E or E_b and for which w + Bk(s) == Bk(node) holds as doubles
 *     (one exists whenever Bk(node) is finite; otherwise the status is 3), and append the row.  The walk stops at J = P_hi.
 *   The detour is the backward rows in document order, the alternative edge, the forward rows: n_detour <= K rows that
 *   replace the returned rows lo .. hi-1; on a path lo <= r < hi.  detour[r][j] = row j; detour_scores[r][j] = 0.0 for a
 *   deletion and max((double) cost cell, 0) / (double) (xo yo) for a typed row (the cost cell of the move index taken: the
 *   edge's t, the forward walk's t, the first list entry of a back-pointer step), as process_scores (dp_utils.py:89-102)
 *   scores a row from its own cost.
 *     span[r] = (lo, hi, n_detour, status): status 0 detour written; 1 too long (the detour has more than K rows);
 *     2 not measured (no alternative edge, no `detour`, or slack above max_slack); 3 walk failed.  For every status but 0
 *     span[r] = (-1, -1, -1, status) and the detour slots of the row are left untouched, as are slots j >= n_detour.
 * Regret of a given row g (any four integers): NaN when g is no edge (no address is formed), else
 *     regret = ((F(u) + w) + Bk(v)) - total, w the weight of the row's move index,
 *   +inf when u is unreachable or v cannot reach the end, 0 for a returned row up to the rounding bound stated for slack.
 *   max_slack does not apply.  Rows g < given_info[0] (clamped to [0, given_cap]) are written, nothing past them; with
 *   given_info[1] != 0 nothing is written.
 *
 * svx_path_alternatives: the kernels of svx_row_alternatives on caller-supplied planes, any B: the arguments of
 *   svx_path_slack, then xp, yp [A+2][B] (svx_sparse_dp), then one svx_alt record (its slack, detour, detour_scores and
 *   given may be NULL; edge, span [cap][4]; detour [cap][K][4]; detour_scores [cap][K]).  Rows r < n_rows (clamped to [0,
 *   cap]) are written.  SVX_ERR_ARG with text, nothing queued: the cases of svx_path_slack; null xp / yp / alt / edge /
 *   span; edge, span, detour or given not 16-byte aligned; max_detour outside [1, SVX_ALT_MAX_DETOUR]; a NaN max_slack;
 *   regret or given_info NULL, or a negative given_cap, beside a non-NULL given.  The node table (8 bytes x (A+2)) is the
 *   context's post-processing scratch.
 * svx_row_alternatives follows every rule of svx_row_slack: level 0 of the LAST svx_align_batch / svx_align_around call,
 *   both halves of a pipelined call, in the pair order of svx_debug_level; n_pairs must equal that call's pair count;
 *   svx_flush first; asynchronous on the context's stream, no host synchronisation.  It reads what svx_row_slack reads and
 *   the level's back-pointers in either layout (a_b_bp bytes, or the a_b_xp / a_b_yp planes).  alt (HOST [n_pairs]): the
 *   arrays of pair p hold n + m + 2 rows; alt[p].edge == NULL skips the pair: nothing of it is written.
 *   summary (device [n_pairs][4] int32, 16-byte aligned) = (rows, rows with an alternative edge, detours written, detours
 *   too long); a pair with info[1] != 0 gets (-1, -1, -1, -1) and nothing else of it is written.
 *   SVX_ERR_ARG with text, nothing queued: a call that ran the tile sweep, which keeps no cost array; no earlier successful
 *   call; a pair count that differs; a null alt / summary; a misaligned summary; and per pair that is not skipped the
 *   record rules above.
 *   Launches: the backward sweep of svx_row_slack (the same kernels, so slack is the same bits), k_row_alt with one
 *   workgroup per pair and one wave per row, and k_given_regret with one thread per given row when any pair has given rows.
 *   Scratch: the descriptors and per pair one Bk plane of (path capacity + 2) x B doubles and a node table of 8 bytes x
 *   (path capacity + 2), in the context's post-processing scratch (svx_scratch_bytes). */
#define SVX_ALT_MAX_DETOUR 256
typedef struct svx_alt {
    double  *slack;            /* device [n+m+2], nullable: alt - total, the bits svx_row_slack writes */
    int32_t *edge;             /* device [n+m+2][4], 16-byte aligned */
    int32_t *span;             /* device [n+m+2][4], 16-byte aligned */
    int32_t *detour;           /* device [n+m+2][K][4], nullable: edges only, every span = (-1,-1,-1,2) */
    double  *detour_scores;    /* device [n+m+2][K], nullable */
    const int32_t *given;      /* device [given_cap][4], nullable, 16-byte aligned */
    const int32_t *given_info; /* device [2] as svx_given.info */
    int32_t given_cap, pad;
    double  *regret;           /* device [given_cap] */
} svx_alt;
int svx_row_alternatives(svx_ctx *ctx, const svx_alt *alt /* HOST [n_pairs] */, int max_detour, double max_slack,
                         int32_t *summary /* device [n_pairs][4] */, int n_pairs);
int svx_path_alternatives(svx_ctx *ctx, const float *costs, const int32_t *b_offset_in, int A, int B, const int32_t *types_host,
                          int T, double del_penalty, int x_in_size, int y_in_size, const double *csum, const double *bsum,
                          const int32_t *xp, const int32_t *yp, const int32_t *rows /* [n_rows][4] */,
                          const int32_t *n_rows /* device [1] */, int cap, const svx_alt *one, int max_detour, double max_slack);

/* Per-level intermediates of the LAST svx_align_batch call on this context -- the entries of the `stack` the reference
 * returns (dp_utils.py:412-537) -- as device pointers into the context's scratch arena (valid until the next call;
 * the scalar fields are read back, which synchronises the stream).  Pointers are NULL for what a level does not have
 * (the coarsest level of a pyramid only has normalisers, penalty and alignments; the tile sweep keeps no cost array).
 * a_b_csum and the back-pointers hold the reference's values on every band cell that is a node of the lattice
 * (0 <= x <= size0, 0 <= y <= size1; +inf / -42 where unreachable).  The band kernels (band <= 64 cells, and every
 * coarse-to-fine level) also fill the band cells outside the lattice like the reference, +inf / -42; the tile sweep
 * stores lattice nodes only, and those cells are UNSPECIFIED there (nothing reads them). */
typedef struct svx_level_view {
    int32_t size0, size1, k0, k1;   /* rows and overlap layers of the two sides at this depth */
    int32_t n_types, band;          /* alignment types of this depth, cells per diagonal (2 * width_over2) */
    int32_t path_len, n_align;      /* search path points (= len(b_offset)); alignments of this depth */
    const float *n0, *n1;           /* [k0][size0], [k1][size1]   stack[d]['n0'], ['n1'] */
    const double *del_penalty;      /* [1]                        stack[d]['del_penalty'] */
    const int32_t *searchpath;      /* [path_len][2]              stack[d]['searchpath'] */
    const float *a_b_costs;         /* [path_len][n_types][band]  stack[d]['a_b_costs'], diagonal-major ([T][A][B] in the reference) */
    const int32_t *b_offset;        /* [path_len]                 stack[d]['b_offset'] */
    const double *a_b_csum;         /* [path_len + 2][band]       stack[d]['a_b_csum'] */
    const uint8_t *a_b_bp;          /* [path_len + 2][band] xp << 4 | yp, 0xFF = -42, or NULL when ... */
    const int32_t *a_b_xp, *a_b_yp; /* ... the types do not pack into 4 bits (then these are set) */
    const int32_t *new_b_offset;    /* [path_len + 2]             stack[d]['new_b_offset'] */
    const int32_t *alignments;      /* [n_align][4] rows (x_start, x_len, y_start, y_len) */
    const double *alignment_scores; /* [n_align] (refined levels) */
    /* the coarsest level of a pyramid (dp_utils.py:465-473), NULL elsewhere: */
    const float *costs_1to1;        /* [size0][size1]             stack[max_depth]['costs_1to1'] (make_dense_costs) */
    const int32_t *x_y_tb_diag;     /* stack[max_depth]['x_y_tb'] (dense_dp back-pointers 0 / 1 / 2, 4 at the origin), stored by
                                     * anti-diagonal: entry (x, y) of the reference's [size0+1][size1+1] array is at
                                     * [(x + y) * (size0 + 1) + x] */
    /* levels >= 1: layer 0 of the level's normalised vectors, [size0][d] / [size1][d] float32 = stack[d]['v0'][0], ['v1'][0]
     * (the other layers of a level are consumed by the pass that forms them and are not kept); NULL at level 0, where the
     * vectors are the caller's inputs */
    const float *v0_l0, *v1_l0;
    /* the sampled 1-1 costs the deletion penalty of this level was estimated from (make_del_knob, dp_utils.py:278-323),
     * in the order of the caller's knob_idx for this level */
    const float *knob_scores;       /* [n_knob] */
    int32_t n_knob, reserved;
} svx_level_view;
int svx_debug_level(svx_ctx *ctx, int pair, int level, svx_level_view *out);
/* Synchronous device -> host copy behind the context's stream (for reading svx_level_view arrays without a tensor library). */
int svx_copy_to_host(svx_ctx *ctx, void *dst_host, const void *src_device, int64_t bytes);

/* Device time of the named stage of the last svx_align_batch call, in milliseconds, measured with
 * HIP events on the context's stream when profiling is on (svx_set_profiling); one name per kernel:
 * "pyr0" "pyr1" "pyrN" "pyr_aux" "knob_sort" "knob_scores0" "knob_scoresN" "knob" "dense_costs" "dense_dp" "path"
 * "band_costs0" "band_costsN" "band_dp0" "band_dpN" "path0" "traceback0" "traceback" "setup" "total" (0 = level 0, N = the
 * deeper levels; "path" and "traceback" without a digit are the deeper levels),
 * "tiles" (the wide-band tile sweep of SVX_SEARCH_STRAIGHT: costs + DP);
 * "tiles_bwd" (svx_row_slack_wide: node table, backward tile sweep, slack kernel; set by that call);
 * "host_plan"/"host_launch" are host wall-clock.  -1 if unknown.
 * svx_set_profiling(ctx, 2): accumulate -- the events are recorded as with 1 but a call neither reads them nor waits
 * for its stream, so calls keep queueing behind one another; svx_stage_ms / svx_stage_launches then return the
 * totals over all svx_align_batch calls since profiling was set to 2 (the first query synchronises the stream). */
int svx_set_profiling(svx_ctx *ctx, int on);
/* Software pipeline over consecutive svx_align_batch calls (default off).  The path of one document pair is a
 * streaming front (pyramid, sampled scores: HBM-bound) followed by a refinement chain whose DP / traceback / search-path
 * kernels are serial per pair and leave the memory system idle.  With the pipeline on, a call cuts its batch into two
 * halves; every streaming kernel runs on the context's stream in one fixed order, the latency-bound kernels of one
 * half run beside the streaming kernels of the other on an internal stream, and the refinement chain of the call's
 * SECOND half is held back to run beside the next call's front.  Contract while it is on: the outputs (and the info
 * words) of a call are complete, in the order of the context's stream, only after svx_flush() (or svx_synchronize /
 * svx_debug_level, which flush); inputs and outputs of a call must stay alive until then.  Results do not depend on
 * the setting.  Wide straight bands (the tile sweep, a persistent kernel over all CUs) always run unpipelined. */
int svx_set_pipeline(svx_ctx *ctx, int on);
/* Launch whatever the pipeline still holds back and make the context's stream wait for it (no host synchronisation).
 * A no-op when nothing is in flight. */
int svx_flush(svx_ctx *ctx);
double svx_stage_ms(svx_ctx *ctx, const char *stage);
/* Number of launches of the named stage in the last batch. */
int svx_stage_launches(svx_ctx *ctx, const char *stage);

#ifdef __cplusplus
}
#endif
#endif /* SVX_H */
