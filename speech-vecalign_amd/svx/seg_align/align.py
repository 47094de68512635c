"""Segment-alignment driver: the reference's `python -m svecalign.seg_align.align` on MI355X.

Same positional arguments, flags, directory conventions and output format as
svecalign/seg_align/align.py (parse_args :13-96, validate_inputs :117-179, main :182-230):

    python -m svx.seg_align.align METADATA OUT_DIR --src_lang en --tgt_lang de \
        --seg_dir D --concat_dir D --embed_dir D [--is_stopes_embed] [--fp16_embed] [-a 6] ...

Additive flags only: --batch_size (document pairs aligned per device pass; the reference loops one
pair at a time), --seed (per-pair sampling streams derived from (seed, pair index): results do not
depend on batch size or shard count; without it the global numpy stream is consumed pair after
pair exactly like the reference), --skip_existing, --rank/--n_shard (default from torchrun's
RANK/WORLD_SIZE: one process per GPU, pairs split by cost, no collective needed).

--margin_dir DIR adds the global margin score of every alignment that is no deletion (and passes --max_cost), without
the reference's second pass of the speech encoder (postprocess/embed_align.py): the embedding of an un-concatenated
alignment's span is the candidate row the DP has just read, so after every batch svx_alignment_rows gathers those rows
on the device, and after the last batch they are scored against the union over ranks (global_margin_scores).  Under
torch.distributed.run the ranks form a process group for that exchange; the alignment files do not change.

--concat_max_num N / --min_dur S (with --max_sil, --concat_max_dur, --apply_dur_cond_to_both_sides) put the reference's text
post-filters between alignment and margin scoring -- filter_by_cost --max_cost, concat_aligns --max_num_align N, filter_by_dur
--min_dur S (example/voxpopuli/run.sh steps 6.1, 6.3, 6.4) -- into this job.  The audio-based filter_untrans_align of step 6.2
is NOT part of the chain.  With --margin_dir the chain runs on the device (svx_concat_rows) and the margin files hold one
line per joined alignment whose span is still a candidate row (at most k0 x k1 segments); wider ones need the encoder and
are only counted.  --post_dir DIR writes the chain's full output, wide lines included, as concat_aligns / filter_by_dur write
it; that is host work on the results already fetched (filters.post_chain).

--contact_tsv PATH reports, per pair, how many nodes of the returned path sit on the edge of the search band
(svx_band_contact): the sign that the band may have cut the best alignment off.  --widen searches such pairs again around
their own result in twice the band until the path clears the edge (svx_align_widen; --widen_rounds, --widen_max_band,
--widen_guard).  It removes search errors, not model errors, so it is opt-in; without these flags nothing changes.

--rescore_dir DIR --rescore_tsv PATH answer the question the contact report leaves open: for every pair that has an
alignment file DIR/{src}-{tgt}/{s}-{t}.txt (gold, an earlier run, another tool's output) that path is priced with the
normalisers and the deletion penalty this run used (svx_score_alignments) and compared with the total of the path the DP
returned: `search` when the given path is cheaper (the search missed it), `model` when it is dearer (no band will find it),
`unpriced` when a row of it has no price.  The alignment files do not change.

--slack_dir DIR says how DECIDED each returned row is, which its cost does not: DIR/{src}-{tgt}/{s}-{t}.txt holds the job's
own alignment lines with a fourth field, the row's slack (svx_row_slack) -- the total of the best path of the same band that
does not contain the row, minus the total of the returned path: `[0, 1]:[0]:0.349737:0.012345`.  0 means a second optimum
exists and the tie rule picked the row; a small value means the row is ambiguous (a repeated phrase, near-silent segments);
several deletion penalties mean it is solid; `inf` means no other path exists in the band.  The alignment files do not change.
--slack_wide_dir DIR writes the same files for a band above 64 cells (--mode band / dense / --prior_band), where the tile
sweep keeps no cost array: the slack comes from a backward tile sweep (svx_row_slack_wide), same definition.  In --mode dense
the band follows the documents: a batch whose documents all have at most 31 rows runs the band kernels and is measured by
svx_row_slack, so one flag serves a corpus of mixed sizes.  Not with --widen (a follow-up: after band doubling the last device
call holds only the pairs that were searched again, and slack would have to be measured round by round).

--alt_dir DIR names the competitor behind a small slack (svx_row_alternatives): DIR/{src}-{tgt}/{s}-{t}.txt holds one
tab-separated line per returned row that has a written detour -- row number, slack, lo, hi, then the detour's rows in the
alignment files' syntax: the rows of the best path avoiding the row that replace the returned rows lo .. hi-1.  Rows with a
slack above --alt_max_slack (default inf) are not measured and detours of more than --alt_max_detour rows (default 16, at most
256; a guess until detour lengths on real documents are known) are not written.  --regret_dir DIR goes with --rescore_dir:
DIR/{src}-{tgt}/{s}-{t}.txt holds the rows of the given path (gaps filled with deletions, as it is priced) as
`[src ids]:[tgt ids]:regret`, the total of the best path of the band containing the row minus the returned total: 0 for a row
the DP returned or could have, small for a near miss, large for a row the model rejects, `nan` for a row the band or the type
set does not hold.  The alignment files do not change.
"""
import argparse
import dataclasses
import logging
import os
from pathlib import Path
from typing import List, Optional, Tuple, Union

import numpy as np

from ..utils.file_utils import check_exist, read_metadata
from ..utils.log_utils import my_tqdm
from ..utils.mp_utils import balanced_shards
from ..vecalign.vecalign import resolve_search_params

logger = logging.getLogger(__name__)


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("metadata", type=str, help="the meta file that each line contains paired audio paths")
    p.add_argument("out_dir", type=str, help="dir to save alignments.")
    p.add_argument("--src_lang", type=str, required=True)
    p.add_argument("--tgt_lang", type=str, required=True)
    p.add_argument("--seg_dir", type=str, required=True, help="the dir for raw segments.")
    p.add_argument("--concat_dir", type=str, required=True, help="the dir for concatenated segments.")
    p.add_argument("--embed_dir", type=str, required=True, help="Dir to embedding files.")
    p.add_argument("--is_stopes_embed", action="store_true", default=False, help="embeddings were dumped by stopes (SpeechLASER).")
    p.add_argument("--fp16_embed", action="store_true", default=False, help="embeddings are raw fp16 (SONAR numpy dumps)")
    p.add_argument('-a', '--alignment_max_size', dest="alignment_max_size", type=int, default=6,
                   help='Searches for alignments up to size N-M, where N+M <= this value.')
    p.add_argument('--search_buffer_size', type=int, default=5, help='Width (one side) of search buffer.')
    p.add_argument('-d', '--del_percentile_frac', dest="del_percentile_frac", type=float, default=0.2,
                   help='Deletion penalty percentile (fraction) of the cost distribution.')
    p.add_argument('--max_size_full_dp', type=int, default=300, help='Largest N for full N^2 dynamic programming.')
    p.add_argument('--costs_sample_size', type=int, default=20000, help='Samples for the cost distribution.')
    p.add_argument('--num_samps_for_norm', type=int, default=100, help='Samples for normalizing embeddings')
    p.add_argument("--ign_indices_dir", type=str, default=None,
                   help="if provided, then some segments will be ignored when loading embeddings.")
    # additive
    p.add_argument("--mode", choices=["ref", "band", "dense", "around"], default="ref",
                   help="search region: ref = the reference's coarse-to-fine recursion (default); band = Sakoe-Chiba band of "
                        "--band cells around the straight diagonal; dense = every cell of the lattice (include/svx.h: SVX_SEARCH_STRAIGHT); "
                        "around = the reference-mode band around a prior alignment, without the pyramid (SVX_SEARCH_AROUND; "
                        "needs --prior_dir or --prior time; --prior_band sets another band)")
    p.add_argument("--prior_dir", type=str, default=None,
                   help="--mode around: alignment files {prior_dir}/{src}-{tgt}/{s}-{t}.txt in this job's output format; a pair "
                        "without one is dropped with a warning")
    p.add_argument("--prior", choices=["time"], default=None,
                   help="--mode around: time = blocks of --prior_window seconds from the segments' timestamps (svx_time_prior)")
    p.add_argument("--prior_window", type=float, default=30.0, help="--prior time: window length, seconds")
    p.add_argument("--prior_lag", type=float, default=0.0, help="--prior time: delay of the target side, seconds (may be negative)")
    p.add_argument("--band", type=int, default=2048, help="--mode band: cells per diagonal (2 * width_over2)")
    p.add_argument("--prior_band", type=int, default=None,
                   help="--mode around: cells per diagonal around the prior (2 * width_over2; even, at least 6) instead of the "
                        "reference-mode band; above 64 cells the wide-band tile sweep runs around the prior (SVX_SEARCH_AROUND_WIDE). "
                        "One number per run: results do not depend on batches or shards.  The pairs whose prior needs a wider band "
                        "to be covered (svx_prior_width) are counted in the log")
    p.add_argument("--contact_tsv", type=str, default=None,
                   help="write one line per pair, 'src tgt touch run clearance nodes rounds final_band' (tab-separated): the nodes of the "
                        "returned path on the edge of the search band, the longest run of them, the smallest distance to the edge in "
                        "cells and the node count (svx_band_contact); a path that touches may be a search error.  With --widen: touch "
                        "after the pair's last round, and -1 for run, clearance and nodes")
    p.add_argument("--widen", action="store_true", default=False,
                   help="search a pair whose path touches the band edge again around that path in twice the band, until it clears "
                        "the edge (svx_align_widen).  Removes search errors, not model errors; meant for bands the user chose "
                        "(--mode band, --mode around)")
    p.add_argument("--widen_rounds", type=int, default=4, help="--widen: doublings at the most")
    p.add_argument("--widen_max_band", type=int, default=None,
                   help="--widen: cells per diagonal at the most (default: the band in use times 2 ** widen_rounds)")
    p.add_argument("--widen_guard", type=int, default=0,
                   help="--widen / --contact_tsv: a node touches when it is at most this many cells from the edge")
    p.add_argument("--rescore_dir", type=str, default=None,
                   help="alignment files {rescore_dir}/{src}-{tgt}/{s}-{t}.txt (either line format of this job's outputs) to price with "
                        "this run's costs (svx_score_alignments); a pair without one gives no line.  Needs --rescore_tsv")
    p.add_argument("--rescore_tsv", type=str, default=None,
                   help="--rescore_dir: write one line per pair, 'src tgt verdict found_total given_total del_penalty rows priced deletions "
                        "wide invalid off_type outside complete' (tab-separated): verdict search = the given path is cheaper than the "
                        "returned one, model = it is dearer, unpriced = it has rows without a price or is no complete path, invalid = "
                        "the file is no monotone alignment (the numbers are then empty)")
    p.add_argument("--slack_dir", type=str, default=None,
                   help="also write {slack_dir}/{src}-{tgt}/{s}-{t}.txt: the alignment lines with a fourth field, the row's slack "
                        "(svx_row_slack): best total of a path of the same band without the row minus the returned path's total, "
                        "%%.6f; 0 = tied with another optimum, inf = no other path.  Needs the band's cost array: not for bands above "
                        "64 cells in --mode band / dense / --prior_band (the tile sweep keeps none)")
    p.add_argument("--slack_wide_dir", type=str, default=None,
                   help="--slack_dir for bands above 64 cells (--mode band / dense / --prior_band): the same files, the slack "
                        "measured by the backward tile sweep (svx_row_slack_wide), which needs no cost array.  Needs an alignment "
                        "type set on an LDS-resident tile shape (at most 16 types on 12 overlap layers, sizes up to 8: -a 2 .. 6); "
                        "narrower bands take --slack_dir (--mode dense: a batch of documents of at most 31 rows is measured that way "
                        "by itself)")
    p.add_argument("--alt_dir", type=str, default=None,
                   help="also write {alt_dir}/{src}-{tgt}/{s}-{t}.txt: per returned row with a written detour one tab-separated line "
                        "'row slack lo hi detour rows...' (svx_row_alternatives): the rows of the best path of the same band without "
                        "the row that replace the returned rows lo .. hi-1, in the alignment files' syntax.  Needs the band's cost "
                        "array, like --slack_dir")
    p.add_argument("--alt_max_detour", type=int, default=16,
                   help="--alt_dir: longest detour written, in rows (1 .. 256); the default is a guess until detour lengths on real "
                        "documents are known")
    p.add_argument("--alt_max_slack", type=float, default=float("inf"), help="--alt_dir: measure only rows with at most this slack")
    p.add_argument("--regret_dir", type=str, default=None,
                   help="--rescore_dir: also write {regret_dir}/{src}-{tgt}/{s}-{t}.txt: the given path's rows as src_ids:tgt_ids:regret, "
                        "the best total of a path of the band WITH the row minus the returned path's total (svx_row_alternatives); "
                        "nan = the band or the type set does not hold the row")
    p.add_argument("--batch_size", type=int, default=32, help="document pairs per device pass")
    p.add_argument("--io_threads", type=int, default=None, help="host threads that parse / read ahead of the GPU (default: the CPU count, at most 32)")
    p.add_argument("--seed", type=int, default=None, help="derive one sampling stream per pair from (seed, pair index)")
    p.add_argument("--skip_existing", action="store_true", default=False, help="do not recompute existing outputs")
    p.add_argument("--rank", type=int, default=int(os.environ.get("RANK", 0)))
    p.add_argument("--n_shard", type=int, default=int(os.environ.get("WORLD_SIZE", 1)))
    p.add_argument("--margin_dir", type=str, default=None,
                   help="also write {margin_dir}/{src}-{tgt}/{s}-{t}.txt: one line src_ids:tgt_ids:margin per alignment that is no "
                        "deletion (and passes --max_cost), scored against the rows of all ranks.  The rows stay on the device until "
                        "the last batch: (e + 2) * d bytes per kept alignment and side, e = the embeddings' element size")
    p.add_argument("--margin", choices=["ratio", "distance"], default="ratio", help="--margin_dir: margin function (https://aclanthology.org/P19-1309)")
    p.add_argument("--k", type=int, default=16, help="--margin_dir: number of nearest neighbours")
    p.add_argument("--max_cost", type=float, default=None,
                   help="--margin_dir: keep the alignments filter_by_cost --max_cost keeps from the alignment file (default: every non-deletion)")
    p.add_argument("--margin_storage", choices=["fp16", "bf16"], default="fp16", help="--margin_dir: storage of the unit-norm database rows")
    p.add_argument("--margin_exchange", choices=["allgather", "ring"], default="allgather",
                   help="--margin_dir: how the ranks' rows meet (global_margin_scores)")
    p.add_argument("--concat_max_num", type=int, default=None,
                   help="join up to N consecutive connected alignments (concat_aligns --max_num_align N) before --margin_dir / --post_dir")
    p.add_argument("--max_sil", type=float, default=1.0, help="--concat_max_num: largest gap between joined alignments, seconds (concat_aligns --max_sil)")
    p.add_argument("--concat_max_dur", type=float, default=20.0, help="--concat_max_num: longest joined source span, seconds (concat_aligns --max_dur)")
    p.add_argument("--apply_dur_cond_to_both_sides", action="store_true", default=False, help="--concat_max_num: --concat_max_dur also limits the target span")
    p.add_argument("--min_dur", type=float, default=None,
                   help="drop (joined) alignments with a side shorter than S seconds (filter_by_dur --min_dur S) before --margin_dir / --post_dir")
    p.add_argument("--post_dir", type=str, default=None,
                   help="also write {post_dir}/{src}-{tgt}/{s}-{t}.txt: the alignments after filter_by_cost --max_cost, concat_aligns and "
                        "filter_by_dur, one src_ids:tgt_ids per line (the audio filter filter_untrans_align is not part of this chain)")
    args = p.parse_args(argv)
    if args.mode == "around":
        if (args.prior_dir is None) == (args.prior is None):
            p.error("--mode around takes exactly one of --prior_dir and --prior time")
        if args.prior == "time" and not args.prior_window * PRIOR_SAMPLE_RATE >= 1:
            p.error("--prior_window must be at least one sample")
        if args.prior_band is not None and (args.prior_band < 6 or args.prior_band % 2 != 0):
            p.error("--prior_band must be even and at least 6")
    elif args.prior_dir is not None or args.prior is not None or args.prior_band is not None:
        p.error("--prior_dir / --prior / --prior_band need --mode around")
    if args.widen_rounds < 0 or args.widen_guard < 0:
        p.error("--widen_rounds and --widen_guard must be >= 0")
    if args.widen_max_band is not None and args.widen_max_band < 6:
        p.error("--widen_max_band must be at least 6")
    if (args.rescore_dir is None) != (args.rescore_tsv is None):
        p.error("--rescore_dir and --rescore_tsv go together")
    if args.rescore_dir is not None and args.widen:
        p.error("--rescore_dir cannot be combined with --widen: after band doubling the last device call holds only the pairs "
                "that were searched again")
    if args.rescore_dir is not None and args.skip_existing:
        p.error("--rescore_dir cannot be combined with --skip_existing: a skipped pair has no costs to price a path with")
    if args.slack_wide_dir is not None and args.slack_dir is not None:
        p.error("--slack_wide_dir and --slack_dir measure the same rows: a band above 64 cells takes --slack_wide_dir, a "
                "narrower one --slack_dir")
    if args.slack_dir is not None:
        if args.widen:
            p.error("--slack_dir cannot be combined with --widen: after band doubling the last device call holds only the pairs "
                    "that were searched again")
        if args.skip_existing:
            p.error("--slack_dir cannot be combined with --skip_existing: a skipped pair has no costs to measure slack with")
        cells = 2 * max(3, (args.band + 1) // 2) if args.mode == "band" else (args.prior_band if args.mode == "around" else None)
        if cells is not None and cells > 64:   # (--mode dense: the band follows the documents; the library refuses it)
            p.error(f"--slack_dir needs the band's cost array: a band of {cells} cells runs the tile sweep, which keeps no cost "
                    "array (at most 64 cells in --mode band and with --prior_band)")
    if args.slack_wide_dir is not None:
        if args.widen:
            p.error("--slack_wide_dir cannot be combined with --widen: after band doubling the last device call holds only the pairs "
                    "that were searched again")
        if args.skip_existing:
            p.error("--slack_wide_dir cannot be combined with --skip_existing: a skipped pair has no costs to measure slack with")
        cells = 2 * max(3, (args.band + 1) // 2) if args.mode == "band" else (args.prior_band if args.mode == "around" else None)
        if args.mode == "ref" or (args.mode != "dense" and (cells is None or cells <= 64)):
            p.error("--slack_wide_dir measures the tile sweep, which runs bands above 64 cells in --mode band / dense and with "
                    "--prior_band: this band keeps its cost array, use --slack_dir")
        from ..vecalign.dp_utils import tile_shape
        if tile_shape(resolve_search_params(args.alignment_max_size, None, args.search_buffer_size)[0]) not in (0, 1):
            p.error(f"--slack_wide_dir: the alignment types of -a {args.alignment_max_size} take the general tile shape, which has "
                    "no backward sweep (at most 16 types on 12 overlap layers: -a 2 .. 6); --slack_dir measures bands of at most "
                    "64 cells with any type set")
    if args.regret_dir is not None and args.rescore_dir is None:
        p.error("--regret_dir needs --rescore_dir: the rows whose regret is wanted come from its files")
    if not 1 <= args.alt_max_detour <= 256:
        p.error("--alt_max_detour must be 1 .. 256")
    if args.alt_max_slack != args.alt_max_slack:
        p.error("--alt_max_slack must be a number")
    for flag in ("alt_dir", "regret_dir"):
        if getattr(args, flag) is None:
            continue
        if args.widen:
            p.error(f"--{flag} cannot be combined with --widen: after band doubling the last device call holds only the pairs "
                    "that were searched again")
        if args.skip_existing:
            p.error(f"--{flag} cannot be combined with --skip_existing: a skipped pair has no costs to measure alternatives with")
        cells = 2 * max(3, (args.band + 1) // 2) if args.mode == "band" else (args.prior_band if args.mode == "around" else None)
        if cells is not None and cells > 64:   # (--mode dense: the band follows the documents; the library refuses it)
            p.error(f"--{flag} needs the band's cost array: a band of {cells} cells runs the tile sweep, which keeps no cost "
                    "array (at most 64 cells in --mode band and with --prior_band)")
    if args.concat_max_num is not None and not 1 <= args.concat_max_num <= 8:
        p.error("--concat_max_num must be 1 .. 8")
    if args.min_dur is not None and args.min_dur < 0:
        p.error("--min_dur must be >= 0")
    if post_chain_wanted(args):
        if args.margin_dir is None and args.post_dir is None:
            p.error("--concat_max_num / --min_dur need --margin_dir or --post_dir")
    if args.post_dir is not None and args.skip_existing:
        p.error("--post_dir cannot be combined with --skip_existing")
    if args.margin_dir is not None and args.skip_existing:
        p.error("--margin_dir needs the rows of every pair: it cannot be combined with --skip_existing")
    if args.max_cost is not None and args.max_cost < 0:
        p.error("--max_cost must be >= 0")
    return args


PRIOR_SAMPLE_RATE = 16000  # --prior time: seconds -> sample positions of the segment files


def frames_wanted(args) -> bool:
    """Whether the segment timestamps are read: for the post-filter chain or for a time prior."""
    return post_chain_wanted(args) or getattr(args, "prior", None) == "time"


def prior_path(args, p) -> Path:
    """--prior_dir: the prior alignment file of a pair, named like its output file."""
    return Path(args.prior_dir) / f"{args.src_lang}-{args.tgt_lang}" / os.path.basename(p.output_path)


def rescore_path(args, p) -> Path:
    """--rescore_dir: the given alignment file of a pair, named like its output file."""
    return Path(args.rescore_dir) / f"{args.src_lang}-{args.tgt_lang}" / os.path.basename(p.output_path)


def post_chain_wanted(args) -> bool:
    """Whether the post-filter chain (cost, joining, duration) runs, and with it the reading of the segment timestamps."""
    return any(getattr(args, k, None) is not None for k in ("concat_max_num", "min_dur", "post_dir"))


def post_chain_params(args) -> dict:
    """The chain's parameters as filters.post_chain / PreparedBatch.concat_rows take them (without the cost threshold)."""
    from ..postprocess.filters import SAMPLE_RATE
    return dict(max_num_align=1 if getattr(args, "concat_max_num", None) is None else args.concat_max_num,
                max_sil=getattr(args, "max_sil", 1.0), max_dur=getattr(args, "concat_max_dur", 20.0),
                both_sides=bool(getattr(args, "apply_dur_cond_to_both_sides", False)),
                min_frames=0 if getattr(args, "min_dur", None) is None else int(SAMPLE_RATE * args.min_dur))   # filter_by_dur.py:23


@dataclasses.dataclass
class VecalignData:
    src_seg_path: str
    tgt_seg_path: str
    src_concat_path: str
    tgt_concat_path: str
    src_embed_path: str
    tgt_embed_path: str
    output_path: str
    src_ignore_indices: Optional[Union[str, Path]] = None
    tgt_ignore_indices: Optional[Union[str, Path]] = None
    index: int = 0  # position in the validated list (seeds derive from it)


def validate_inputs(audio_pairs: List[Tuple[str, str]], src_seg_dir: Path, tgt_seg_dir: Path, src_concat_dir: Path,
                    tgt_concat_dir: Path, src_embed_dir: Path, tgt_embed_dir: Path, out_dir: Path,
                    ign_indices_dir: Optional[Path] = None) -> List[VecalignData]:
    """Resolve the per-pair file set; pairs with a missing file are dropped (align.py:117-179)."""
    res = []
    for src_audio, tgt_audio in audio_pairs:
        s, t = Path(src_audio), Path(tgt_audio)
        found = {}
        for kind, sdir, tdir, suffix in (("seg", src_seg_dir, tgt_seg_dir, ".txt"),
                                         ("concat", src_concat_dir, tgt_concat_dir, ".txt"),
                                         ("embed", src_embed_dir, tgt_embed_dir, ".embed")):
            sp, tp = (sdir / s.name).with_suffix(suffix), (tdir / t.name).with_suffix(suffix)
            if not check_exist(sp) or not check_exist(tp):
                found = None
                break
            found[kind] = (sp.as_posix(), tp.as_posix())
        if found is None:
            continue
        src_ign = tgt_ign = None
        if ign_indices_dir is not None:
            src_ign = ign_indices_dir / f"{s.stem}-{t.stem}.src.txt"
            tgt_ign = ign_indices_dir / f"{s.stem}-{t.stem}.tgt.txt"
            src_ign = src_ign if check_exist(src_ign) else None
            tgt_ign = tgt_ign if check_exist(tgt_ign) else None
        res.append(VecalignData(found["seg"][0], found["seg"][1], found["concat"][0], found["concat"][1],
                                found["embed"][0], found["embed"][1], (out_dir / f"{s.stem}-{t.stem}.txt").as_posix(),
                                src_ign, tgt_ign, index=len(res)))
    return res


def pair_rng(seed: Optional[int], index: int):
    """Independent legacy RandomState per pair, a pure function of (seed, pair index)."""
    if seed is None:
        return None
    return np.random.RandomState(np.random.SeedSequence([seed, index]).generate_state(4))


def format_alignment_rows(rows: np.ndarray, scores: Optional[np.ndarray]) -> bytes:
    """print_alignments' text (vecalign.py:174-184) for alignment rows (x_start, x_len, y_start, y_len), by the
    native formatter (svx_format_alignments): byte-identical to the Python '%s:%s:%.6f' of lists."""
    import ctypes
    from .. import _lib
    lib = _lib.load()
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    n = int(rows.shape[0])
    sc = None if scores is None else np.ascontiguousarray(scores, dtype=np.float64)
    cap = 64 * n + 16 * int(rows[:, 1].sum() + rows[:, 3].sum()) + 16
    buf = ctypes.create_string_buffer(cap)
    need = lib.svx_format_alignments(ctypes.c_void_p(rows.ctypes.data), ctypes.c_void_p(sc.ctypes.data if sc is not None else 0), n, buf, cap)
    if need < 0 or need > cap:
        raise Exception("svx_format_alignments: buffer of %d bytes, %d needed" % (cap, need))
    return buf.raw[:need]


def _write_result(path: str, rows: np.ndarray, scores: np.ndarray):
    tmp = path + ".tmp"
    with open(tmp, "wb") as fp:  # write-then-rename, the repo's crash-safety idiom
        fp.write(format_alignment_rows(rows, scores))
    Path(tmp).replace(path)


def format_slack_lines(rows: np.ndarray, scores: np.ndarray, slack: np.ndarray) -> str:
    """--slack_dir: the lines of the alignment file, each with ':%.6f' of the row's slack behind it ('inf' for +inf)."""
    lines = format_alignment_rows(rows, scores).decode().splitlines()
    assert len(lines) == len(slack), f"{len(lines)}, {len(slack)}"
    return "".join("%s:%.6f\n" % (ln, float(v)) for ln, v in zip(lines, slack))


def _write_slack(path: str, rows: np.ndarray, scores: np.ndarray, slack: np.ndarray):
    _write_text(path, format_slack_lines(rows, scores, slack))


def format_alt_lines(slack: np.ndarray, span: np.ndarray, detours) -> str:
    """--alt_dir: one line per row r with a written detour (span[r] = (lo, hi, n_detour, 0)): r, '%.6f' of the slack, lo, hi and
    the detour's rows as the alignment file prints rows, tab-separated.  detours[r]: None or (rows [k, 4], scores [k])."""
    out = []
    for r in range(len(span)):
        if int(span[r][3]) != 0 or detours[r] is None:
            continue
        rows = format_alignment_rows(detours[r][0], detours[r][1]).decode().splitlines()
        out.append("\t".join(["%d" % r, "%.6f" % float(slack[r]), "%d" % int(span[r][0]), "%d" % int(span[r][1])] + rows) + "\n")
    return "".join(out)


def format_regret_lines(rows: np.ndarray, regret: np.ndarray) -> str:
    """--regret_dir: `[src ids]:[tgt ids]:%.6f` per given row, the field being the row's regret ('nan': no edge of the band)."""
    lines = format_alignment_rows(rows, None).decode().splitlines()
    assert len(lines) == len(regret), f"{len(lines)}, {len(regret)}"
    return "".join("%s:%.6f\n" % (ln, float(v)) for ln, v in zip(lines, regret))


def _write_alt(path: str, slack: np.ndarray, span: np.ndarray, detour: np.ndarray, scores: np.ndarray):
    detours = [(detour[r, :span[r, 2]], scores[r, :span[r, 2]]) if span[r, 3] == 0 else None for r in range(len(span))]
    _write_text(path, format_alt_lines(slack, span, detours))


def _write_regret(path: str, rows: np.ndarray, regret: np.ndarray):
    _write_text(path, format_regret_lines(rows, regret))


def _write_post(path: str, rows: np.ndarray, scores: np.ndarray, frames, max_cost, chain: dict):
    """--post_dir: the chain's output for one pair, as concat_aligns / filter_by_dur write it; like them, no file when nothing is left."""
    from ..postprocess.filters import post_chain
    from ..vecalign.dp_utils import rows_to_alignments
    out = post_chain([(s, t, c) for (s, t), c in zip(rows_to_alignments(rows), scores.tolist())], frames[0], frames[1], max_cost, **chain)
    if out:
        _write_text(path, "".join(f"{s}:{t}\n" for s, t in out))


def _write_text(path: str, text: str):
    tmp = path + ".tmp"
    with open(tmp, "w") as fp:
        fp.write(text)
    Path(tmp).replace(path)


class MarginRows:
    """--margin_dir: the kept alignments' rows of every batch of this rank, on the device until the last batch."""

    def __init__(self, args):
        from ..postprocess.filters import cost_limit
        self.args = args
        self.limit = float("inf") if args.max_cost is None else cost_limit(args.max_cost)
        self.chain = dict(post_chain_params(args), max_score=self.limit) if post_chain_wanted(args) else None
        self.n_fit = self.n_wide = 0
        self.parts = []    # per batch: (x_rows, y_rows, x_unit, y_unit) trimmed to the kept rows
        self.files = []    # per pair with kept rows, in row order: (file name, ["src_ids:tgt_ids", ...])
        self.d = self.dtype = None

    def gather(self, pb):
        """Behind pb.run() on the compute stream (asynchronous)."""
        if self.chain is not None:
            pb.concat_rows(self.chain, self.args.margin_storage)
        else:
            pb.alignment_rows(self.limit, self.args.margin_storage)

    def collect(self, chunk, pb, info, align, offs):
        """After the batch's fetch event: trim the row buffers to the count and note the ids of the kept alignments."""
        cnt = pb.rows_count()
        if self.chain is not None:
            self.n_fit += cnt
            self.n_wide += int(pb.h_rows[0][1])
        x_rows, y_rows, x_unit, y_unit, _, _ = pb.rows
        self.d, self.dtype = int(x_rows.shape[1]), x_rows.dtype
        pb.rows = None
        if cnt == 0:
            return
        self.parts.append(tuple(t[:cnt].clone() for t in (x_rows, y_rows, x_unit, y_unit)))
        src = pb.h_rows[1].numpy()[:cnt]   # (pair, row) per kept alignment, or svx_concat_rows' meta
        bounds = np.searchsorted(src[:, 0], np.arange(len(chunk) + 1))
        for i, p in enumerate(chunk):
            if self.chain is not None:
                rows = src[bounds[i]:bounds[i + 1], 4:8]
            else:
                rows = align[int(offs[i]) + src[bounds[i]:bounds[i + 1], 1]]
            if len(rows):
                self.files.append((os.path.basename(p.output_path),
                                   ["%s:%s" % (list(range(r[0], r[0] + r[1])), list(range(r[2], r[2] + r[3]))) for r in rows.tolist()]))

    def finish(self, ctx):
        """Score this rank's rows against the union over ranks and write the margin files."""
        import torch
        from ..postprocess.score_align import _dist_rank_world, global_margin_scores
        a = self.args
        if self.chain is not None:
            logger.info(f"post-filter chain: {self.n_fit} joined alignments fit a candidate row and are margin-scored, "
                        f"{self.n_wide} are wider (they need the encoder and are left out of {a.margin_dir})")
        _, world, _ = _dist_rank_world()
        udt = torch.float16 if a.margin_storage == "fp16" else torch.bfloat16
        if world > 1:   # a rank without pairs still takes part in the exchange: it needs the others' row shape
            import torch.distributed as dist
            codes = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
            shape = torch.tensor([self.d or 0, codes.get(self.dtype, 0)], dtype=torch.int64, device=ctx.tdev)
            dist.all_reduce(shape, op=dist.ReduceOp.MAX)
            if self.d is None:
                self.d, self.dtype = int(shape[0]), {v: k for k, v in codes.items()}[int(shape[1])]
        if not self.d:
            return
        if self.parts:
            x, y, xu, yu = (torch.cat(ts, dim=0) for ts in zip(*self.parts))
        else:
            x, y = (torch.empty((0, self.d), dtype=self.dtype, device=ctx.tdev) for _ in range(2))
            xu, yu = (torch.empty((0, self.d), dtype=udt, device=ctx.tdev) for _ in range(2))
        self.parts = []
        scores = global_margin_scores(x, y, k=a.k, margin=a.margin, storage=a.margin_storage, exchange=a.margin_exchange,
                                      x_unit=xu, y_unit=yu).cpu().numpy()
        out_dir = Path(a.margin_dir) / f"{a.src_lang}-{a.tgt_lang}"
        out_dir.mkdir(parents=True, exist_ok=True)
        at = 0
        for name, ids in self.files:   # `src:tgt:score` as score_align.write_to_output prints it
            _write_text((out_dir / name).as_posix(), "".join(f"{s}:{scores[at + j]}\n" for j, s in enumerate(ids)))
            at += len(ids)
        assert at == scores.shape[0], f"{at}, {scores.shape}"


def _prepare_pair(p: VecalignData, args, src_k: int, tgt_k: int):
    """Host half of one document pair (runs on a pool thread; the heavy parts are native / I/O and release the
    GIL): candidate index tables from the segment and candidate files, embedding files into pinned memory."""
    from ..utils.embedding_utils import candidate_table_from_files, read_embeddings_pinned
    st, _ = candidate_table_from_files(p.src_seg_path, p.src_concat_path, src_k, p.src_ignore_indices)
    tt, _ = candidate_table_from_files(p.tgt_seg_path, p.tgt_concat_path, tgt_k, p.tgt_ignore_indices)
    se = read_embeddings_pinned(p.src_embed_path, args.is_stopes_embed, args.fp16_embed)
    te = read_embeddings_pinned(p.tgt_embed_path, args.is_stopes_embed, args.fp16_embed)
    fr = None
    if frames_wanted(args):   # (start, end) sample positions per segment, for joining, the duration filter and a time prior
        from ..utils.file_utils import read_segments
        fr = tuple(np.asarray(read_segments(path), dtype=np.int64).reshape(-1, 2) for path in (p.src_seg_path, p.tgt_seg_path))
        for f in fr:
            if len(f) and (f.min() < -2 ** 31 or f.max() >= 2 ** 31):
                raise ValueError(f"{p.src_seg_path}: sample positions beyond int32")
    pr = None
    if getattr(args, "prior_dir", None) is not None:
        from ..utils.file_utils import read_alignments
        pr = read_alignments(prior_path(args, p))
    given = None   # --rescore_dir: None (no file), ("ok", the complete path) or ("invalid", why)
    if getattr(args, "rescore_dir", None) is not None and check_exist(rescore_path(args, p)):
        from ..utils.file_utils import read_alignments
        from ..vecalign.dp_utils import complete_alignments
        try:
            given = ("ok", complete_alignments(read_alignments(rescore_path(args, p)), int(st.shape[1]), int(tt.shape[1])))
        except ValueError as e:
            logger.warning(f"--rescore_dir: {rescore_path(args, p)} is no monotone alignment and is not priced: {e}")
            given = ("invalid", str(e))
    return st, tt, se, te, fr, pr, given


def align_pairs(pairs: List[VecalignData], args, batch_size: int, io_threads: Optional[int] = None, stats: Optional[dict] = None):
    """The reference's serial loop (align.py:206-230) as a three-stage pipeline around svx_align_batch:
      host threads   parse segment / candidate files into index tables, read .embed files into pinned memory
                     (`io_threads`, running ahead by two batches);
      copy stream    uploads batch i+1 while the compute stream aligns batch i (device gather of the candidate
                     tensor, then the whole of vecalign());
      writer threads format and write the alignment files of batch i-1.
    Results do not depend on the batch size, the thread count or the shard count when --seed is given."""
    import torch
    from collections import deque
    from multiprocessing.pool import ThreadPool
    from .. import _lib
    from ..utils.embedding_utils import gather_candidates
    from ..vecalign.dp_utils import PreparedBatch
    types, src_k, tgt_k, width_over2 = resolve_search_params(args.alignment_max_size, None, args.search_buffer_size)
    todo = [p for p in pairs if not (args.skip_existing and Path(p.output_path).exists())]
    margin = MarginRows(args) if getattr(args, "margin_dir", None) is not None else None
    chain = post_chain_params(args) if post_chain_wanted(args) else None
    post_dir = None
    if getattr(args, "post_dir", None) is not None:
        post_dir = Path(args.post_dir) / f"{args.src_lang}-{args.tgt_lang}"
        post_dir.mkdir(parents=True, exist_ok=True)
    slack_dir, slack_wide = None, getattr(args, "slack_wide_dir", None) is not None
    if getattr(args, "slack_dir", None) is not None or slack_wide:   # (one file format, two ways to measure)
        slack_dir = Path(args.slack_wide_dir if slack_wide else args.slack_dir) / f"{args.src_lang}-{args.tgt_lang}"
        slack_dir.mkdir(parents=True, exist_ok=True)
    alt_dir, regret_dir = (None if getattr(args, flag, None) is None else Path(getattr(args, flag)) / f"{args.src_lang}-{args.tgt_lang}"
                           for flag in ("alt_dir", "regret_dir"))
    for dpath in (alt_dir, regret_dir):
        if dpath is not None:
            dpath.mkdir(parents=True, exist_ok=True)
    if not todo:
        if margin is not None and int(os.environ.get("WORLD_SIZE", "1")) > 1:   # the other ranks wait for this one in the exchange
            margin.finish(_lib.context())
        return
    ctx = _lib.context()
    dev = ctx.tdev
    nthr = io_threads or max(2, min(32, (os.cpu_count() or 4)))
    # (the current device is per thread: pool threads that allocate pinned memory must name this rank's GPU, or every
    #  rank would open a context on GPU 0)
    dev_index = dev.index if dev.index is not None else torch.cuda.current_device()
    io_pool = ThreadPool(nthr, initializer=torch.cuda.set_device, initargs=(dev_index,))
    out_pool = ThreadPool(max(2, nthr // 2))
    copy_stream = torch.cuda.Stream(device=dev)
    compute = torch.cuda.current_stream(dev)
    batches = [todo[b0:b0 + batch_size] for b0 in range(0, len(todo), batch_size)]
    ahead = deque()   # (chunk, [async results of _prepare_pair])
    nxt = 0

    def submit_more():
        nonlocal nxt
        while nxt < len(batches) and len(ahead) < 3:
            ahead.append((batches[nxt], [io_pool.apply_async(_prepare_pair, (p, args, src_k, tgt_k)) for p in batches[nxt]]))
            nxt += 1

    def finish(job):
        chunk, pb, ev, held = job
        ev.synchronize()
        if getattr(pb, "h_widths", None) is not None:   # --prior_band: priors whose blocks the band in use does not cover
            uncovered[0] += int((pb.h_widths.numpy() > pb.width_over2).sum())
        info, align, scores, _, offs = pb.raw_results()
        report = getattr(pb, "widen_report", None)
        if report is not None:
            widened[0] += int((report[:, 0] > 0).sum())
            touching[0] += int((report[:, 3] > 0).sum())
        elif getattr(pb, "h_contact", None) is not None:
            touching[0] += int((pb.h_contact.numpy()[:, 0] > 0).sum())
        if contact_tsv is not None:
            for i, p in enumerate(chunk):
                s, t = os.path.basename(p.src_seg_path), os.path.basename(p.tgt_seg_path)
                if report is not None:
                    vals = [int(report[i, 3]), -1, -1, -1, int(report[i, 0]), 2 * int(report[i, 1])]
                else:
                    vals = pb.h_contact.numpy()[i].tolist() + [0, 2 * int(pb.width_over2)]
                contact_lines.append("\t".join([s, t] + [str(v) for v in vals]) + "\n")
        if rescore_tsv is not None:
            from ..vecalign.dp_utils import search_error
            h = None if getattr(pb, "h_given", None) is None else [x.numpy() for x in pb.h_given]
            for i, p in enumerate(chunk):
                given = held[0][i][6]
                if given is None:
                    continue
                s, t = os.path.basename(p.src_seg_path), os.path.basename(p.tgt_seg_path)
                if given[0] != "ok":
                    rescore_lines.append("\t".join([s, t, "invalid"] + [""] * 11) + "\n")
                    continue
                found, got, rep = float(h[0][i, 0]), float(h[1][i, 0]), h[2][i].tolist()
                rescore_lines.append("\t".join([s, t, search_error(found, got, rep), "%.6f" % found, "%.6f" % got, "%.6f" % float(h[1][i, 1])]
                                               + [str(int(v)) for v in rep]) + "\n")
        if margin is not None:
            margin.collect(chunk, pb, info, align, offs)
        writes = []
        for i, p in enumerate(chunk):
            o, cnt = int(offs[i]), int(info[i, 0])
            writes.append(out_pool.apply_async(_write_result, (p.output_path, align[o:o + cnt], scores[o:o + cnt])))
            if slack_dir is not None:
                writes.append(out_pool.apply_async(_write_slack, ((slack_dir / os.path.basename(p.output_path)).as_posix(), align[o:o + cnt],
                                                                  scores[o:o + cnt], pb.h_slack.numpy()[o:o + cnt])))
            if alt_dir is not None:
                h = pb.h_alt
                writes.append(out_pool.apply_async(_write_alt, ((alt_dir / os.path.basename(p.output_path)).as_posix(),
                                                                h['slack'].numpy()[o:o + cnt], h['span'].numpy()[o:o + cnt],
                                                                h['detour'].numpy()[o:o + cnt], h['detour_scores'].numpy()[o:o + cnt])))
            if regret_dir is not None and pb.regret_rows[i] is not None:
                g0, g1 = int(pb.alt_given_offs[i]), int(pb.alt_given_offs[i + 1])
                writes.append(out_pool.apply_async(_write_regret, ((regret_dir / os.path.basename(p.output_path)).as_posix(),
                                                                   pb.regret_rows[i], pb.h_alt['regret'].numpy()[g0:g1])))
            if post_dir is not None:
                writes.append(out_pool.apply_async(_write_post, ((post_dir / os.path.basename(p.output_path)).as_posix(), align[o:o + cnt],
                                                                 scores[o:o + cnt], held[0][i][4], args.max_cost, chain)))
        return writes, (pb, held)  # (the pinned result buffers stay alive until the writers are done)

    pending_job, pending_writes = None, deque()
    uncovered = [0]
    widen = bool(getattr(args, "widen", False))
    contact_tsv = getattr(args, "contact_tsv", None)
    guard = int(getattr(args, "widen_guard", 0))
    widened, touching, contact_lines = [0], [0], []
    rescore_tsv, rescore_lines = getattr(args, "rescore_tsv", None), []
    bar = my_tqdm(total=len(todo))
    try:
        submit_more()
        while ahead:
            chunk, futs = ahead.popleft()
            submit_more()
            prepared = [f.get() for f in futs]
            # ---- uploads on the copy stream (pinned -> device), then gather + align on the compute stream
            with torch.cuda.stream(copy_stream):
                dev_in = [(torch.from_numpy(st).to(dev, non_blocking=True), torch.from_numpy(tt).to(dev, non_blocking=True),
                           se.to(dev, non_blocking=True), te.to(dev, non_blocking=True)) for st, tt, se, te, _, _, _ in prepared]
                up = torch.cuda.Event()
                up.record(copy_stream)
            compute.wait_event(up)
            docs = []
            for (st, tt, se, te, _, _, _), (dst, dtt, dse, dte) in zip(prepared, dev_in):
                for x in (dst, dtt, dse, dte):
                    x.record_stream(compute)
                sv, tv = gather_candidates(dse, dst), gather_candidates(dte, dtt)
                if sv.dtype != tv.dtype:
                    sv, tv = sv.float(), tv.float()
                docs.append((sv, tv))
            rngs = None if args.seed is None else [pair_rng(args.seed, p.index) for p in chunk]
            mode = getattr(args, "mode", "ref")
            if mode == "ref":
                w2, search = width_over2, "coarse_to_fine"
            elif mode == "band":
                w2, search = max(3, (args.band + 1) // 2), "straight"
            elif mode == "around" and getattr(args, "prior_band", None) is not None:  # an explicit band around the prior
                w2, search = args.prior_band // 2, "around_wide"
            elif mode == "around":  # the reference-mode band around a prior, no pyramid
                w2, search = width_over2, "around"
            else:  # dense: the band covers the lattice (width_over2 > max(N, M))
                w2, search = max(max(int(sv.shape[1]), int(tv.shape[1])) for sv, tv in docs) + 1, "straight"
            time_prior = mode == "around" and args.prior == "time"
            priors = None if mode != "around" else [None if time_prior else q[5] for q in prepared]
            pb = PreparedBatch(docs, types, args.del_percentile_frac, w2, args.max_size_full_dp,
                               args.costs_sample_size, args.num_samps_for_norm, rngs=rngs, search=search,
                               frames=[q[4] for q in prepared] if (margin is not None and chain is not None) or time_prior else None,
                               priors=priors)
            if time_prior:
                pb.time_prior(int(round(args.prior_window * PRIOR_SAMPLE_RATE)), int(round(args.prior_lag * PRIOR_SAMPLE_RATE)))
            if search == "around_wide":
                pb.prior_width_async()   # (read back with the results: fetch_async)
            if widen:   # (synchronous: every round reads its contact report back)
                max_w2 = None if getattr(args, "widen_max_band", None) is None else max(pb.width_over2, args.widen_max_band // 2)
                pb.widen_report = pb.run_widen(guard=guard, max_width_over2=max_w2, max_rounds=args.widen_rounds)
            else:
                pb.run()
                if contact_tsv is not None:
                    contact = pb.band_contact(0, guard)
                    pb.h_contact = torch.empty(contact.shape, dtype=contact.dtype, pin_memory=True)
                    pb.h_contact.copy_(contact, non_blocking=True)   # (lands before the event of fetch_async)
            if slack_dir is not None:   # one call behind run(); read back with the results
                # (--slack_wide_dir in --mode dense: the band follows the batch's documents, and a batch of documents of at most
                #  31 rows runs the band kernels, which keep their cost array: svx_row_slack measures that one)
                sl, _ = pb.row_slack_wide() if slack_wide and pb.took_tile_sweep() else pb.row_slack()
                pb.h_slack = torch.empty(sl.shape, dtype=sl.dtype, pin_memory=True)
                pb.h_slack.copy_(sl, non_blocking=True)
            if alt_dir is not None or regret_dir is not None:   # one call behind run(); read back with the results
                from ..vecalign.dp_utils import given_rows_from_alignments
                pb.regret_rows = [given_rows_from_alignments(q[6][1]) if regret_dir is not None and q[6] is not None and q[6][0] == "ok"
                                  else None for q in prepared]
                alt = pb.row_alternatives(args.alt_max_detour, args.alt_max_slack, given=pb.regret_rows if regret_dir is not None else None,
                                          detour=alt_dir is not None)
                pb.alt_given_offs = alt.get('given_offs')
                pb.h_alt = {k: torch.empty(v.shape, dtype=v.dtype, pin_memory=True) for k, v in alt.items() if torch.is_tensor(v)}
                for k, hx in pb.h_alt.items():
                    hx.copy_(alt[k], non_blocking=True)
            if rescore_tsv is not None and any(q[6] is not None and q[6][0] == "ok" for q in prepared):
                # two calls behind run(): the returned paths' totals, then the given paths'; read back with the results
                ok = [q[6] is not None and q[6][0] == "ok" for q in prepared]
                own = pb.score_alignments(["own" if k else None for k in ok])
                got = pb.score_alignments([q[6][1] if k else None for q, k in zip(prepared, ok)])
                pb.h_given = tuple(torch.empty(x.shape, dtype=x.dtype, pin_memory=True) for x in (own.total, got.total, got.report))
                for hx, dx in zip(pb.h_given, (own.total, got.total, got.report)):
                    hx.copy_(dx, non_blocking=True)
                pb.given_keep = (own, got)
            if margin is not None:
                margin.gather(pb)
            ev = pb.fetch_async()
            job = (chunk, pb, ev, (prepared, dev_in))
            # ---- while this batch computes: hand the previous batch to the writers
            if pending_job is not None:
                pending_writes.append(finish(pending_job))
                bar.update(len(pending_job[0]))
            pending_job = job
            while len(pending_writes) > 1:
                for w in pending_writes.popleft()[0]:
                    w.get()
        if pending_job is not None:
            pending_writes.append(finish(pending_job))
            bar.update(len(pending_job[0]))
        for writes, _ in pending_writes:
            for w in writes:
                w.get()
        if margin is not None:
            margin.finish(ctx)
    except BaseException:
        # a failed pair must not leave threads behind: drop the reads still queued, let the writes already handed
        # over finish (their files are complete or absent: write-then-rename), then re-raise
        io_pool.terminate()
        for writes, _ in pending_writes:
            for w in writes:
                try:
                    w.get(timeout=120)
                except Exception:
                    pass
        out_pool.terminate()
        raise
    finally:
        bar.close()
        io_pool.close()
        out_pool.close()
        io_pool.join()
        out_pool.join()
    if getattr(args, "prior_band", None) is not None:
        logger.info(f"--prior_band {args.prior_band}: {uncovered[0]} of {len(todo)} pairs have a covering band above the band in use")
    if contact_tsv is not None:
        shard = "" if getattr(args, "n_shard", 1) <= 1 else f".{args.rank}"   # (one file per rank: the ranks do not communicate)
        _write_text(contact_tsv + shard, "".join(contact_lines))
    if rescore_tsv is not None:
        shard = "" if getattr(args, "n_shard", 1) <= 1 else f".{args.rank}"   # (one file per rank, like --contact_tsv)
        _write_text(rescore_tsv + shard, "".join(rescore_lines))
    if widen or contact_tsv is not None:
        logger.info(f"band contact: {touching[0]} of {len(todo)} pairs touch the edge of their final band"
                    + (f", {widened[0]} were searched again in a wider band" if widen else ""))
    if stats is not None:
        stats["widened"] = widened[0]
        stats["still_touching"] = touching[0]
        stats["uncovered_priors"] = uncovered[0]
        stats["pairs"] = len(todo)
        stats["io_threads"] = nthr


def main(argv=None):
    args = parse_args(argv)
    logger.info(args)
    src_lang, tgt_lang = args.src_lang, args.tgt_lang
    out_dir = Path(args.out_dir) / f"{src_lang}-{tgt_lang}"
    out_dir.mkdir(parents=True, exist_ok=True)
    ign = None
    if args.ign_indices_dir is not None:
        ign = Path(args.ign_indices_dir) / f"{src_lang}-{tgt_lang}"
        logger.info(f"Will ignore segments indicated by {ign}")
    valid = validate_inputs(read_metadata(args.metadata),
                            Path(args.seg_dir) / src_lang, Path(args.seg_dir) / tgt_lang,
                            Path(args.concat_dir) / src_lang, Path(args.concat_dir) / tgt_lang,
                            Path(args.embed_dir) / src_lang, Path(args.embed_dir) / tgt_lang, out_dir, ign)
    if getattr(args, "prior_dir", None) is not None:
        have = [p for p in valid if check_exist(prior_path(args, p))]
        if len(have) < len(valid):
            logger.warning(f"--prior_dir: {len(valid) - len(have)} of {len(valid)} pairs have no prior alignment and are dropped")
        valid = have
    if args.n_shard > 1:
        # one process per GPU; document pairs are independent, so shards never communicate
        import torch
        if torch.cuda.is_available():
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", args.rank)) % max(1, torch.cuda.device_count()))
        costs = [os.path.getsize(p.src_embed_path) + os.path.getsize(p.tgt_embed_path) for p in valid]
        valid = [valid[i] for i in balanced_shards(costs, args.n_shard)[args.rank]]
        logger.info(f"rank {args.rank} of {args.n_shard}: {len(valid)} pairs")
    align_pairs(valid, args, max(1, args.batch_size), io_threads=args.io_threads)


if __name__ == '__main__':
    main()
