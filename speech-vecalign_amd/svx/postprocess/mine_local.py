"""python -m svx.postprocess.mine_local METADATA OUT_DIR --src_lang en --tgt_lang de --concat_dir D --embed_dir D
    [--is_stopes_embed] [--fp16_embed] [--k 16] [--margin ratio|distance|absolute]
    [--retrieval max|forward|backward|intersection] [--threshold T] [--gpu_type fp16-shard] [--batch_rows N]
    [--rank R --n_shard S] [--skip_existing]

Local Mining, the second mining baseline Speech-Vecalign is compared against: the margin-based mining of
`svx.postprocess.mine` run inside every parallel document pair instead of over the whole corpus.  The file conventions
are those of `svx.seg_align.align`: the pairs come from METADATA (`src_audio<TAB>tgt_audio`), a document's rows are the
rows of {embed_dir}/{lang}/{stem}.embed, and row r is line r ("start end") of {concat_dir}/{lang}/{stem}.txt.

Pairs are packed into batches of at most --batch_rows rows per side; a batch is uploaded, rows holding a NaN become zero
rows (as the aligner's gather makes them), all rows are unit-normalised into the storage type (svx_unit_rows) and the
batch is mined with `mine.mine_local`: one grouped search per direction, whatever the number of pairs.

Output: {out_dir}/{src}-{tgt}/{s}-{t}.txt, one line per mined pair, `score<TAB>src candidate line<TAB>tgt candidate line`,
in `mine_bitexts`' order, the score printed as `mine.format_pairs` prints it.  A pair whose embedding and candidate files
differ in their row counts is skipped with an error line; it and a pair with fewer than k rows on either side get an
empty file.  Ignore-index files and the audio filters are not part of this job."""
import argparse
import dataclasses
import logging
import os
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ..utils.file_utils import check_exist, read_lines, read_metadata
from ..utils.mp_utils import balanced_shards
from .mine import MARGINS, RETRIEVALS

logger = logging.getLogger(__name__)
# 2^18 rows per side: 0.5 GB of unit rows, up to 1 GB of fp32 input and 50 MB of k = 16 lists per side at d = 1024
DEFAULT_BATCH_ROWS = 1 << 18


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("metadata", type=str, help="the meta file that each line contains paired audio paths")
    p.add_argument("out_dir", type=str, help="dir to save the mined pairs.")
    p.add_argument("--src_lang", type=str, required=True)
    p.add_argument("--tgt_lang", type=str, required=True)
    p.add_argument("--concat_dir", type=str, required=True, help="the dir for concatenated segments.")
    p.add_argument("--embed_dir", type=str, required=True, help="Dir to embedding files.")
    p.add_argument("--is_stopes_embed", action="store_true", default=False, help="embeddings were dumped by stopes (SpeechLASER).")
    p.add_argument("--fp16_embed", action="store_true", default=False, help="embeddings are raw fp16 (SONAR numpy dumps)")
    p.add_argument("--k", type=int, default=16, help="number of nearest number.")
    p.add_argument("--margin", type=str, default="ratio", choices=sorted(MARGINS), help="See: https://aclanthology.org/P19-1309")
    p.add_argument("--retrieval", type=str, default="max", choices=RETRIEVALS)
    p.add_argument("--threshold", type=float, default=None, help="keep pairs with a score above it.")
    p.add_argument("--gpu_type", type=str, default="fp16-shard", help="fp16* keeps the rows in fp16, bf16* in bf16.")
    p.add_argument("--batch_rows", type=int, default=DEFAULT_BATCH_ROWS, help="most rows per side mined in one device pass")
    p.add_argument("--rank", type=int, default=int(os.environ.get("RANK", 0)))
    p.add_argument("--n_shard", type=int, default=int(os.environ.get("WORLD_SIZE", 1)))
    p.add_argument("--skip_existing", action="store_true", default=False, help="do not recompute existing outputs")
    a = p.parse_args(argv)
    if not 1 <= a.k <= 64:
        p.error("--k must be 1 .. 64")
    if a.batch_rows < 1:
        p.error("--batch_rows must be positive")
    if not 0 <= a.rank < a.n_shard:
        p.error(f"invalid rank/n_shard {a.rank}/{a.n_shard}")
    return a


@dataclasses.dataclass
class LocalPair:
    src_concat_path: str
    tgt_concat_path: str
    src_embed_path: str
    tgt_embed_path: str
    output_path: str
    n_src: int = -1   # rows of the embedding files (filled by count_rows)
    n_tgt: int = -1


def resolve_pairs(audio_pairs: Sequence[Tuple[str, ...]], src_concat_dir: Path, tgt_concat_dir: Path, src_embed_dir: Path,
                  tgt_embed_dir: Path, out_dir: Path) -> List[LocalPair]:
    """The per-pair file set, as align.validate_inputs resolves it; pairs with a missing file are dropped."""
    res = []
    for pair in audio_pairs:
        s, t = Path(pair[0]), Path(pair[1])
        paths = []
        for sdir, tdir, suffix in ((src_concat_dir, tgt_concat_dir, ".txt"), (src_embed_dir, tgt_embed_dir, ".embed")):
            sp, tp = (sdir / s.name).with_suffix(suffix), (tdir / t.name).with_suffix(suffix)
            if not check_exist(sp) or not check_exist(tp):
                paths = None
                break
            paths += [sp.as_posix(), tp.as_posix()]
        if paths is not None:
            res.append(LocalPair(*paths, (out_dir / f"{s.stem}-{t.stem}.txt").as_posix()))
    return res


def shard_pairs(pairs: List[LocalPair], n_shard: int, rank: int) -> List[LocalPair]:
    """This rank's pairs: the list split by embedding-file size (mp_utils.balanced_shards); every pair lands in one shard."""
    if n_shard <= 1:
        return list(pairs)
    costs = [os.path.getsize(p.src_embed_path) + os.path.getsize(p.tgt_embed_path) for p in pairs]
    return [pairs[i] for i in balanced_shards(costs, n_shard)[rank]]


def count_rows(p: LocalPair, use_stopes: bool, fp16_embed: bool) -> Optional[Tuple[List[str], List[str]]]:
    """Fills p.n_src / p.n_tgt from the embedding files and returns the candidate lines of the two documents, or None (with
    an error line) when a document's embedding file and candidate file differ in their row counts."""
    from ..utils.embedding_utils import embedding_file_layout
    lines, ok = [], True
    for side, embed, concat in (("n_src", p.src_embed_path, p.src_concat_path), ("n_tgt", p.tgt_embed_path, p.tgt_concat_path)):
        rows = embedding_file_layout(embed, use_stopes, fp16_embed)[1]
        setattr(p, side, int(rows))
        lines.append(read_lines(concat))
        if len(lines[-1]) != rows:
            logger.error(f"{embed} holds {rows} rows, {concat} {len(lines[-1])} lines: the pair is skipped")
            ok = False
    return (lines[0], lines[1]) if ok else None


def plan_batches(counts: Sequence[Tuple[int, int]], batch_rows: int) -> List[List[int]]:
    """counts[i] = (source rows, target rows) of pair i -> lists of consecutive pair indices with at most batch_rows rows
    per side in each; a pair that is larger than that on its own makes a batch of its own."""
    batches, cur, nx, ny = [], [], 0, 0
    for i, (a, b) in enumerate(counts):
        if cur and (nx + a > batch_rows or ny + b > batch_rows):
            batches.append(cur)
            cur, nx, ny = [], 0, 0
        cur.append(i)
        nx, ny = nx + a, ny + b
    if cur:
        batches.append(cur)
    return batches


def _write_text(path: str, text: str):
    tmp = path + ".tmp"
    with open(tmp, "w") as fp:  # write-then-rename, the repo's crash-safety idiom
        fp.write(text)
    Path(tmp).replace(path)


def _unit_side(ctx, paths, use_stopes, fp16_embed, storage, pool):
    """The embedding files of one side of a batch -> one fp16 / bf16 device tensor of unit rows, file after file."""
    import ctypes
    from .. import _lib
    from ..utils.embedding_utils import read_embeddings_pinned
    t = ctx.torch
    ctx.use_current_stream()
    hosts = pool.map(lambda path: read_embeddings_pinned(path, use_stopes, fp16_embed), paths)
    if len({(h.dtype, h.shape[1]) for h in hosts}) != 1:
        raise ValueError("the embedding files of a batch differ in element type or dimension")
    x = t.cat([h.to(ctx.tdev, non_blocking=True) for h in hosts], dim=0).contiguous()
    x[t.isnan(x).any(dim=1)] = 0   # a row holding a NaN becomes a zero row (embedding_utils.py:183-190)
    out = t.empty(x.shape, dtype=t.float16 if storage == "fp16" else t.bfloat16, device=ctx.tdev)
    code = {t.float32: _lib.SVX_F32, t.float16: _lib.SVX_F16}[x.dtype]
    ctx.check(ctx.lib.svx_unit_rows(ctx.h, ctypes.c_void_p(x.data_ptr()), code, int(x.shape[0]), int(x.shape[1]),
                                    ctypes.c_void_p(out.data_ptr()), _lib.SVX_F16 if storage == "fp16" else _lib.SVX_BF16))
    return out


def mine_pairs(pairs: List[LocalPair], args, stats: Optional[dict] = None):
    """Mine every pair of the list and write its file."""
    from multiprocessing.pool import ThreadPool
    from .. import _lib
    from .mine import mine_local
    storage = "bf16" if args.gpu_type.startswith("bf16") else "fp16"
    todo = [p for p in pairs if not (args.skip_existing and Path(p.output_path).exists())]
    n_skipped = n_small = n_lines = 0
    ready = []   # (pair, source lines, target lines)
    for p in todo:
        lines = count_rows(p, args.is_stopes_embed, args.fp16_embed)
        if lines is None:
            n_skipped += 1
            _write_text(p.output_path, "")
        elif p.n_src < args.k or p.n_tgt < args.k:
            n_small += 1
            _write_text(p.output_path, "")
        else:
            ready.append((p,) + lines)
    if ready:
        ctx = _lib.context()
        pool = ThreadPool(max(2, min(16, os.cpu_count() or 4)))
        try:
            for batch in plan_batches([(p.n_src, p.n_tgt) for p, _, _ in ready], args.batch_rows):
                chunk = [ready[i] for i in batch]
                x = _unit_side(ctx, [p.src_embed_path for p, _, _ in chunk], args.is_stopes_embed, args.fp16_embed, storage, pool)
                y = _unit_side(ctx, [p.tgt_embed_path for p, _, _ in chunk], args.is_stopes_embed, args.fp16_embed, storage, pool)
                x_off = np.concatenate([[0], np.cumsum([p.n_src for p, _, _ in chunk])]).astype(np.int64)
                y_off = np.concatenate([[0], np.cumsum([p.n_tgt for p, _, _ in chunk])]).astype(np.int64)
                scores, src, tgt, group = mine_local(x, y, x_off, y_off, args.k, args.margin, args.retrieval, args.threshold)
                bounds = np.searchsorted(group, np.arange(len(chunk) + 1))
                for g, (p, sl, tl) in enumerate(chunk):
                    lo, hi = int(bounds[g]), int(bounds[g + 1])
                    _write_text(p.output_path, "".join(f"{s}\t{sl[i]}\t{tl[j]}\n" for s, i, j in zip(scores[lo:hi], src[lo:hi], tgt[lo:hi])))
                    n_lines += hi - lo
        finally:
            pool.close()
            pool.join()
    logger.info(f"{len(ready)} pairs mined ({n_lines} lines), {n_small} with fewer than k = {args.k} rows on a side, "
                f"{n_skipped} skipped for a row-count mismatch, {len(pairs) - len(todo)} existing")
    if stats is not None:
        stats.update(mined=len(ready), small=n_small, skipped=n_skipped, existing=len(pairs) - len(todo), lines=n_lines)


def main(argv=None, stats: Optional[dict] = None):
    args = parse_args(argv)
    logger.info(args)
    src_lang, tgt_lang = args.src_lang, args.tgt_lang
    out_dir = Path(args.out_dir) / f"{src_lang}-{tgt_lang}"
    out_dir.mkdir(parents=True, exist_ok=True)
    pairs = resolve_pairs(read_metadata(args.metadata), Path(args.concat_dir) / src_lang, Path(args.concat_dir) / tgt_lang,
                          Path(args.embed_dir) / src_lang, Path(args.embed_dir) / tgt_lang, out_dir)
    if args.n_shard > 1:
        # one process per GPU; document pairs are independent, so shards never communicate
        import torch
        if torch.cuda.is_available():
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", args.rank)) % max(1, torch.cuda.device_count()))
        pairs = shard_pairs(pairs, args.n_shard, args.rank)
        logger.info(f"rank {args.rank} of {args.n_shard}: {len(pairs)} pairs")
    mine_pairs(pairs, args, stats)


if __name__ == '__main__':
    main()
