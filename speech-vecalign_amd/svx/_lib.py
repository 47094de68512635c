"""ctypes binding of libsvx.so (include/svx.h).  No CPU fallback: if the library or a GPU is
missing, importing/creating a context raises."""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SVX_LIB") or os.path.join(_HERE, "libsvx.so")   # (SVX_LIB: A/B builds, profiles/build_variant.sh)

SVX_F32, SVX_F16, SVX_BF16 = 0, 1, 2
SVX_MAX_TYPES = 128
SVX_MAX_LEVELS = 16
SVX_MARGIN_RATIO, SVX_MARGIN_DISTANCE, SVX_MARGIN_ABSOLUTE = 0, 1, 2
SVX_SEARCH_COARSE_TO_FINE, SVX_SEARCH_STRAIGHT, SVX_SEARCH_AROUND, SVX_SEARCH_AROUND_WIDE = 0, 1, 2, 3

SVX_OK, SVX_ERR_ARG, SVX_ERR_OVERLAPS, SVX_ERR_HIP, SVX_ERR_TRACEBACK = 0, 1, 2, 3, 4
SVX_ERR_NOMEM, SVX_ERR_EXTEND, SVX_ERR_PATH, SVX_ERR_BP = 5, 6, 7, 8

# messages of the reference for the device-side failure codes (dp_utils.py:124,167,243)
DEVICE_ERRORS = {
    SVX_ERR_TRACEBACK: "traceback bug",
    SVX_ERR_BP: "got unknown value",
    SVX_ERR_EXTEND: "asked to extend alignments but already bigger than requested",
    SVX_ERR_PATH: "search path is not a unit-step lattice path",
}

c_int, c_i64, c_f32, c_f64, c_vp = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_void_p


class AlignParams(ctypes.Structure):
    _fields_ = [
        ("dtype", ctypes.c_int32),
        ("d", ctypes.c_int32),
        ("n_types", ctypes.c_int32),
        ("types", ctypes.c_int32 * (2 * SVX_MAX_TYPES)),
        ("width_over2", ctypes.c_int32),
        ("max_size_full_dp", ctypes.c_int32),
        ("costs_sample_size", ctypes.c_int32),
        ("num_samps_for_norm", ctypes.c_int32),
        ("del_percentile_frac", ctypes.c_double),
        ("search_mode", ctypes.c_int32),
        ("reserved0", ctypes.c_int32),
    ]


class LevelView(ctypes.Structure):
    _fields_ = [
        ("size0", ctypes.c_int32), ("size1", ctypes.c_int32), ("k0", ctypes.c_int32), ("k1", ctypes.c_int32),
        ("n_types", ctypes.c_int32), ("band", ctypes.c_int32), ("path_len", ctypes.c_int32), ("n_align", ctypes.c_int32),
        ("n0", c_vp), ("n1", c_vp), ("del_penalty", c_vp), ("searchpath", c_vp), ("a_b_costs", c_vp), ("b_offset", c_vp),
        ("a_b_csum", c_vp), ("a_b_bp", c_vp), ("a_b_xp", c_vp), ("a_b_yp", c_vp), ("new_b_offset", c_vp),
        ("alignments", c_vp), ("alignment_scores", c_vp),
        ("costs_1to1", c_vp), ("x_y_tb_diag", c_vp), ("v0_l0", c_vp), ("v1_l0", c_vp),
        ("knob_scores", c_vp), ("n_knob", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


class Pair(ctypes.Structure):
    _fields_ = [
        ("vecs0", c_vp), ("vecs1", c_vp),
        ("n", ctypes.c_int32), ("m", ctypes.c_int32), ("k0", ctypes.c_int32), ("k1", ctypes.c_int32),
        ("norm_idx", c_vp), ("knob_idx", c_vp),
        ("norms0", c_vp), ("norms1", c_vp),
        ("align", c_vp), ("scores", c_vp), ("info", c_vp), ("del_pen", c_vp),
    ]


class Frames(ctypes.Structure):
    """svx_frames: per pair the device arrays [n][2], [m][2] of (start, end) sample positions."""
    _fields_ = [("src", c_vp), ("tgt", c_vp)]


class Prior(ctypes.Structure):
    """svx_prior: device rows [cap][4] and info [2] of a prior alignment (svx_align_around, svx_time_prior, svx_prior_width)."""
    _fields_ = [("rows", c_vp), ("info", c_vp), ("cap", ctypes.c_int32), ("pad", ctypes.c_int32)]


class WidenParams(ctypes.Structure):
    """svx_widen_params: band doubling (svx_align_widen)."""
    _fields_ = [("guard", ctypes.c_int32), ("max_width_over2", ctypes.c_int32), ("max_rounds", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class Given(ctypes.Structure):
    """svx_given: device rows [cap][4] and info [2] of a given alignment, and where its scores [cap], total [2] and
    report [8] go (svx_score_alignments)."""
    _fields_ = [("rows", c_vp), ("info", c_vp), ("cap", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("scores", c_vp), ("total", c_vp), ("report", c_vp)]


class SlackWide(ctypes.Structure):
    """svx_slack_wide: where the slack of one pair goes and, optionally, its Bk plane (svx_row_slack_wide)."""
    _fields_ = [("slack", c_vp), ("bsum", c_vp)]


class Alt(ctypes.Structure):
    """svx_alt: where the alternatives of one pair go (svx_row_alternatives, svx_path_alternatives)."""
    _fields_ = [("slack", c_vp), ("edge", c_vp), ("span", c_vp), ("detour", c_vp), ("detour_scores", c_vp),
                ("given", c_vp), ("given_info", c_vp), ("given_cap", ctypes.c_int32), ("pad", ctypes.c_int32), ("regret", c_vp)]


SVX_ALT_MAX_DETOUR = 256


class ConcatParams(ctypes.Structure):
    """svx_concat_params (include/svx.h)."""
    _fields_ = [
        ("max_score", ctypes.c_double),
        ("max_num_align", ctypes.c_int32), ("sample_rate", ctypes.c_int32),
        ("max_sil", ctypes.c_double), ("max_dur", ctypes.c_double),
        ("both_sides", ctypes.c_int32), ("pad", ctypes.c_int32),
        ("min_frames", ctypes.c_int64),
    ]


SVX_CONCAT_MAX = 8
SVX_KNOB_SORT_STAGE_LDS = 150 * 1024   # bytes of LDS within which svx_knob_sort stages its scatter (include/svx.h)

_SIGS = {
    "svx_create": (c_int, [c_int, ctypes.POINTER(c_vp)]),
    "svx_destroy": (c_int, [c_vp]),
    "svx_set_stream": (c_int, [c_vp, c_vp]),
    "svx_synchronize": (c_int, [c_vp]),
    "svx_last_error": (ctypes.c_char_p, [c_vp]),
    "svx_version": (ctypes.c_char_p, []),
    "svx_scratch_bytes": (c_i64, [c_vp]),
    "svx_dense_costs": (c_int, [c_vp, c_vp, c_int, c_int, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_int, c_int, c_vp]),
    "svx_dense_dp": (c_int, [c_vp, c_vp, c_int, c_int, c_f32, c_vp, c_vp]),
    "svx_score_path": (c_int, [c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_int, c_vp]),
    "svx_sparse_costs": (c_int, [c_vp, c_vp, c_int, c_int, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_int,
                                 ctypes.POINTER(ctypes.c_int32), c_int, c_int, c_vp, c_vp]),
    "svx_sparse_dp": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, ctypes.POINTER(ctypes.c_int32), c_int, c_f64, c_int, c_int,
                              c_vp, c_vp, c_vp, c_vp]),
    "svx_sparse_dp_backward": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, ctypes.POINTER(ctypes.c_int32), c_int, c_f64, c_int, c_int,
                                       c_vp]),
    "svx_path_slack": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, ctypes.POINTER(ctypes.c_int32), c_int, c_f64, c_int, c_int,
                               c_vp, c_vp, c_vp, c_vp, c_int, c_vp]),
    "svx_make_norm1": (c_int, [c_vp, c_vp, c_i64, c_int]),
    "svx_downsample": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_vp]),
    "svx_compute_norms": (c_int, [c_vp, c_vp, c_int, c_int, c_vp, c_int, c_int, c_int, c_vp, c_int, c_vp]),
    "svx_del_penalty": (c_int, [c_vp, c_vp, c_i64, c_f64, c_vp]),
    "svx_knob_sort": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "svx_dense_traceback": (c_int,[c_vp, c_vp, c_int, c_int, c_vp, c_vp]),
    "svx_sparse_traceback": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "svx_search_path": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp]),
    "svx_gather_rows": (c_int, [c_vp, c_vp, c_i64, c_int, c_int, c_vp, c_i64, c_vp]),
    "svx_unit_rows": (c_int, [c_vp, c_vp, c_int, c_i64, c_int, c_vp, c_int]),
    "svx_knn_mean_sim": (c_int, [c_vp, c_vp, c_int, c_i64, c_vp, c_int, c_i64, c_int, c_int, c_vp]),
    "svx_knn_topk_merge": (c_int, [c_vp, c_vp, c_int, c_i64, c_vp, c_int, c_i64, c_int, c_int, c_vp, c_int, c_vp]),
    "svx_knn_search": (c_int, [c_vp, c_vp, c_int, c_i64, c_vp, c_int, c_i64, c_int, c_int, c_i64, c_vp, c_vp, c_int]),
    "svx_knn_search_groups": (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_int, c_vp, c_vp]),
    "svx_margin_scores": (c_int, [c_vp, c_vp, c_vp, c_int, c_i64, c_int, c_vp, c_vp, c_int, c_vp]),
    "svx_knn_list_means": (c_int, [c_vp, c_vp, c_i64, c_int, c_vp]),
    "svx_margin_candidates": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_i64, c_i64, c_int, c_vp, c_vp, c_vp]),
    "svx_mine_greedy": (c_i64, [c_vp, c_i64, c_vp, c_vp, c_i64, c_i64, c_vp]),
    "svx_mt19937_choice": (c_int, [c_vp, ctypes.POINTER(ctypes.c_int32), c_i64, c_i64, c_vp]),
    "svx_norm_index_count": (c_i64, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "svx_knob_index_count": (c_i64, [c_int, c_int, c_int, c_int]),
    "svx_draw_indices": (c_int, [c_vp, ctypes.POINTER(ctypes.c_int32), c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                 c_vp, c_vp]),
    "svx_candidate_table": (c_int, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, c_int, c_vp, c_int,
                                    ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(c_i64), ctypes.c_char_p, c_int]),
    "svx_format_alignments": (c_i64, [c_vp, c_vp, c_i64, c_vp, c_i64]),
    "svx_num_levels": (c_int, [c_int, c_int, c_int]),
    "svx_knob_count": (c_i64, [c_int, c_int, c_int]),
    "svx_align_batch": (c_int, [c_vp, ctypes.POINTER(AlignParams), ctypes.POINTER(Pair), c_int]),
    "svx_align_around": (c_int, [c_vp, ctypes.POINTER(AlignParams), ctypes.POINTER(Pair), ctypes.POINTER(Prior), c_int]),
    "svx_time_prior": (c_int, [c_vp, ctypes.POINTER(Pair), ctypes.POINTER(Frames), c_int, c_i64, c_i64, ctypes.POINTER(Prior)]),
    "svx_prior_width": (c_int, [c_vp, ctypes.POINTER(Pair), ctypes.POINTER(Prior), c_int, c_vp]),
    "svx_band_contact": (c_int, [c_vp, c_int, c_int, c_vp]),
    "svx_align_widen": (c_int, [c_vp, ctypes.POINTER(AlignParams), ctypes.POINTER(Pair), ctypes.POINTER(Prior), c_int,
                                ctypes.POINTER(WidenParams), c_vp]),
    "svx_score_alignments": (c_int, [c_vp, ctypes.POINTER(Given), c_int]),
    "svx_row_slack": (c_int, [c_vp, ctypes.POINTER(c_vp), c_vp, c_int]),
    "svx_row_slack_wide": (c_int, [c_vp, ctypes.POINTER(SlackWide), c_vp, c_int]),
    "svx_row_alternatives": (c_int, [c_vp, ctypes.POINTER(Alt), c_int, c_f64, c_vp, c_int]),
    "svx_path_alternatives": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, ctypes.POINTER(ctypes.c_int32), c_int, c_f64, c_int, c_int,
                                      c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, ctypes.POINTER(Alt), c_int, c_f64]),
    "svx_alignment_rows": (c_int, [c_vp, c_int, c_int, ctypes.POINTER(Pair), c_int, c_f64, c_i64, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp]),
    "svx_concat_rows": (c_int, [c_vp, c_int, c_int, ctypes.POINTER(Pair), ctypes.POINTER(Frames), c_int, ctypes.POINTER(ConcatParams), c_i64,
                                c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp]),
    "svx_debug_level": (c_int, [c_vp, c_int, c_int, ctypes.POINTER(LevelView)]),
    "svx_copy_to_host": (c_int, [c_vp, c_vp, c_vp, c_i64]),
    "svx_set_profiling": (c_int, [c_vp, c_int]),
    "svx_set_pipeline": (c_int, [c_vp, c_int]),
    "svx_flush": (c_int, [c_vp]),
    "svx_stage_ms": (c_f64, [c_vp, ctypes.c_char_p]),
    "svx_stage_launches": (c_int, [c_vp, ctypes.c_char_p]),
}

EXPORTS = tuple(_SIGS)

_lib = None
_lock = threading.Lock()


def load():
    """Load libsvx.so (built by __graft_entry__.build() / `make -C speech-vecalign_amd/csrc`)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ImportError(
                    "libsvx.so not found at %s: build it with `make -C speech-vecalign_amd/csrc` "
                    "(there is no CPU fallback)" % LIB_PATH)
            L = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in _SIGS.items():
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


class SvxError(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class Context:
    """One svx_ctx per (process, device)."""

    def __init__(self, device=0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("svx needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
        self.lib = load()
        self.device = int(device)
        h = c_vp()
        rc = self.lib.svx_create(self.device, ctypes.byref(h))
        if rc != 0:
            raise SvxError(rc, self.lib.svx_last_error(None).decode())
        self.h = h
        self.torch = torch
        self.tdev = torch.device("cuda", self.device)
        self.pipeline = False
        # the stream handle use_current_stream() bound last (a new context is on the default stream, 0).  A caller who drives
        # svx_set_stream through ctypes leaves it stale; the only consequence is one extra clearing of _held, after a
        # flush the C side has done anyway
        self._bound = 0
        self._held = []   # batches whose device work the pipeline may still hold back: kept alive until the next flush
        if os.environ.get("SVX_PIPELINE") == "1":   # default for this process (the GPU suite is also run once this way)
            self.set_pipeline(True)

    def use_current_stream(self):
        """Bind torch's current stream (include/svx.h: svx_set_stream).  On a change the C side flushes the pipeline under
        the old binding and makes the new stream wait for everything the context did on the old one."""
        handle = int(self.torch.cuda.current_stream(self.tdev).cuda_stream)
        self.check(self.lib.svx_set_stream(self.h, c_vp(handle)))   # (the same handle again: one pointer compare)
        if handle != self._bound:
            self._bound = handle
            del self._held[:]   # flushed by the C side, as in flush()

    def current(self):
        """This context, bound to torch's current stream: the first line of every entry that launches on a context it did
        not just take from context()."""
        self.use_current_stream()
        return self

    def check(self, rc):
        if rc != 0:
            msg = self.lib.svx_last_error(self.h).decode()
            if rc == SVX_ERR_OVERLAPS:
                raise Exception(msg)  # the reference raises a plain Exception with this text
            raise SvxError(rc, msg)

    def sync(self):
        self.use_current_stream()
        self.check(self.lib.svx_synchronize(self.h))
        del self._held[:]

    def set_pipeline(self, on):
        """Software pipeline over consecutive svx_align_batch calls (include/svx.h: svx_set_pipeline); while it is on,
        outputs are complete only after flush() / sync()."""
        if self._held:   # svx_set_pipeline flushes only on a change of state: the held batches may still have a queued second half
            self.flush()
        self.check(self.lib.svx_set_pipeline(self.h, 1 if on else 0))
        self.pipeline = bool(on)

    def flush(self):
        self.use_current_stream()   # (a flush under another stream than the batch's: joined there, then this one waits)
        self.check(self.lib.svx_flush(self.h))
        # everything the pipeline held back is now ordered in front of whatever follows on the current stream, so memory
        # released from here on is reused behind it
        del self._held[:]

    def hold(self, batch):
        """The pipeline reads a batch's tensors on internal streams the tensor library knows nothing about, possibly
        during the NEXT call: keep the last few batches alive until a flush."""
        if self.pipeline and not any(b is batch for b in self._held):   # (a batch that is run again and again counts once)
            if len(self._held) >= 4:
                self.flush()
            self._held.append(batch)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.svx_destroy(self.h)
                self.h = None
        except Exception:
            pass


_ctxs = {}


def context(device=None):
    """The svx context of `device` (default: torch's current device, so that a process that called
    torch.cuda.set_device(LOCAL_RANK) works on its own GPU without passing the index around)."""
    if device is None:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("svx needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
        device = torch.cuda.current_device()
    device = int(device)
    if device not in _ctxs:
        _ctxs[device] = Context(device)
    c = _ctxs[device]
    c.use_current_stream()
    return c
