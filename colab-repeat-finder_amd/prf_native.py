"""ctypes binding of libprf.so (C ABI in include/prf.h) -- the only door to the GPU.

There is no CPU fallback behind this module: if the shared library is missing, or no gfx950
device is usable, the calls raise.  PyTorch is not involved; the library owns its device
memory and its HIP stream.
"""
import ctypes
import operator
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PRF_LIB", os.path.join(_HERE, "libprf.so"))  # PRF_LIB: diagnostic builds only

PRF_OK = 0
PRF_EINVAL = -1
PRF_ENODEV = -2
PRF_EHIP = -3
PRF_ENOMEM = -4
PRF_EUNSUPPORTED = -5
PRF_ESYMBOL = -6
PRF_EINDEX = -7

SCAN_DEFAULT = 0
SCAN_FORCE_GENERIC = 1
SCAN_NO_FETCH = 2
SCAN_DEFER_TIMING = 4
TIMING_RING = 128


class PrfError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"libprf error {code}: {message}")
        self.code = code
        self.message = message


class _Contig(ctypes.Structure):
    _fields_ = [("ascii", ctypes.c_void_p), ("len", ctypes.c_uint64)]


class _Part(ctypes.Structure):
    _fields_ = [("contig", ctypes.c_uint32), ("begin", ctypes.c_uint64), ("end", ctypes.c_uint64)]


class _Hit(ctypes.Structure):
    _fields_ = [("start", ctypes.c_uint64), ("end", ctypes.c_uint64), ("k", ctypes.c_uint32), ("contig", ctypes.c_uint32)]


class _Hits(ctypes.Structure):
    _fields_ = [("rows", ctypes.POINTER(_Hit)), ("n", ctypes.c_uint64)]


class _IHit(ctypes.Structure):
    _fields_ = [("start", ctypes.c_uint64), ("end", ctypes.c_uint64), ("k", ctypes.c_uint32), ("contig", ctypes.c_uint32),
                ("nmask", ctypes.c_uint64)]


class _IHits(ctypes.Structure):
    _fields_ = [("rows", ctypes.POINTER(_IHit)), ("n", ctypes.c_uint64)]


IHIT_DTYPE = [("start", "<u8"), ("end", "<u8"), ("k", "<u4"), ("contig", "<u4"), ("nmask", "<u8")]
MEMO_STRIDE = 8
MEMO_SLOTS = 1 << 22
INT_CHUNK = 1 << 20    # PRF_INT_CHUNK: landing positions per lane of the chunked interrupted walk
INT_CHUNK_MIN = 2      # PRF_INT_CHUNK_MIN


class ScanStats(ctypes.Structure):
    _fields_ = [("scan_ms", ctypes.c_double), ("phase1_ms", ctypes.c_double), ("phase2_ms", ctypes.c_double),
                ("positions", ctypes.c_uint64), ("packed_bytes", ctypes.c_uint64), ("n_candidates", ctypes.c_uint64),
                ("n_hits", ctypes.c_uint64), ("n_launches", ctypes.c_uint32), ("path", ctypes.c_uint32),
                ("seq", ctypes.c_uint64), ("sorted_on_device", ctypes.c_uint32), ("tiles_launched", ctypes.c_uint32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


def interruption_budgets(kmin, kmax, max_interruptions, by_k, ignore_other_k=False):
    """The budget of varying phases of every motif size kmin .. kmax as a list (entry j: k = kmin + j).  by_k: a dict {k: m} --
    a k it omits takes max_interruptions; a key outside kmin .. kmax is a ValueError unless ignore_other_k -- or a sequence with
    one entry per motif size; a sequence names every k, so a max_interruptions other than 0 that disagrees with one of its
    entries is a ValueError.  A negative or non-integer budget is a ValueError."""
    if kmin < 1 or kmax < kmin:
        raise ValueError(f"motif sizes {kmin} .. {kmax}: an empty range")
    scalar = max_interruptions or 0
    if isinstance(by_k, dict):
        other = sorted(k for k in by_k if not (isinstance(k, int) and kmin <= k <= kmax))
        if other and not ignore_other_k:
            raise ValueError(f"max_interruptions_by_k names motif size {other[0]}, outside {kmin} .. {kmax}")
        out = [by_k.get(k, scalar) for k in range(kmin, kmax + 1)]
    else:
        out = list(by_k)
        if len(out) != kmax - kmin + 1:
            raise ValueError(f"max_interruptions_by_k has {len(out)} entries for the {kmax - kmin + 1} motif sizes {kmin} .. {kmax}")
        if scalar and any(m != scalar for m in out):
            raise ValueError(f"max_interruptions is {scalar} and max_interruptions_by_k gives another budget: pass one of them, or 0")
    for j, m in enumerate(out):
        try:
            out[j] = operator.index(m)
        except TypeError:
            out[j] = -1
        if isinstance(m, bool) or not 0 <= out[j] <= 0xFFFFFFFF:
            raise ValueError(f"max_interruptions for motif size {kmin + j} is set to {m}. It must be at least 0.")
    return out


EXPORTS = ["prf_abi_version", "prf_device_count", "prf_last_error", "prf_open", "prf_close", "prf_genome_load",
           "prf_genome_free", "prf_genome_positions", "prf_scan_genome", "prf_scan", "prf_free_hits",
           "prf_measure_hbm_read", "prf_last_hits_to_device", "prf_plan_describe", "prf_fasta_open", "prf_fasta_count",
           "prf_fasta_entry", "prf_fasta_close", "prf_write_bed", "prf_write_tsv", "prf_genome_synth", "prf_scan_timings", "prf_set_row_sink", "prf_fasta_open_contig", "prf_scan_genome_async",
           "prf_scan_wait", "prf_genome_standin", "prf_genome_select", "prf_genome_tile_classes", "prf_tile_positions", "prf_scan_timings_split", "prf_last_hits_packed_to_device",
           "prf_genome_contig_bases", "prf_scan_literal", "prf_scan_genome_async_packed", "prf_stream_wait_for",
           "prf_genome_footprint", "prf_scan_interrupted", "prf_scan_interrupted_ex", "prf_free_ihits",
           "prf_scan_interrupted_chunked", "prf_scan_interrupted_by_k"]
# the periodicity entry points (include/prf_period.h, which prf.h includes)
PERIOD_EXPORTS = ["prf_period_counts", "prf_period_bits", "prf_period_counts_seq", "prf_period_bits_seq"]
# the dot-plot entry points (include/prf_dotplot.h, which prf.h includes)
DOTPLOT_EXPORTS = ["prf_dotplot_bits", "prf_dotplot_counts", "prf_dotplot_bits_ex", "prf_dotplot_counts_ex", "prf_dotplot_bits_seq",
                   "prf_dotplot_counts_seq", "prf_dotplot_shape"]
# the entry points of the dot plot of two ranges (include/prf_dotpair.h, which prf.h includes)
DOTPAIR_EXPORTS = ["prf_dotpair_bits", "prf_dotpair_counts", "prf_dotpair_bits_ex", "prf_dotpair_counts_ex", "prf_dotpair_bits_seq",
                   "prf_dotpair_counts_seq"]
# the entry points of the list of diagonal runs of that dot plot (include/prf_dotruns.h, which prf.h includes)
DOTRUNS_EXPORTS = ["prf_dotpair_runs", "prf_dotpair_runs_ex", "prf_dotpair_runs_seq"]
DOTRUN_DTYPE = [("row", "<u8"), ("col", "<u8"), ("len", "<u8"), ("dir", "<u4"), ("reserved", "<u4")]   # prf_dotrun, 32 bytes
DOTRUN_MAIN, DOTRUN_ANTI = 1, 2      # prf_dotrun.dir, and the bits of `directions`
DOTRUN_MAX_ROWS = 1 << 24            # PRF_DOTRUN_MAX_ROWS
DOTRUN_LONG_ROWS = 1 << 20           # PRF_DOTRUN_LONG_ROWS
DOTRUN_PROBE = 16                    # PRF_DOTRUN_PROBE
DOTRUN_FOLLOW = 2048                 # PRF_DOTRUN_FOLLOW
DOTRUN_DEFAULT_CAPACITY = 1 << 16    # rows the first of the binding's two calls has room for
# the entry points of the list of those runs chained across mismatches (include/prf_dotchain.h, which prf.h includes)
DOTCHAIN_EXPORTS = ["prf_dotpair_chains", "prf_dotpair_chains_ex", "prf_dotpair_chains_seq"]
DOTCHAIN_DTYPE = [("row", "<u8"), ("col", "<u8"), ("len", "<u8"), ("matches", "<u8"), ("dir", "<u4"), ("seeds", "<u4")]   # prf_dotchain, 40 bytes
DOTCHAIN_MAX_GAP = 4096              # PRF_DOTCHAIN_MAX_GAP
DOTCHAIN_MAX_ROWS = 1 << 24          # PRF_DOTCHAIN_MAX_ROWS
DOTCHAIN_LONG_ROWS = 1 << 20         # PRF_DOTCHAIN_LONG_ROWS
DOTCHAIN_FOLLOW = 2048               # PRF_DOTCHAIN_FOLLOW
DOTCHAIN_DEFAULT_CAPACITY = 1 << 16  # rows the first of the binding's two calls has room for
# the entry points of the list of junctions between those chains (include/prf_dotlink.h, which prf.h includes)
DOTLINK_EXPORTS = ["prf_dotpair_links", "prf_dotpair_links_ex", "prf_dotpair_links_seq"]
DOTLINK_DTYPE = [("row", "<u8"), ("col", "<u8"), ("from_row", "<u8"), ("from_col", "<u8"), ("dir", "<u4"), ("shift", "<i4"),
                 ("gap", "<u4"), ("overlap", "<u4")]   # prf_dotlink, 48 bytes
DOTLINK_MAX_SHIFT = 32               # PRF_DOTLINK_MAX_SHIFT
DOTLINK_OVERLAP = 16                 # PRF_DOTLINK_OVERLAP
DOTLINK_DEFAULT_CAPACITY = 1 << 16   # rows the first of the binding's two calls has room for
# one row of join_chains per group of chains joined by links
DOTGROUP_DTYPE = [("row", "<u8"), ("col", "<u8"), ("end_row", "<u8"), ("end_col", "<u8"), ("span_a", "<u8"), ("span_b", "<u8"),
                  ("matches", "<u8"), ("gap_cells", "<u8"), ("dir", "<u4"), ("chains", "<u4"), ("seeds", "<u4"), ("indel", "<u4"),
                  ("open", "?")]
# the entry points of the list of diverged tandem repeats: chains on the period lines of one range (include/prf_periodchain.h,
# which prf.h includes)
PERIODCHAIN_EXPORTS = ["prf_period_chains", "prf_period_chains_ex", "prf_period_chains_seq"]
PCHAIN_DTYPE = [("start", "<u8"), ("len", "<u8"), ("matches", "<u8"), ("k", "<u4"), ("seeds", "<u4")]   # prf_pchain, 32 bytes
PCHAIN_MAX_ROWS = 1 << 24            # PRF_PCHAIN_MAX_ROWS
PCHAIN_LONG_ROWS = 1 << 20           # PRF_PCHAIN_LONG_ROWS
PCHAIN_DEFAULT_CAPACITY = 1 << 16    # rows the first of the binding's two calls has room for
# the entry points of the list of junctions between those chains across neighbouring period lines (include/prf_periodlink.h,
# which prf.h includes)
PERIODLINK_EXPORTS = ["prf_period_links", "prf_period_links_ex", "prf_period_links_seq"]
PLINK_DTYPE = [("start", "<u8"), ("from_end", "<u8"), ("k", "<u4"), ("shift", "<i4"), ("gap", "<u4"), ("overlap", "<u4")]   # prf_plink, 32 bytes
PLINK_DEFAULT_CAPACITY = 1 << 16     # rows the first of the binding's two calls has room for
# one row of join_period_chains per group of period chains joined by links
PGROUP_DTYPE = [("start", "<u8"), ("end", "<u8"), ("span_a", "<u8"), ("span_b", "<u8"), ("matches", "<u8"), ("gap_cells", "<u8"),
                ("k_first", "<u4"), ("k_min", "<u4"), ("k_max", "<u4"), ("period", "<u4"), ("chains", "<u4"), ("seeds", "<u4"),
                ("indel", "<u4"), ("net_shift", "<i4"), ("open", "?")]
# one row of tandem_groups per gapped repeat
TANDEM_GROUP_DTYPE = [("start", "<u8"), ("end", "<u8"), ("period", "<u4"), ("copies", "<f8"), ("identity", "<f8"), ("indel", "<u4"),
                      ("chains", "<u4"), ("seeds", "<u4")]
# one row of tandem_rows per repeat
TANDEM_DTYPE = [("start", "<u8"), ("end", "<u8"), ("k", "<u4"), ("copies", "<f8"), ("identity", "<f8"), ("matches", "<u8"),
                ("seeds", "<u4")]
# the entry points of the consensus motifs of such repeats (include/prf_consensus.h, which prf.h includes)
CONSENSUS_EXPORTS = ["prf_period_consensus", "prf_period_consensus_ex", "prf_period_consensus_seq"]
REPEAT_DTYPE = [("start", "<u8"), ("end", "<u8"), ("k", "<u4"), ("reserved", "<u4")]                         # prf_repeat, 24 bytes
CONSENSUS_DTYPE = [("offset", "<u8"), ("agree", "<u8"), ("acgt", "<u8"), ("k", "<u4"), ("reserved", "<u4")]  # prf_consensus, 32 bytes
CONSENSUS_MAX_ROWS = 1 << 24         # PRF_CONSENSUS_MAX_ROWS
CONSENSUS_MAX_LETTERS = 1 << 26      # PRF_CONSENSUS_MAX_LETTERS: the sum of k per call
CONSENSUS_SLICE = 4096               # PRF_CONSENSUS_SLICE: positions per work item by default (an unmeasured guess)
# one row of consensus_rows per repeat: TANDEM_DTYPE and what the consensus adds
TANDEM_CONSENSUS_DTYPE = TANDEM_DTYPE + [("consensus_identity", "<f8"), ("primitive", "<u4")]
# the entry points of the consensus motifs over segments with a phase (include/prf_phased.h, which prf.h includes)
PHASED_EXPORTS = ["prf_phased_consensus", "prf_phased_consensus_ex", "prf_phased_consensus_seq"]
SEGMENT_DTYPE = [("start", "<u8"), ("end", "<u8"), ("row", "<u4"), ("phase", "<u4")]                          # prf_segment, 24 bytes
PHASED_MAX_SEGMENTS = 1 << 24        # PRF_PHASED_MAX_SEGMENTS
# one row of group_segments' pieces per consensus row of a gapped repeat
PIECE_DTYPE = [("group", "<u8"), ("anchor", "<u8"), ("end", "<u8"), ("k", "<u4"), ("segments", "<u4"), ("positions", "<u8")]
# one row of group_consensus_rows per gapped repeat: TANDEM_GROUP_DTYPE and what the consensus of its largest piece adds
GROUP_CONSENSUS_DTYPE = TANDEM_GROUP_DTYPE + [("consensus_identity", "<f8"), ("primitive", "<u4"), ("pieces", "<u4"), ("covered", "<f8")]
# the entry points of the alignment of repeats to their motifs (include/prf_align.h, which prf.h includes)
ALIGN_EXPORTS = ["prf_motif_align", "prf_motif_align_seq"]
ALIGNMENT_DTYPE = [("edits", "<u4"), ("indels", "<u4"), ("consumed", "<u4"), ("start_column", "<u4"), ("end_column", "<u4"),
                   ("reserved", "<u4")]                                                                       # prf_alignment, 24 bytes
ALIGN_MAX_K = 1024                   # PRF_ALIGN_MAX_K
ALIGN_MAX_LEN = 1 << 19              # PRF_ALIGN_MAX_LEN: positions per repeat
# what alignment_rows appends to its rows
ALIGNED_FIELDS = [("edits", "<u4"), ("subs", "<u4"), ("ins", "<u4"), ("del", "<u4"), ("aligned_matches", "<u4"),
                  ("aligned_identity", "<f8"), ("aligned_copies", "<f8")]
# the entry points of the alignment with its path (include/prf_alignpath.h, which prf.h includes)
ALIGNPATH_EXPORTS = ["prf_motif_align_path", "prf_motif_align_path_ex", "prf_motif_align_path_seq"]
ALIGNPATH_MAX_POSITIONS = 1 << 30    # PRF_ALIGNPATH_MAX_POSITIONS: entries of one call's path
PATH_INS = 0x8000                    # PRF_PATH_INS: the position is an insertion behind the entry's column
PATH_SUB = 0x4000                    # PRF_PATH_SUB: the position is aligned to the entry's column and does not match it
PATH_COLUMN = 0x03FF                 # PRF_PATH_COLUMN
# what path_copies returns per copy
PATH_COPY_DTYPE = [("copy", "<u4"), ("start", "<u8"), ("end", "<u8"), ("subs", "<u4"), ("ins", "<u4"), ("dels", "<u4")]
# the entry points of the local alignment of windows to motifs (include/prf_alignlocal.h, which prf.h includes)
ALIGNLOCAL_EXPORTS = ["prf_motif_align_local", "prf_motif_align_local_seq"]
LOCAL_ALIGNMENT_DTYPE = [("score", "<u4"), ("first", "<u4"), ("end", "<u4"), ("start_column", "<u4"), ("end_column", "<u4"),
                         ("reserved", "<u4")]                                                                 # prf_local_alignment, 24 bytes
ALIGNLOCAL_MAX_WEIGHT = 16           # PRF_ALIGNLOCAL_MAX_WEIGHT: each of match, mismatch, indel
# what local_rows appends to its rows
LOCAL_FIELDS = [("local_start", "<u8"), ("local_end", "<u8"), ("score", "<u4")]
DIRECTIONS = {"main": 1, "anti": 2, "both": 3}
DOT_LAUNCH_CELLS = 1 << 36   # PRF_DOT_LAUNCH_CELLS
DOT_MAX_CELLS = 1 << 42      # PRF_DOT_MAX_CELLS
DOT_MAX_RUN = 64             # PRF_DOT_MAX_RUN

_lib = None
_lib_lock = threading.Lock()


class _HostOnly:
    """A library that exports only the host-side entry points (FASTA reader, BED/TSV writers, planner): the prototypes of the
    others are accepted and dropped, calling one raises.  Test infrastructure (tests/test_asan_host.py), selected by
    PRF_LIB_HOST_ONLY=1 together with PRF_LIB."""

    class _Absent:
        def __init__(self, name):
            self._name = name

        def __call__(self, *args):
            raise ImportError(f"{self._name} is not part of the host-only build")

    def __init__(self, cdll):
        self._cdll = cdll

    def __getattr__(self, name):
        try:
            f = getattr(self._cdll, name)
        except AttributeError:
            f = _HostOnly._Absent(name)
        self.__dict__[name] = f
        return f


def load_library():
    """dlopen libprf.so and declare the prototypes.  Raises if the library was not built."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(make -C colab-repeat-finder_amd/csrc).  There is no CPU fallback.")
        lib = ctypes.CDLL(LIB_PATH)
        if os.environ.get("PRF_LIB_HOST_ONLY") == "1":
            lib = _HostOnly(lib)      # the sanitizer build of the host-only parts (make asan): the GPU entry points are absent
        vp = ctypes.c_void_p
        lib.prf_abi_version.restype = ctypes.c_int
        lib.prf_device_count.restype = ctypes.c_int
        lib.prf_last_error.restype = ctypes.c_char_p
        lib.prf_open.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        lib.prf_close.argtypes = [vp]
        lib.prf_close.restype = None
        lib.prf_genome_load.argtypes = [vp, ctypes.POINTER(_Contig), ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(vp)]
        lib.prf_genome_synth.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.c_int,
                                         ctypes.c_uint32, ctypes.POINTER(vp)]
        lib.prf_genome_standin.argtypes = lib.prf_genome_synth.argtypes
        lib.prf_tile_positions.restype = ctypes.c_uint64
        lib.prf_genome_select.argtypes = [vp, ctypes.POINTER(_Part), ctypes.c_int]
        lib.prf_genome_tile_classes.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
        lib.prf_genome_free.argtypes = [vp]
        lib.prf_genome_free.restype = None
        lib.prf_genome_positions.argtypes = [vp]
        lib.prf_genome_positions.restype = ctypes.c_uint64
        lib.prf_scan_genome.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                        ctypes.c_uint32, ctypes.POINTER(_Hits), ctypes.POINTER(ScanStats)]
        lib.prf_scan.argtypes = [vp, ctypes.POINTER(_Contig), ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                 ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_Hits),
                                 ctypes.POINTER(ScanStats)]
        lib.prf_scan_literal.argtypes = [vp, ctypes.POINTER(_Contig), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                         ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(_Hits), ctypes.POINTER(ScanStats)]
        lib.prf_free_hits.argtypes = [ctypes.POINTER(_Hits)]
        lib.prf_scan_interrupted.argtypes = [vp, ctypes.POINTER(_Contig), ctypes.c_int] + [ctypes.c_uint32] * 5 + [
            ctypes.POINTER(_IHits), ctypes.POINTER(ScanStats)]
        lib.prf_scan_interrupted_ex.argtypes = [vp, ctypes.POINTER(_Contig), ctypes.c_int] + [ctypes.c_uint32] * 6 + [
            ctypes.c_uint64, ctypes.POINTER(_IHits), ctypes.POINTER(ScanStats), ctypes.POINTER(ctypes.c_uint64)]
        lib.prf_scan_interrupted_chunked.argtypes = [vp, ctypes.POINTER(_Contig), ctypes.c_int] + [ctypes.c_uint32] * 6 + [
            ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(_IHits), ctypes.POINTER(ScanStats), ctypes.POINTER(ctypes.c_uint64)]
        lib.prf_scan_interrupted_by_k.argtypes = [vp, ctypes.POINTER(_Contig), ctypes.c_int] + [ctypes.c_uint32] * 4 + [
            ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(_IHits),
            ctypes.POINTER(ScanStats), ctypes.POINTER(ctypes.c_uint64)]
        lib.prf_free_ihits.argtypes = [ctypes.POINTER(_IHits)]
        u64p = ctypes.POINTER(ctypes.c_uint64)
        lib.prf_period_counts.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.c_uint64, vp, ctypes.c_uint64, u64p, ctypes.POINTER(ScanStats)]
        lib.prf_period_bits.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                        vp, ctypes.c_uint64, u64p, ctypes.POINTER(ScanStats)]
        lib.prf_period_counts_seq.argtypes = [vp, ctypes.POINTER(_Contig), ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                              ctypes.c_uint32, ctypes.c_uint64, vp, ctypes.c_uint64, u64p, ctypes.POINTER(ScanStats)]
        lib.prf_period_bits_seq.argtypes = [vp, ctypes.POINTER(_Contig), ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                            ctypes.c_uint32, vp, ctypes.c_uint64, u64p, ctypes.POINTER(ScanStats)]
        window = [ctypes.c_uint64] * 6 + [ctypes.c_uint32]          # begin, end, row0, row1, col0, col1, min_diagonal_run
        bits_tail = [vp, ctypes.c_uint64, u64p, ctypes.POINTER(ScanStats)]
        counts_tail = [ctypes.c_uint64, vp, ctypes.c_uint64, u64p, u64p, ctypes.POINTER(ScanStats)]
        lib.prf_dotplot_bits.argtypes = [vp, vp, ctypes.c_uint32] + window + bits_tail
        lib.prf_dotplot_counts.argtypes = [vp, vp, ctypes.c_uint32] + window + counts_tail
        lib.prf_dotplot_bits_ex.argtypes = [vp, vp, ctypes.c_uint32] + window + bits_tail + [ctypes.c_uint64]
        lib.prf_dotplot_counts_ex.argtypes = [vp, vp, ctypes.c_uint32] + window + counts_tail + [ctypes.c_uint64]
        lib.prf_dotplot_bits_seq.argtypes = [vp, ctypes.POINTER(_Contig)] + window + bits_tail
        lib.prf_dotplot_counts_seq.argtypes = [vp, ctypes.POINTER(_Contig)] + window + counts_tail
        lib.prf_dotplot_shape.argtypes = [ctypes.c_uint32] + [ctypes.POINTER(ctypes.c_uint32)] * 3
        span = [ctypes.c_uint64] * 2                                # begin, end
        pair_window = [ctypes.c_uint32] + window[2:]                # strand, row0, row1, col0, col1, min_diagonal_run
        on_genome = [vp, vp, ctypes.c_uint32] + span + [ctypes.c_uint32] + span + pair_window
        one_shot = [vp, ctypes.POINTER(_Contig)] + span + [ctypes.POINTER(_Contig)] + span + pair_window
        lib.prf_dotpair_bits.argtypes = on_genome + bits_tail
        lib.prf_dotpair_counts.argtypes = on_genome + counts_tail
        lib.prf_dotpair_bits_ex.argtypes = on_genome + bits_tail + [ctypes.c_uint64]
        lib.prf_dotpair_counts_ex.argtypes = on_genome + counts_tail + [ctypes.c_uint64]
        lib.prf_dotpair_bits_seq.argtypes = one_shot + bits_tail
        lib.prf_dotpair_counts_seq.argtypes = one_shot + counts_tail
        runs_tail = [ctypes.c_uint32] + [ctypes.c_uint64] * 4 + [ctypes.c_uint32, ctypes.c_uint64, vp, ctypes.c_uint64, u64p,
                                                                 ctypes.POINTER(ScanStats)]   # strand, window, directions, min_len ...
        lib.prf_dotpair_runs.argtypes = on_genome[:-6] + runs_tail
        lib.prf_dotpair_runs_ex.argtypes = on_genome[:-6] + runs_tail + [ctypes.c_uint64]
        lib.prf_dotpair_runs_seq.argtypes = one_shot[:-6] + runs_tail
        chains_tail = runs_tail[:6] + [ctypes.c_uint64, ctypes.c_uint32] + runs_tail[6:]   # ... directions, min_seed, max_gap, min_len ...
        lib.prf_dotpair_chains.argtypes = on_genome[:-6] + chains_tail
        lib.prf_dotpair_chains_ex.argtypes = on_genome[:-6] + chains_tail + [ctypes.c_uint64]
        lib.prf_dotpair_chains_seq.argtypes = one_shot[:-6] + chains_tail
        links_tail = runs_tail[:6] + [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32] + runs_tail[7:]   # ... min_seed, max_gap, max_shift ...
        lib.prf_dotpair_links.argtypes = on_genome[:-6] + links_tail
        lib.prf_dotpair_links_ex.argtypes = on_genome[:-6] + links_tail + [ctypes.c_uint64]
        lib.prf_dotpair_links_seq.argtypes = one_shot[:-6] + links_tail
        # begin, end, pos0, pos1, kmin, kmax, n_matches, min_seed, max_gap, min_len, dst, capacity, n_chains, stats
        pchains_tail = [ctypes.c_uint64] * 4 + [ctypes.c_uint32] * 3 + [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, vp,
                                                                        ctypes.c_uint64, u64p, ctypes.POINTER(ScanStats)]
        lib.prf_period_chains.argtypes = [vp, vp, ctypes.c_uint32] + pchains_tail
        lib.prf_period_chains_ex.argtypes = [vp, vp, ctypes.c_uint32] + pchains_tail + [ctypes.c_uint64]
        lib.prf_period_chains_seq.argtypes = [vp, ctypes.POINTER(_Contig)] + pchains_tail
        plinks_tail = pchains_tail[:9] + [ctypes.c_uint32] + pchains_tail[10:]     # ... max_gap, max_shift, dst, capacity, n_links, stats
        lib.prf_period_links.argtypes = [vp, vp, ctypes.c_uint32] + plinks_tail
        lib.prf_period_links_ex.argtypes = [vp, vp, ctypes.c_uint32] + plinks_tail + [ctypes.c_uint64]
        lib.prf_period_links_seq.argtypes = [vp, ctypes.POINTER(_Contig)] + plinks_tail
        # begin, end, rows, n_rows, dst, motifs, letters_capacity, counts, stats
        consensus_tail = [ctypes.c_uint64] * 2 + [vp, ctypes.c_uint64, vp, vp, ctypes.c_uint64, vp, ctypes.POINTER(ScanStats)]
        lib.prf_period_consensus.argtypes = [vp, vp, ctypes.c_uint32] + consensus_tail
        lib.prf_period_consensus_ex.argtypes = [vp, vp, ctypes.c_uint32] + consensus_tail + [ctypes.c_uint64]
        lib.prf_period_consensus_seq.argtypes = [vp, ctypes.POINTER(_Contig)] + consensus_tail
        # begin, end, ks, n_rows, segments, n_segments, dst, motifs, letters_capacity, counts, stats
        phased_tail = consensus_tail[:4] + [vp, ctypes.c_uint64] + consensus_tail[4:]
        lib.prf_phased_consensus.argtypes = [vp, vp, ctypes.c_uint32] + phased_tail
        lib.prf_phased_consensus_ex.argtypes = [vp, vp, ctypes.c_uint32] + phased_tail + [ctypes.c_uint64]
        lib.prf_phased_consensus_seq.argtypes = [vp, ctypes.POINTER(_Contig)] + phased_tail
        # begin, end, rows, n_rows, motifs, letters_length, dst, stats
        align_tail = [ctypes.c_uint64] * 2 + [vp, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64, vp, ctypes.POINTER(ScanStats)]
        lib.prf_motif_align.argtypes = [vp, vp, ctypes.c_uint32] + align_tail
        lib.prf_motif_align_seq.argtypes = [vp, ctypes.POINTER(_Contig)] + align_tail
        path_tail = align_tail[:-1] + [vp, ctypes.c_uint64, vp, ctypes.POINTER(ScanStats)]
        lib.prf_motif_align_path.argtypes = [vp, vp, ctypes.c_uint32] + path_tail
        lib.prf_motif_align_path_ex.argtypes = [vp, vp, ctypes.c_uint32] + path_tail + [ctypes.c_uint64]
        lib.prf_motif_align_path_seq.argtypes = [vp, ctypes.POINTER(_Contig)] + path_tail
        # begin, end, rows, n_rows, motifs, letters_length, match, mismatch, indel, dst, stats
        local_tail = align_tail[:6] + [ctypes.c_uint32] * 3 + align_tail[6:]
        lib.prf_motif_align_local.argtypes = [vp, vp, ctypes.c_uint32] + local_tail
        lib.prf_motif_align_local_seq.argtypes = [vp, ctypes.POINTER(_Contig)] + local_tail
        lib.prf_free_ihits.restype = None
        lib.prf_free_hits.restype = None
        lib.prf_measure_hbm_read.argtypes = [vp, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
        lib.prf_last_hits_to_device.argtypes = [vp, vp, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
        lib.prf_set_row_sink.argtypes = [vp, vp, ctypes.c_uint64]
        lib.prf_last_hits_packed_to_device.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
        lib.prf_genome_contig_bases.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
        lib.prf_genome_footprint.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        lib.prf_scan_genome_async.argtypes = [vp, vp] + [ctypes.c_uint32] * 4 + [ctypes.POINTER(ctypes.c_uint64)]
        lib.prf_scan_genome_async_packed.argtypes = [vp, vp] + [ctypes.c_uint32] * 4 + [vp, ctypes.c_uint64, ctypes.c_uint64,
                                                                                         ctypes.POINTER(ctypes.c_uint64)]
        lib.prf_stream_wait_for.argtypes = [vp, vp]
        lib.prf_scan_wait.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(ScanStats)]
        lib.prf_scan_timings.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_float)]
        lib.prf_scan_timings_split.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_float),
                                               ctypes.POINTER(ctypes.c_float)]
        lib.prf_plan_describe.argtypes = [ctypes.c_uint32] * 4 + [ctypes.c_char_p, ctypes.c_uint64]
        lib.prf_fasta_open.argtypes = [ctypes.c_char_p, ctypes.POINTER(vp)]
        lib.prf_fasta_open_contig.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(vp)]
        lib.prf_fasta_count.argtypes = [vp]
        lib.prf_fasta_entry.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp),
                                        ctypes.POINTER(ctypes.c_uint64)]
        lib.prf_fasta_close.argtypes = [vp]
        lib.prf_fasta_close.restype = None
        lib.prf_write_bed.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(_Contig),
                                      ctypes.c_int, ctypes.POINTER(_Hits), ctypes.POINTER(ctypes.c_uint64)]
        lib.prf_write_tsv.argtypes = [ctypes.c_char_p, ctypes.POINTER(_Contig), ctypes.POINTER(_Hits),
                                      ctypes.POINTER(ctypes.c_uint64)]
        _lib = lib
        return lib


def _check(lib, rc):
    if rc != PRF_OK:
        raise PrfError(rc, lib.prf_last_error().decode("utf-8", "replace"))


def _contig_array(seqs):
    """(array, keep-alive list).  seqs: bytes objects, or (address, length) pairs of memory that outlives the call."""
    arr = (_Contig * max(1, len(seqs)))()
    keep = []
    for i, s in enumerate(seqs):
        if isinstance(s, tuple):
            arr[i].ascii, arr[i].len = s
            continue
        if isinstance(s, bytearray):
            s = bytes(s)
        if not isinstance(s, bytes):
            raise TypeError("contigs must be bytes")
        keep.append(s)
        arr[i].ascii = ctypes.cast(ctypes.c_char_p(s), ctypes.c_void_p)
        arr[i].len = len(s)
    return arr, keep


def _rows(hits):
    n = hits.n
    if n == 0:
        return []
    import numpy as np
    buf = np.ctypeslib.as_array(ctypes.cast(hits.rows, ctypes.POINTER(ctypes.c_uint8)), shape=(n * ctypes.sizeof(_Hit),))
    rec = buf.view(np.dtype([("start", "<u8"), ("end", "<u8"), ("k", "<u4"), ("contig", "<u4")])).copy()
    return rec


END_OF_CONTIG = (1 << 64) - 1   # period_counts / period_bits: `end` beyond any contig, clipped by the library to its length


def _period_check(kmin, kmax, window):
    if kmin < 1 or kmax < kmin:
        raise ValueError(f"motif sizes {kmin} .. {kmax}: an empty range")
    if window is not None and (window < 64 or window % 64):
        raise ValueError(f"window is {window}. It must be a multiple of 64, at least 64.")


def _clip(begin, end, length):
    """(positions of [begin, end) of a sequence of `length` positions, `end` as the library takes it).  end None: the length."""
    stop = length if end is None else min(end, length)
    if begin < 0 or begin > (stop if end is None else end):
        raise ValueError(f"begin {begin} is behind end {stop if end is None else end}")
    return max(0, stop - begin), END_OF_CONTIG if end is None else end


def _matrix_call(lib, shape, dtype, n_sizes, call):
    """The output array dtype[shape] of a periodicity or dot-plot call, filled by call(dst, capacity, *size pointers, stats); the
    n_sizes size words the library publishes are the last n_sizes entries of shape.  Returns (array, stats)."""
    import numpy as np
    total = shape[0] * shape[1]
    out = np.zeros(max(1, total), dtype=dtype)
    sizes, stats = [ctypes.c_uint64(0) for _ in range(n_sizes)], ScanStats()
    _check(lib, call(out.ctypes.data_as(ctypes.c_void_p), total, *[ctypes.byref(n) for n in sizes], ctypes.byref(stats)))
    assert tuple(n.value for n in sizes) == shape[-n_sizes:], ([n.value for n in sizes], shape)
    return out[:total].reshape(shape), stats


def dotplot_shape(min_diagonal_run=3):
    """(rows per workgroup tile, 64-column words per workgroup span, halo rows) of a dot-plot launch (prf_dotplot_shape; host
    only; the same for genomes with and without letters outside ACGTN): tile and span boundaries of a window lie at multiples of these from its first row and column."""
    lib = load_library()
    out = [ctypes.c_uint32(0) for _ in range(3)]
    _check(lib, lib.prf_dotplot_shape(min_diagonal_run, *[ctypes.byref(v) for v in out]))
    return tuple(v.value for v in out)


def unpack_bits(bits, n_columns):
    """uint8[rows, n_columns] of 0 / 1 from packed rows (bit j of word w = column 64 w + j): dotplot_bits, period_bits."""
    import numpy as np
    bits = np.ascontiguousarray(bits, dtype="<u8")
    rows = bits.shape[0]
    if rows == 0 or n_columns == 0:
        return np.zeros((rows, n_columns), dtype=np.uint8)
    return np.unpackbits(bits.view(np.uint8).reshape(rows, -1), axis=1, bitorder="little")[:, :n_columns]


def _dot_window(n_rows, n_cols, rows, cols, min_diagonal_run, block):
    """((row0, row1, col0, col1) as given to the library, (rows, columns) of the clipped window) after the binding's checks, for a
    matrix of n_rows x n_cols."""
    if isinstance(min_diagonal_run, bool) or not 0 <= operator.index(min_diagonal_run) <= 0xFFFFFFFF:
        raise ValueError(f"min_diagonal_run is set to {min_diagonal_run}. It must be at least 0.")
    if block is not None and (block < 64 or block % 64 or block > 32768):
        raise ValueError(f"block is {block}. It must be a multiple of 64, at least 64 and at most 32768.")
    out = []
    for name, pair in (("rows", rows), ("cols", cols)):
        lo, hi = (0, None) if pair is None else pair
        if lo < 0 or (hi is not None and lo > hi):
            raise ValueError(f"{name} {lo} .. {hi}: an empty range is given as lo == hi")
        out.append((lo, END_OF_CONTIG if hi is None else hi))
    clipped = [max(0, min(hi, length) - min(lo, length)) for (lo, hi), length in zip(out, (n_rows, n_cols))]
    return (out[0][0], out[0][1], out[1][0], out[1][1]), tuple(clipped)


STRANDS = {"+": 0, "-": 1}     # the strand argument of the dotpair calls


def _matrix_range(target, begin, end):
    """(what the library is given in front of the range, positions of the clipped range, `end` as the library takes it, what must
    stay alive during the call: None for a genome) for a target that is (genome, contig) or one sequence (str or bytes)."""
    if isinstance(target, tuple):
        genome, contig = target
        if genome.lens is None or not 0 <= contig < len(genome.lens):
            raise ValueError(f"contig {contig}: the genome holds {genome.n_contigs}")
        where, length, keep = (contig,), genome.lens[contig], None
    else:
        seq = target.encode("ascii", "replace") if isinstance(target, str) else target
        arr, keep = _contig_array([seq])
        where, length = (arr,), len(seq)
    n, c_end = _clip(begin, end, length)
    return where, n, c_end, keep


def _matrix(ctx, target, begin, end, with_stats, period=None, dot=None, versus=None):
    """The one path of the periodicity and dot-plot calls.  target: (genome, contig), or one sequence (str or bytes) for the
    one-shot _seq entry points.  period: (kmin, kmax, window); dot: (min_diagonal_run, block, rows, cols, launch_cells); window
    or block None: the bits.  versus: (target, begin, end, strand) of the columns' range, which turns the dot plot into the one
    of two ranges (target of the same kind; a genome must be the same one).  Returns the array, or (array, ScanStats) with_stats."""
    import numpy as np
    if period is not None:
        _period_check(*period)
    where, n, c_end, keep = _matrix_range(target, begin, end)
    one_shot = keep is not None
    form, tail = ("_seq" if one_shot else ""), ()
    if not one_shot:
        where = (target[0]._h,) + where
    if period is not None:
        kmin, kmax, unit = period
        product, args = "period", (begin, c_end, kmin, kmax)
        shape, n_sizes = (kmax - kmin + 1, -(-n // (64 if unit is None else unit))), 1
    else:
        t, unit, rows, cols, launch_cells = dot
        product, args, n_b = "dotplot", (begin, c_end), n
        if versus is not None:
            b_target, b_begin, b_end, strand = versus
            if strand not in STRANDS:
                raise ValueError(f"strand is {strand!r}. It must be '+' or '-'.")
            if one_shot == isinstance(b_target, tuple):
                raise ValueError("the two ranges must both be sequences or both lie in a genome")
            if not one_shot and b_target[0] is not target[0]:
                raise ValueError("the two ranges must lie in the same resident genome")
            b_where, n_b, b_c_end, _b_keep = _matrix_range(b_target, b_begin, b_end)
            product, args = "dotpair", args + b_where + (b_begin, b_c_end, STRANDS[strand])
        win, (n_rows, n_cols) = _dot_window(n, n_b, rows, cols, t, unit)
        args += win + (t,)
        if not form:                                      # on a genome: the _ex forms, which take launch_cells
            form, tail = "_ex", (launch_cells,)
        shape, n_sizes = ((n_rows, -(-n_cols // 64)), 1) if unit is None else ((-(-n_rows // unit), -(-n_cols // unit)), 2)
    if unit is not None:
        args += (unit,)
    fn = getattr(ctx.lib, f"prf_{product}_{'bits' if unit is None else 'counts'}{form}")
    out, stats = _matrix_call(ctx.lib, shape, np.uint64 if unit is None else np.uint32, n_sizes,
                              lambda *out_args: fn(ctx._h, *where, *args, *out_args, *tail))
    return (out, stats) if with_stats else out


def _int_check(name, value, lo, hi=None):
    """Refuses a value that is no integer (a bool is none) of lo .. hi; hi None: no upper bound."""
    if isinstance(value, bool) or operator.index(value) < lo or (hi is not None and operator.index(value) > hi):
        raise ValueError(f"{name} is set to {value}. It must be " + (f"at least {lo}." if hi is None else f"{lo} .. {hi}."))


def _list_entry(ctx, name, genome, launch_cells):
    """(entry point, what it is given in front of the ranges, what behind the stats) of a list product: the one-shot _seq form for
    sequences (genome None), the _ex form, which takes launch_cells, on a genome."""
    if genome is None:
        return getattr(ctx.lib, name + "_seq"), (ctx._h,), ()
    return getattr(ctx.lib, name + "_ex"), (ctx._h, genome._h), (launch_cells,)


def _pair_list_args(ctx, name, a_target, a_range, b_target, b_range, strand, directions, params, rows, cols, launch_cells):
    """(entry point, head, args, tail, what must stay alive during the call) of a list product of the dot plot of two ranges: the
    targets are (genome, contig) pairs of one genome, or two sequences.  params: (name, value, lo, hi) of the integers the entry
    point takes behind `directions`, in its order, checked in that order."""
    if strand not in STRANDS:
        raise ValueError(f"strand is {strand!r}. It must be '+' or '-'.")
    if directions not in DIRECTIONS:
        raise ValueError(f"directions is {directions!r}. It must be 'main', 'anti' or 'both'.")
    for param in params:
        _int_check(*param)
    one_shot = not isinstance(a_target, tuple)
    if one_shot == isinstance(b_target, tuple):
        raise ValueError("the two ranges must both be sequences or both lie in a genome")
    if not one_shot and b_target[0] is not a_target[0]:
        raise ValueError("the two ranges must lie in the same resident genome")
    a_where, na, a_end, a_keep = _matrix_range(a_target, *a_range)
    b_where, nb, b_end, b_keep = _matrix_range(b_target, *b_range)
    win, _ = _dot_window(na, nb, rows, cols, 0, None)
    args = a_where + (a_range[0], a_end) + b_where + (b_range[0], b_end, STRANDS[strand]) + win + (DIRECTIONS[directions],)
    fn, head, tail = _list_entry(ctx, name, None if one_shot else a_target[0], launch_cells)
    return fn, head, args + tuple(param[1] for param in params), tail, (a_keep, b_keep)


def _period_list_args(ctx, name, target, begin, end, kmin, kmax, params, n_matches, positions, launch_cells):
    """The same of a list product of the period lines of a range: target is (genome, contig) or one sequence.  params: the integers
    behind `n_matches`."""
    if isinstance(kmin, bool) or isinstance(kmax, bool) or not 1 <= operator.index(kmin) <= operator.index(kmax) <= 0xFFFFFFFF:
        raise ValueError(f"periods {kmin} .. {kmax}: an empty range")
    for param in params:
        _int_check(*param)
    lo, hi = (0, None) if positions is None else positions
    if lo < 0 or (hi is not None and lo > hi):
        raise ValueError(f"positions {lo} .. {hi}: an empty range is given as lo == hi")
    where, _n, c_end, keep = _matrix_range(target, begin, end)
    args = where + (begin, c_end, lo, END_OF_CONTIG if hi is None else hi, kmin, kmax, 1 if n_matches else 0)
    fn, head, tail = _list_entry(ctx, name, None if keep is not None else target[0], launch_cells)
    return fn, head, args + tuple(param[1] for param in params), tail, keep


def _list_call(ctx, fn, head, args, tail, dtype, capacity, max_rows, noun, advice, with_stats, fields=None):
    """The one path of the list products: calls once with `capacity` rows of room and once more with the exact number if there were
    more.  Returns the rows (their `fields`, or all), or (rows, ScanStats) with_stats."""
    import numpy as np
    while True:
        out = np.zeros(max(1, capacity), dtype=dtype)
        n, stats = ctypes.c_uint64(0), ScanStats()
        _check(ctx.lib, fn(*head, *args, out.ctypes.data_as(ctypes.c_void_p), capacity, ctypes.byref(n), ctypes.byref(stats), *tail))
        if n.value <= capacity:
            break
        if n.value > max_rows:
            raise PrfError(PRF_EUNSUPPORTED, f"{n.value} {noun} are more than one call returns ({max_rows}): ask for a larger {advice}")
        capacity = n.value
    rows = (out[:n.value] if fields is None else out[:n.value][fields]).copy()
    return (rows, stats) if with_stats else rows


def _runs(ctx, a_target, a_range, b_target, b_range, strand, directions, min_len, rows, cols, with_stats, launch_cells):
    """The dotpair_runs calls; the rows lose their reserved field."""
    *call, _keep = _pair_list_args(ctx, "prf_dotpair_runs", a_target, a_range, b_target, b_range, strand, directions,
                                   [("min_len", min_len, 1)], rows, cols, launch_cells)
    return _list_call(ctx, *call, DOTRUN_DTYPE, DOTRUN_DEFAULT_CAPACITY, DOTRUN_MAX_ROWS, "runs", "min_len or for smaller windows",
                      with_stats, ["row", "col", "len", "dir"])


def _chains(ctx, a_target, a_range, b_target, b_range, strand, directions, min_seed, max_gap, min_len, rows, cols, with_stats,
            launch_cells):
    """The dotpair_chains calls."""
    *call, _keep = _pair_list_args(ctx, "prf_dotpair_chains", a_target, a_range, b_target, b_range, strand, directions,
                                   [("min_seed", min_seed, 1), ("max_gap", max_gap, 0, DOTCHAIN_MAX_GAP), ("min_len", min_len, 0)],
                                   rows, cols, launch_cells)
    return _list_call(ctx, *call, DOTCHAIN_DTYPE, DOTCHAIN_DEFAULT_CAPACITY, DOTCHAIN_MAX_ROWS, "chains",
                      "min_seed or min_len or for smaller windows", with_stats)


def _links(ctx, a_target, a_range, b_target, b_range, strand, directions, min_seed, max_gap, max_shift, rows, cols, with_stats,
           launch_cells):
    """The dotpair_links calls."""
    *call, _keep = _pair_list_args(ctx, "prf_dotpair_links", a_target, a_range, b_target, b_range, strand, directions,
                                   [("min_seed", min_seed, 1), ("max_gap", max_gap, 0, DOTCHAIN_MAX_GAP),
                                    ("max_shift", max_shift, 1, DOTLINK_MAX_SHIFT)], rows, cols, launch_cells)
    return _list_call(ctx, *call, DOTLINK_DTYPE, DOTLINK_DEFAULT_CAPACITY, DOTCHAIN_MAX_ROWS, "links", "min_seed or for smaller windows",
                      with_stats)


def _period_chains(ctx, target, begin, end, kmin, kmax, min_seed, max_gap, min_len, n_matches, positions, with_stats, launch_cells):
    """The period_chains calls."""
    *call, _keep = _period_list_args(ctx, "prf_period_chains", target, begin, end, kmin, kmax,
                                     [("min_seed", min_seed, 1), ("max_gap", max_gap, 0, DOTCHAIN_MAX_GAP), ("min_len", min_len, 0)],
                                     n_matches, positions, launch_cells)
    return _list_call(ctx, *call, PCHAIN_DTYPE, PCHAIN_DEFAULT_CAPACITY, PCHAIN_MAX_ROWS, "chains",
                      "min_seed or min_len, fewer periods or fewer positions", with_stats)


def _period_links(ctx, target, begin, end, kmin, kmax, min_seed, max_gap, max_shift, n_matches, positions, with_stats, launch_cells):
    """The period_links calls."""
    *call, _keep = _period_list_args(ctx, "prf_period_links", target, begin, end, kmin, kmax,
                                     [("min_seed", min_seed, 1), ("max_gap", max_gap, 0, DOTCHAIN_MAX_GAP),
                                      ("max_shift", max_shift, 1, DOTLINK_MAX_SHIFT)], n_matches, positions, launch_cells)
    return _list_call(ctx, *call, PLINK_DTYPE, PLINK_DEFAULT_CAPACITY, PCHAIN_MAX_ROWS, "links",
                      "min_seed, fewer periods or fewer positions", with_stats)


def _repeat_table(target, begin, end, repeats, slice_positions=0):
    """The argument checks that the calls over repeats (start, end, k) share.  Returns (what the library is given in front of the
    range, `end` as the library takes it, what must stay alive during the call, the rows as REPEAT_DTYPE, their number, the sum of
    k)."""
    import numpy as np
    try:
        start, stop, k = (np.asarray(repeats[name]) for name in ("start", "end", "k"))
    except (KeyError, ValueError, IndexError, TypeError):
        raise ValueError("repeats must be a structured array with the fields start, end and k") from None
    _int_check("slice_positions", slice_positions, 0)
    n_rows = len(start)
    if n_rows > CONSENSUS_MAX_ROWS:
        raise ValueError(f"{n_rows} repeats are more than one call takes ({CONSENSUS_MAX_ROWS}): send them in batches")
    where, n, c_end, keep = _matrix_range(target, begin, end)
    rows = np.zeros(max(1, n_rows), dtype=REPEAT_DTYPE)
    letters = 0
    if n_rows:
        if (k < 1).any() or (k > 0xFFFFFFFF).any():
            raise ValueError(f"repeat {int(np.argmax((k < 1) | (k > 0xFFFFFFFF)))}: k must be at least 1")
        bad = (start < 0) | (start >= stop) | (stop > n)
        if bad.any():
            at = int(np.argmax(bad))
            raise ValueError(f"repeat {at}: [{start[at]}, {stop[at]}) is not a stretch of the range's {n} positions")
        rows["start"][:n_rows], rows["end"][:n_rows], rows["k"][:n_rows] = start, stop, k
        letters = int(rows["k"][:n_rows].sum(dtype=np.uint64))
        if letters > CONSENSUS_MAX_LETTERS:
            raise ValueError(f"the k of the repeats add up to {letters}, more than one call takes ({CONSENSUS_MAX_LETTERS}): send them in batches")
    return where, c_end, keep, rows, n_rows, letters


def _period_consensus(ctx, target, begin, end, repeats, counts, with_stats, slice_positions):
    """The period_consensus calls.  target: (genome, contig) or one sequence.  Returns (rows of CONSENSUS_DTYPE, list of str), then
    the counts as an array of (sum of k, 4) if asked, then the ScanStats with_stats."""
    import numpy as np
    where, c_end, keep, rows, n_rows, letters = _repeat_table(target, begin, end, repeats, slice_positions)
    out = np.zeros(max(1, n_rows), dtype=CONSENSUS_DTYPE)
    motifs = np.zeros(max(1, letters), dtype=np.uint8)
    table = np.zeros((max(1, letters), 4), dtype=np.uint32) if counts else None
    stats = ScanStats()
    if keep is not None:
        fn, head, tail = ctx.lib.prf_period_consensus_seq, (ctx._h,), ()
    else:
        fn, head, tail = ctx.lib.prf_period_consensus_ex, (ctx._h, target[0]._h), (slice_positions,)
    _check(ctx.lib, fn(*head, *where, begin, c_end, rows.ctypes.data, n_rows, out.ctypes.data, motifs.ctypes.data, letters,
                       table.ctypes.data if counts else None, ctypes.byref(stats), *tail))
    text = motifs[:letters].tobytes().decode("ascii")
    got = out[:n_rows].copy()
    result = (got, [text[o:o + kk] for o, kk in zip(got["offset"].tolist(), got["k"].tolist())])
    if counts:
        result += (table[:letters],)
    return result + (stats,) if with_stats else result


def _phased_consensus(ctx, target, begin, end, ks, segments, counts, with_stats, slice_positions):
    """The phased_consensus calls.  target: (genome, contig) or one sequence.  Returns what _period_consensus returns."""
    import numpy as np
    try:
        k = np.asarray(ks)
        if k.ndim != 1 or (len(k) and k.dtype.kind not in "iu"):
            raise TypeError
    except (ValueError, TypeError):
        raise ValueError("ks must be a sequence of integers, one k per row") from None
    try:
        start, stop, row, phase = (np.asarray(segments[name]) for name in ("start", "end", "row", "phase"))
    except (KeyError, ValueError, IndexError, TypeError):
        raise ValueError("segments must be a structured array with the fields start, end, row and phase") from None
    _int_check("slice_positions", slice_positions, 0)
    n_rows, n_segments = len(k), len(start)
    if n_rows > CONSENSUS_MAX_ROWS:
        raise ValueError(f"{n_rows} rows are more than one call takes ({CONSENSUS_MAX_ROWS}): send them in batches")
    if n_segments > PHASED_MAX_SEGMENTS:
        raise ValueError(f"{n_segments} segments are more than one call takes ({PHASED_MAX_SEGMENTS}): send them in batches")
    where, n, c_end, keep = _matrix_range(target, begin, end)
    widths = np.zeros(max(1, n_rows), dtype=np.uint32)
    table = np.zeros(max(1, n_segments), dtype=SEGMENT_DTYPE)
    letters = 0
    if n_rows:
        if (k < 1).any() or (k > 0xFFFFFFFF).any():
            raise ValueError(f"row {int(np.argmax((k < 1) | (k > 0xFFFFFFFF)))}: k must be at least 1")
        widths[:n_rows] = k
        letters = int(widths[:n_rows].sum(dtype=np.uint64))
        if letters > CONSENSUS_MAX_LETTERS:
            raise ValueError(f"the k of the rows add up to {letters}, more than one call takes ({CONSENSUS_MAX_LETTERS}): send them in batches")
    if n_segments:
        bad = (start < 0) | (start >= stop) | (stop > n)
        if bad.any():
            at = int(np.argmax(bad))
            raise ValueError(f"segment {at}: [{start[at]}, {stop[at]}) is not a stretch of the range's {n} positions")
        bad = (row < 0) | (row >= n_rows)
        if bad.any():
            at = int(np.argmax(bad))
            raise ValueError(f"segment {at}: row {row[at]} is not one of the {n_rows} rows")
        bad = (phase < 0) | (phase >= widths[:n_rows][row.astype(np.int64)])
        if bad.any():
            at = int(np.argmax(bad))
            raise ValueError(f"segment {at}: phase {phase[at]} is not below the k = {widths[int(row[at])]} of row {row[at]}")
        table["start"], table["end"], table["row"], table["phase"] = start, stop, row, phase
    out = np.zeros(max(1, n_rows), dtype=CONSENSUS_DTYPE)
    motifs = np.zeros(max(1, letters), dtype=np.uint8)
    sums = np.zeros((max(1, letters), 4), dtype=np.uint32) if counts else None
    stats = ScanStats()
    if keep is not None:
        fn, head, tail = ctx.lib.prf_phased_consensus_seq, (ctx._h,), ()
    else:
        fn, head, tail = ctx.lib.prf_phased_consensus_ex, (ctx._h, target[0]._h), (slice_positions,)
    _check(ctx.lib, fn(*head, *where, begin, c_end, widths.ctypes.data, n_rows, table.ctypes.data, n_segments, out.ctypes.data,
                       motifs.ctypes.data, letters, sums.ctypes.data if counts else None, ctypes.byref(stats), *tail))
    text = motifs[:letters].tobytes().decode("ascii")
    got = out[:n_rows].copy()
    result = (got, [text[o:o + kk] for o, kk in zip(got["offset"].tolist(), got["k"].tolist())])
    if counts:
        result += (sums[:letters],)
    return result + (stats,) if with_stats else result


def _motif_letters(motifs, ks):
    """The motifs of rows of these k as one buffer of letters: a list of str, one per row, or the letters (str or bytes) that a
    consensus call returned, which are checked for their length only -- the library names a letter it does not take."""
    if isinstance(motifs, (str, bytes, bytearray)):
        text = motifs.encode("ascii", "replace") if isinstance(motifs, str) else bytes(motifs)
        if len(text) != sum(ks):
            raise ValueError(f"the motifs hold {len(text)} letters, the k of the repeats add up to {sum(ks)}")
        return text
    try:
        parts = list(motifs)
    except TypeError:
        parts = [None]
    if not all(isinstance(m, (str, bytes, bytearray)) for m in parts):
        raise ValueError("motifs must be a list of str, one per repeat, or the letters a consensus call returned")
    parts = [m.encode("ascii", "replace") if isinstance(m, str) else bytes(m) for m in parts]
    if len(parts) != len(ks):
        raise ValueError(f"{len(parts)} motifs for {len(ks)} repeats")
    for at, (m, k) in enumerate(zip(parts, ks)):
        if len(m) != k:
            raise ValueError(f"repeat {at}: the motif has {len(m)} letters, k is {k}")
    return b"".join(parts)


def _motif_align(ctx, target, begin, end, repeats, motifs, with_stats):
    """The motif_align calls.  target: (genome, contig) or one sequence.  Returns the rows of ALIGNMENT_DTYPE, then the ScanStats
    with_stats."""
    import numpy as np
    where, c_end, keep, rows, n_rows, letters = _repeat_table(target, begin, end, repeats)
    if n_rows:
        k, length = rows["k"][:n_rows], rows["end"][:n_rows] - rows["start"][:n_rows]
        if (k > ALIGN_MAX_K).any():
            at = int(np.argmax(k > ALIGN_MAX_K))
            raise ValueError(f"repeat {at}: k = {k[at]} is more than an alignment takes ({ALIGN_MAX_K})")
        if (length > ALIGN_MAX_LEN).any():
            at = int(np.argmax(length > ALIGN_MAX_LEN))
            raise ValueError(f"repeat {at}: {length[at]} positions are more than an alignment takes ({ALIGN_MAX_LEN})")
    text = _motif_letters(motifs, rows["k"][:n_rows].tolist())
    out = np.zeros(max(1, n_rows), dtype=ALIGNMENT_DTYPE)
    stats = ScanStats()
    if keep is not None:
        fn, head = ctx.lib.prf_motif_align_seq, (ctx._h,)
    else:
        fn, head = ctx.lib.prf_motif_align, (ctx._h, target[0]._h)
    _check(ctx.lib, fn(*head, *where, begin, c_end, rows.ctypes.data, n_rows, text, len(text), out.ctypes.data, ctypes.byref(stats)))
    got = out[:n_rows].copy()
    return (got, stats) if with_stats else got


def alignment_rows(rows, align):
    """Rows with the fields start, end and k -- or period, as the rows of tandem_groups() and group_consensus_rows() call it --
    with what motif_align says of them, in their order: the fields of `rows`, then ALIGNED_FIELDS: edits, subs = edits - indels,
    ins = (indels + n - consumed) / 2, del = (indels - n + consumed) / 2, aligned_matches = n - subs - ins (the rows of
    tandem_rows() have a `matches` of their own: the chain's), aligned_identity = aligned_matches / (n + del) and aligned_copies =
    consumed / k, with n = end - start.  Host numpy."""
    import numpy as np
    k_field = "k" if "k" in rows.dtype.names else "period"
    if len(rows) != len(align):
        raise ValueError("alignment_rows needs the rows motif_align returned for these repeats")
    out = np.zeros(len(rows), dtype=rows.dtype.descr + ALIGNED_FIELDS)
    for name in rows.dtype.names:
        out[name] = rows[name]
    n = (rows["end"].astype(np.int64) - rows["start"].astype(np.int64))
    edits, indels, consumed = (align[f].astype(np.int64) for f in ("edits", "indels", "consumed"))
    if len(rows) and (((indels + n - consumed) % 2 != 0).any() or (consumed > n + indels).any() or (n > consumed + indels).any()):
        raise ValueError("alignment_rows needs the rows motif_align returned for these repeats")
    out["edits"], out["subs"] = edits, edits - indels
    out["ins"], out["del"] = (indels + n - consumed) // 2, (indels - n + consumed) // 2
    out["aligned_matches"] = n - out["subs"] - out["ins"]
    out["aligned_identity"] = out["aligned_matches"] / np.maximum(n + out["del"], 1)
    out["aligned_copies"] = consumed / np.maximum(rows[k_field].astype(np.int64), 1)
    return out


def _local_weights(match, mismatch, indel):
    for name, w in (("match", match), ("mismatch", mismatch), ("indel", indel)):
        _int_check(name, w, 1)
        if w > ALIGNLOCAL_MAX_WEIGHT:
            raise ValueError(f"{name} = {w} is more than a local alignment takes ({ALIGNLOCAL_MAX_WEIGHT})")
    return int(match), int(mismatch), int(indel)


def _motif_align_local(ctx, target, begin, end, repeats, motifs, match, mismatch, indel, with_stats):
    """The motif_align_local calls.  target: (genome, contig) or one sequence.  Returns the rows of LOCAL_ALIGNMENT_DTYPE, then
    the ScanStats with_stats."""
    import numpy as np
    weights = _local_weights(match, mismatch, indel)
    where, c_end, keep, rows, n_rows, letters = _repeat_table(target, begin, end, repeats)
    if n_rows:
        k, length = rows["k"][:n_rows], rows["end"][:n_rows] - rows["start"][:n_rows]
        if (k > ALIGN_MAX_K).any():
            at = int(np.argmax(k > ALIGN_MAX_K))
            raise ValueError(f"repeat {at}: k = {k[at]} is more than an alignment takes ({ALIGN_MAX_K})")
        if (length > ALIGN_MAX_LEN).any():
            at = int(np.argmax(length > ALIGN_MAX_LEN))
            raise ValueError(f"repeat {at}: {length[at]} positions are more than an alignment takes ({ALIGN_MAX_LEN})")
    text = _motif_letters(motifs, rows["k"][:n_rows].tolist())
    out = np.zeros(max(1, n_rows), dtype=LOCAL_ALIGNMENT_DTYPE)
    stats = ScanStats()
    if keep is not None:
        fn, head = ctx.lib.prf_motif_align_local_seq, (ctx._h,)
    else:
        fn, head = ctx.lib.prf_motif_align_local, (ctx._h, target[0]._h)
    _check(ctx.lib, fn(*head, *where, begin, c_end, rows.ctypes.data, n_rows, text, len(text), *weights, out.ctypes.data, ctypes.byref(stats)))
    got = out[:n_rows].copy()
    return (got, stats) if with_stats else got


def flank_repeats(repeats, flank, n):
    """The WINDOWS motif_align_local searches around found repeats: rows with the fields start, end and k -- or period -- of a
    range of n positions, each padded by `flank` on both sides and clipped to the range: (max(0, start - flank), min(n, end +
    flank), k) as REPEAT_DTYPE.  Where the window would hold more than ALIGN_MAX_LEN positions the flank is cut down to what
    fits, the same on both sides (one more in front if what fits is odd) before the clipping.  Returns (windows, sent): sent[i]
    is False for a row whose own length or k is above a limit (ALIGN_MAX_LEN, ALIGN_MAX_K); its window is the row itself and must
    not be sent.  Host numpy."""
    import numpy as np
    _int_check("flank", flank, 0)
    _int_check("n", n, 0)
    k_field = "k" if "k" in repeats.dtype.names else "period"
    start, stop, k = (repeats[name].astype(np.int64) for name in ("start", "end", k_field))
    if len(start) and ((start < 0) | (start >= stop) | (stop > n)).any():
        at = int(np.argmax((start < 0) | (start >= stop) | (stop > n)))
        raise ValueError(f"repeat {at}: [{start[at]}, {stop[at]}) is not a stretch of the range's {n} positions")
    length = stop - start
    sent = (length <= ALIGN_MAX_LEN) & (k <= ALIGN_MAX_K) & (k >= 1)
    room = np.clip(ALIGN_MAX_LEN - length, 0, 2 * int(flank))                   # what both flanks may add together
    behind = np.where(sent, np.minimum(int(flank), room // 2), 0)
    front = np.where(sent, np.minimum(int(flank), room - behind), 0)
    windows = np.zeros(len(start), dtype=REPEAT_DTYPE)
    windows["start"], windows["end"], windows["k"] = np.maximum(0, start - front), np.minimum(int(n), stop + behind), np.clip(k, 0, 0xFFFFFFFF)
    return windows, sent


def local_rows(rows, windows, local):
    """Rows with the fields start and end, with what motif_align_local says of their windows (flank_repeats), in their order: the
    fields of `rows`, then LOCAL_FIELDS: local_start = the window's start + first and local_end = the window's start + end,
    relative to the range like start and end, and score.  A row with score 0, or one not sent (flank_repeats; its row of `local`
    stays all zeros), keeps its own interval and score 0.  Host numpy."""
    import numpy as np
    if not len(rows) == len(windows) == len(local):
        raise ValueError("local_rows needs the windows of these rows and the rows motif_align_local returned for them")
    out = np.zeros(len(rows), dtype=rows.dtype.descr + LOCAL_FIELDS)
    for name in rows.dtype.names:
        out[name] = rows[name]
    score = local["score"].astype(np.int64)
    took = score > 0
    w_start = windows["start"].astype(np.int64)
    if len(rows) and took.any():
        first, end = local["first"].astype(np.int64), local["end"].astype(np.int64)
        if ((first >= end) | (w_start + end > windows["end"].astype(np.int64)))[took].any():
            raise ValueError("local_rows needs the windows of these rows and the rows motif_align_local returned for them")
    out["local_start"] = np.where(took, w_start + local["first"], rows["start"])
    out["local_end"] = np.where(took, w_start + local["end"], rows["end"])
    out["score"] = np.where(took, score, 0)
    return out


def _motif_align_path(ctx, target, begin, end, repeats, motifs, with_counts, with_stats, trace_bytes):
    """The motif_align_path calls.  target: (genome, contig) or one sequence.  Returns (rows of ALIGNMENT_DTYPE, the paths: one
    uint16 array per repeat, views of one buffer), then the counts as an array of (sum of k, 6) with_counts, then the ScanStats
    with_stats."""
    import numpy as np
    where, c_end, keep, rows, n_rows, letters = _repeat_table(target, begin, end, repeats)
    _int_check("trace_bytes", trace_bytes, 0)
    length = rows["end"][:n_rows] - rows["start"][:n_rows]
    if n_rows:
        k = rows["k"][:n_rows]
        if (k > ALIGN_MAX_K).any():
            at = int(np.argmax(k > ALIGN_MAX_K))
            raise ValueError(f"repeat {at}: k = {k[at]} is more than an alignment takes ({ALIGN_MAX_K})")
        if (length > ALIGN_MAX_LEN).any():
            at = int(np.argmax(length > ALIGN_MAX_LEN))
            raise ValueError(f"repeat {at}: {length[at]} positions are more than an alignment takes ({ALIGN_MAX_LEN})")
    positions = int(length.sum(dtype=np.uint64))
    if positions > ALIGNPATH_MAX_POSITIONS:
        raise ValueError(f"the repeats add up to {positions} positions, more than one call's path takes ({ALIGNPATH_MAX_POSITIONS}): send them in batches")
    text = _motif_letters(motifs, rows["k"][:n_rows].tolist())
    out = np.zeros(max(1, n_rows), dtype=ALIGNMENT_DTYPE)
    path = np.zeros(max(1, positions), dtype=np.uint16)
    table = np.zeros((max(1, letters), 6), dtype=np.uint32) if with_counts else None
    stats = ScanStats()
    tail = (begin, c_end, rows.ctypes.data, n_rows, text, len(text), out.ctypes.data, path.ctypes.data, positions,
            table.ctypes.data if with_counts else None, ctypes.byref(stats))
    if keep is not None:
        if trace_bytes:
            raise ValueError("trace_bytes belongs to a resident genome: the one-shot form has no such knob")
        rc = ctx.lib.prf_motif_align_path_seq(ctx._h, *where, *tail)
    else:
        rc = ctx.lib.prf_motif_align_path_ex(ctx._h, target[0]._h, *where, *tail, trace_bytes)
    _check(ctx.lib, rc)
    firsts = np.concatenate([[0], np.cumsum(length, dtype=np.uint64)]).astype(np.int64).tolist()
    result = (out[:n_rows].copy(), [path[firsts[at]:firsts[at + 1]] for at in range(n_rows)])
    if with_counts:
        result += (table[:letters],)
    return result + (stats,) if with_stats else result


def path_deletions(path_row, k):
    """Per position i of a row's path but the last, the number of deleted motif letters between i and i + 1, from the path alone:
    with state = path[i] & PATH_COLUMN, (c - 1 - state) mod k if i + 1 is aligned at column c, (c - state) mod k if it is an
    insertion with column c.  Host numpy."""
    import numpy as np
    p = np.asarray(path_row).astype(np.int64)
    state, col, ins = p[:-1] & PATH_COLUMN, p[1:] & PATH_COLUMN, (p[1:] & PATH_INS) != 0
    return np.where(ins, col - state, col - 1 - state) % int(k)


def path_cigar(path_row, k):
    """The CIGAR of a row's path: run lengths of = (match), X (substitution), I (insertion: a position against nothing) and
    D (deletion: motif letters against nothing, path_deletions), in the order of the positions.  Host numpy."""
    import numpy as np
    p = np.asarray(path_row).astype(np.int64)
    if not len(p):
        return ""
    ops = np.where(p & PATH_INS, ord("I"), np.where(p & PATH_SUB, ord("X"), ord("="))).astype(np.uint8)
    dels = np.concatenate([path_deletions(p, k), [0]])
    out, run_op, run = [], None, 0
    for op, d in zip(ops.tobytes().decode(), dels.tolist()):
        if op == run_op:
            run += 1
        else:
            if run:
                out.append(f"{run}{run_op}")
            run_op, run = op, 1
        if d:
            out.append(f"{run}{run_op}{d}D")
            run_op, run = None, 0
    if run:
        out.append(f"{run}{run_op}")
    return "".join(out)


def aligned_consensus(counts, motifs):
    """The motifs re-estimated from the aligned columns: per column the letter with the most aligned positions (counts[:, 0:4] of
    motif_align_path), ties in the order A, C, G, T; a column without any keeps its letter.  motifs: a list of str, or the letters
    in one str or bytes; the result has the same form (bytes come back as str).  Host numpy."""
    import numpy as np
    counts = np.asarray(counts)
    joined = isinstance(motifs, (str, bytes, bytearray))
    parts = [motifs] if joined else list(motifs)
    parts = [m if isinstance(m, str) else bytes(m).decode("ascii") for m in parts]
    text = "".join(parts)
    if counts.ndim != 2 or counts.shape[0] != len(text) or counts.shape[1] < 4:
        raise ValueError(f"aligned_consensus needs the counts motif_align_path returned for these motifs: {counts.shape} for {len(text)} letters")
    best = np.argmax(counts[:, :4], axis=1)                                   # the first of equal maxima
    keep = counts[:, :4].max(axis=1, initial=0) == 0
    new = np.where(keep, np.frombuffer(text.encode("ascii"), dtype=np.uint8), np.frombuffer(b"ACGT", dtype=np.uint8)[best])
    new = new.astype(np.uint8).tobytes().decode("ascii")
    if joined:
        return new
    out, at = [], 0
    for m in parts:
        out.append(new[at:at + len(m)])
        at += len(m)
    return out


def path_copies(path_row, start, k):
    """The copies of a row's alignment as rows of PATH_COPY_DTYPE (copy, start, end, subs, ins, dels): the positions are cut each
    time the path enters the row's start column (path[0] & PATH_COLUMN) by an aligned position; `start` is the row's first
    position, so start and end are positions of the range.  The deletions between two positions count with the copy of the position
    in front of them.  The rows add up to the row: its positions, its SUB and INS entries and its deletions.  Host numpy."""
    import numpy as np
    p = np.asarray(path_row).astype(np.int64)
    n = len(p)
    if not n:
        return np.zeros(0, dtype=PATH_COPY_DTYPE)
    aligned = (p & PATH_INS) == 0
    cuts = np.flatnonzero(aligned & ((p & PATH_COLUMN) == (p[0] & PATH_COLUMN)))
    cuts = cuts[cuts > 0]
    bounds = np.concatenate([[0], cuts, [n]])
    dels = np.concatenate([path_deletions(p, k), [0]])
    sub, ins = ((p & PATH_SUB) != 0) & aligned, ~aligned
    out = np.zeros(len(bounds) - 1, dtype=PATH_COPY_DTYPE)
    out["copy"] = np.arange(len(out))
    out["start"], out["end"] = bounds[:-1] + int(start), bounds[1:] + int(start)
    for field, what in (("subs", sub), ("ins", ins), ("dels", dels)):
        out[field] = np.add.reduceat(what.astype(np.int64), bounds[:-1])
    return out


def refine_motifs(target, contig, begin, end, repeats, motifs, rounds=2, trace_bytes=0):
    """TRF-style refinement: `rounds` times at most, align the repeats to their motifs (motif_align_path with counts) and take
    the aligned consensus as the new motifs; stops early when no motif changes.  target: a Genome (contig is its contig) or a
    Context (contig is then the sequence).  Returns (motifs as a list of str, the alignment of the last call, per repeat the
    number of rounds that changed its motif).  The alignment is that of the returned motifs: if the last round still changed a
    motif, the repeats are aligned once more."""
    import numpy as np
    _int_check("rounds", rounds, 1)
    ks = np.asarray(repeats["k"]).tolist()
    text = _motif_letters(motifs, ks).decode("ascii")
    offsets = np.concatenate([[0], np.cumsum(ks)]).astype(np.int64).tolist()
    current = [text[offsets[at]:offsets[at + 1]] for at in range(len(ks))]
    changed = np.zeros(len(ks), dtype=np.uint32)

    def call():
        if isinstance(target, Context):
            return target.motif_align_path(contig, repeats, current, begin, end, with_counts=True)
        return target.motif_align_path(contig, begin, end, repeats, current, with_counts=True, trace_bytes=trace_bytes)

    align, stale = None, True
    for _ in range(rounds):
        align, _paths, counts = call()
        new = aligned_consensus(counts, current)
        moved = np.array([a != b for a, b in zip(current, new)], dtype=bool)
        stale = bool(moved.any())
        if not stale:
            break
        changed += moved
        current = new
    if stale:
        align = call()[0]
    return current, align, changed


def _link_paths(chains, links):
    """(paths, link_out, is_open) of the chains of period_chains (min_len = 0) and the links of period_links of the same window
    and settings: every chain has at most one link in and one out, so the links form paths.  paths: one list of chain indices per
    path, in the order of the paths' first chains; link_out[x]: the index of the link that leaves chain x, or -1; is_open[y]: a
    link into chain y names a predecessor that is not in `chains`.  The one place where links are resolved to chains."""
    n = len(chains)
    start, length, line = (chains[f].astype("int64").tolist() for f in ("start", "len", "k"))
    first = {key: at for at, key in enumerate(zip(start, line))}
    last = {(s + l - 1, k): at for at, (s, l, k) in enumerate(zip(start, length, line))}
    nxt, link_out, has_in, is_open = [-1] * n, [-1] * n, [False] * n, [False] * n
    for at, (t_s, t_e, k, s) in enumerate(zip(*(links[f].tolist() for f in ("start", "from_end", "k", "shift")))):
        y = first.get((t_s, k))
        if y is None:
            raise ValueError(f"the link into (start {t_s}, k {k}) names a successor that is not in the list of chains: "
                             "join_period_chains needs the chains of the same window, range of k, min_seed and max_gap, fetched at min_len = 0")
        x = last.get((t_e, k - s))
        if x is None:
            is_open[y] = True
        else:
            nxt[x], link_out[x], has_in[y] = y, at, True
    paths = []
    for head in range(n):
        if has_in[head]:
            continue
        path, cur = [], head
        while cur >= 0:
            path.append(cur)
            cur = nxt[cur]
        paths.append(path)
    return paths, link_out, is_open


def period_paths(chains, links):
    """The paths join_period_chains folds into groups, in its order: one list of chain indices per group."""
    return _link_paths(chains, links)[0]


def group_segments(chains, links, joined=None):
    """The PHASED SEGMENTS of the gapped repeats of join_period_chains(chains, links) (the same inputs): what phased_consensus needs
    to name them.  joined: what join_period_chains(chains, links, with_paths=True) returned, if the caller has it (else the join
    is made here).  Returns (pieces, segments): rows of PIECE_DTYPE and of SEGMENT_DTYPE; segment.row indexes pieces, and the
    segments of a piece are consecutive, in ascending order, and disjoint.
    Per path, with P the group's period: only the chains on line P give positions, [start, start + len + P) each.  The first opens
    a PIECE, one consensus row of k = P whose column 0 is the piece's first position (anchor).  Between two consecutive on-period
    chains A and B of the path: exactly one chain Y with len_Y <= k_Y in between is an isolated indel of k_Y - P bases (negative: a
    deletion) -- B continues the piece, its columns moved by the piece's drift D += k_Y - P, and the inserted bases fall in no
    column; anything else (two or more chains in between, or a Y longer than its line) leaves the phase undecided: the piece ends
    and B opens a new one.  A chain's segment begins where the piece's previous segment ended if they overlap, and is dropped if
    nothing is left; its phase is (segment start - anchor - D) mod P.  Chains in front of the first or behind the last on-period
    chain give nothing.  pieces: group (the index into join_period_chains' rows), anchor, end (of the last segment), k,
    segments, positions (the sum of the segments' lengths).  Host numpy."""
    import numpy as np
    groups, paths = joined if joined is not None else join_period_chains(chains, links, with_paths=True)
    start, length, line = (chains[f].astype(np.int64).tolist() for f in ("start", "len", "k"))
    pieces, segments = [], []
    for at, (path, period) in enumerate(zip(paths, groups["period"].tolist())):
        on = [j for j, c in enumerate(path) if line[c] == period]
        piece = None                                           # [group, anchor, end, k, segments, positions], drift alongside
        drift = 0
        for prev, j in zip([None] + on[:-1], on):
            c = path[j]
            between = [] if prev is None else path[prev + 1:j]
            if piece is not None and len(between) == 1 and length[between[0]] <= line[between[0]]:
                drift += line[between[0]] - period
            else:
                piece, drift = [at, start[c], start[c], period, 0, 0], 0
                pieces.append(piece)
            lo, hi = max(start[c], piece[2]), start[c] + length[c] + period
            if lo >= hi:
                continue
            segments.append((lo, hi, len(pieces) - 1, (lo - piece[1] - drift) % period))
            piece[2], piece[4], piece[5] = hi, piece[4] + 1, piece[5] + hi - lo
    return (np.array([tuple(p) for p in pieces], dtype=PIECE_DTYPE).reshape(len(pieces)),
            np.array(segments, dtype=SEGMENT_DTYPE).reshape(len(segments)))


def group_consensus_rows(groups, pieces, cons, motifs):
    """The gapped repeats of tandem_groups(join_period_chains(...), drop_covered=False) -- or the rows of join_period_chains
    themselves -- with what phased_consensus says of the pieces group_segments cut them into.  Returns (rows of
    GROUP_CONSENSUS_DTYPE, motifs as a list of str), one per group, in their order: the fields of TANDEM_GROUP_DTYPE; the motif of
    the piece with the most positions (ties: the first); consensus_identity = agree / positions of that piece; primitive = the
    smallest period of that motif; pieces = the group's number of pieces; covered = the share of the group's [start, end) that
    the chosen piece's segments cover.  A group without a piece (no chain on its period line: none today) gets '', 0, 0, 0, 0."""
    import numpy as np
    if not (len(pieces) == len(cons) == len(motifs)) or (len(cons) and (cons["k"] != pieces["k"]).any()):
        raise ValueError("group_consensus_rows needs the rows phased_consensus returned for these pieces")
    if len(pieces) and int(pieces["group"].max()) >= len(groups):
        raise ValueError("group_consensus_rows needs the groups whose chains and links gave these pieces")
    out = np.zeros(len(groups), dtype=GROUP_CONSENSUS_DTYPE)
    for name, _ in TANDEM_GROUP_DTYPE:
        if name in ("copies", "identity") and name not in groups.dtype.names:
            continue
        out[name] = groups[name]
    if "copies" not in groups.dtype.names:
        plain = tandem_groups(groups, drop_covered=False)
        out["copies"], out["identity"] = plain["copies"], plain["identity"]
    best, names = {}, [""] * len(groups)
    for at, (g, n) in enumerate(zip(pieces["group"].tolist(), pieces["positions"].tolist())):
        out["pieces"][g] += 1
        if g not in best or n > best[g][1]:
            best[g] = (at, n)
    for g, (at, n) in best.items():
        span = int(groups["end"][g]) - int(groups["start"][g])
        names[g] = motifs[at]
        out["consensus_identity"][g] = int(cons["agree"][at]) / max(n, 1)
        out["primitive"][g] = primitive_period(motifs[at])
        out["covered"][g] = n / max(span, 1)
    return out, names


def primitive_period(motif):
    """The smallest divisor d of len(motif) for which the motif is d-periodic (motif == motif[:d] * (len / d))."""
    k = len(motif)
    for d in range(1, k + 1):
        if k % d == 0 and motif[:d] * (k // d) == motif:
            return d
    return 0


_COMPLEMENT = str.maketrans("ACGTN", "TGCAN")


def canonical_motif(motif):
    """The catalogue key of a motif over A, C, G, T, N: the lexicographically least string among the rotations of the motif and of
    its reverse complement (N pairs with N).  Two loci of one satellite, read from any phase and either strand, share it."""
    motif = motif.upper()
    if set(motif) - set("ACGTN"):
        raise ValueError(f"a motif over A, C, G, T, N is needed, not {motif!r}")
    if not motif:
        return motif
    best = None
    for text in (motif, motif.translate(_COMPLEMENT)[::-1]):
        twice = text + text
        least = min(twice[i:i + len(text)] for i in range(len(text)))
        best = least if best is None or least < best else best
    return best


def consensus_rows(tandem, cons, motifs):
    """The repeats of tandem_rows with what period_consensus says of them, one row of TANDEM_CONSENSUS_DTYPE each, in their order:
    the fields of TANDEM_DTYPE, consensus_identity = agree / (end - start) (copy against motif, where identity is copy against the
    copy in front) and primitive = the smallest period of the consensus motif itself.  Host numpy."""
    import numpy as np
    if not (len(tandem) == len(cons) == len(motifs)) or (len(cons) and (cons["k"] != tandem["k"]).any()):
        raise ValueError("consensus_rows needs the rows period_consensus returned for these repeats")
    out = np.zeros(len(tandem), dtype=TANDEM_CONSENSUS_DTYPE)
    for name, _ in TANDEM_DTYPE:
        out[name] = tandem[name]
    span = (tandem["end"] - tandem["start"]).astype(np.float64)
    out["consensus_identity"] = cons["agree"].astype(np.float64) / np.maximum(span, 1.0)
    out["primitive"] = [primitive_period(m) for m in motifs]
    return out


def join_period_chains(chains, links, with_paths=False):
    """The GAPPED tandem repeats of a window: the chains of period_chains (fetched at min_len = 0) joined along the links of
    period_links of the same window, range of k, min_seed and max_gap; join_chains' sibling.  Every chain has at most one link in
    and one out, so the links form paths; one row of PGROUP_DTYPE per path (a chain without links is a path of one), in the order
    of the paths' first chains: start: the first chain's; end: the last chain's start + len + k (the positions the repeat
    covers are [start, end)); k_first, k_min, k_max: the first chain's line, the smallest and the largest of the path; period:
    the k of the chain with the most matches (ties: the smaller k); chains, seeds; matches: the chains' matches minus the
    overlaps of the links inside the group; indel: the sum of |shift| -- an indel of d bases inside a repeat of period >=
    min_seed counts 2 d, out to the detour line and back, one of d bases at the repeat's end or between two different periods
    counts d; net_shift: the sum of the shifts (k_last - k_first); gap_cells: the sum of the links' gaps; span_a: the last
    chain's last cell - start + 1; span_b = span_a + k_last - k_first; open: a link into the group's first chain names a
    predecessor that is not in `chains` (it lies on a line outside the range of k or in front of the window).  with_paths: returns
    (rows, paths), the paths as period_paths gives them, for group_segments."""
    import numpy as np
    paths, link_out, is_open = _link_paths(chains, links)
    start, length, line = (chains[f].astype(np.int64) for f in ("start", "len", "k"))
    last_cell = start + length - 1
    out = np.zeros(len(paths), dtype=PGROUP_DTYPE)
    matches, seeds, ks = chains["matches"].tolist(), chains["seeds"].tolist(), line.tolist()
    shift, gap, overlap = (links[f].tolist() for f in ("shift", "gap", "overlap"))
    for at, path in enumerate(paths):
        g, head, cur = out[at], path[0], path[-1]
        total = n_seeds = indel = net = gap_cells = 0
        k_min = k_max = ks[head]
        best = (-1, 0)                                          # (matches, -k) of the chain that names the period
        for c in path:
            total, n_seeds = total + matches[c], n_seeds + seeds[c]
            k_min, k_max, best = min(k_min, ks[c]), max(k_max, ks[c]), max(best, (matches[c], -ks[c]))
            via = link_out[c]
            if via >= 0:
                total, indel, net, gap_cells = total - overlap[via], indel + abs(shift[via]), net + shift[via], gap_cells + gap[via]
        g["start"], g["end"], g["open"] = start[head], start[cur] + length[cur] + ks[cur], is_open[head]
        g["k_first"], g["k_min"], g["k_max"], g["period"] = ks[head], k_min, k_max, -best[1]
        g["span_a"] = last_cell[cur] - start[head] + 1
        g["span_b"] = int(g["span_a"]) + ks[cur] - ks[head]
        g["matches"], g["seeds"], g["chains"], g["indel"], g["net_shift"], g["gap_cells"] = total, n_seeds, len(path), indel, net, gap_cells
    return (out, paths) if with_paths else out


def tandem_groups(groups, drop_covered=True, with_index=False):
    """The repeats of a list of join_period_chains, one row of TANDEM_GROUP_DTYPE each, in the list's order: start, end, period,
    copies = (end - start) / period, identity = matches / max(span_a, span_b), indel, chains, seeds.  A repeat of period 3 is
    also periodic at 6, 9, ... and, with an indel, at neighbouring lines: drop_covered removes a group iff another group of the
    list with a strictly smaller period covers its [start, end).  with_index: returns (rows, the index of every row in
    `groups`), for group_consensus_rows, whose pieces name groups by that index.  Host numpy."""
    import numpy as np
    out = np.zeros(len(groups), dtype=TANDEM_GROUP_DTYPE)
    for f in ("start", "end", "period", "indel", "chains", "seeds"):
        out[f] = groups[f]
    out["copies"] = (groups["end"] - groups["start"]).astype(np.float64) / np.maximum(groups["period"], 1).astype(np.float64)
    out["identity"] = groups["matches"].astype(np.float64) / np.maximum(np.maximum(groups["span_a"], groups["span_b"]), 1).astype(np.float64)
    if not drop_covered or len(out) < 2:
        return (out, np.arange(len(out))) if with_index else out
    # by start, longest first, smallest period first: a group can only be covered by a group in front of it in this order (or by
    # one with the same interval, which has a smaller period and sorts in front).  Of the groups in front, per period, the
    # largest end is kept; a prefix minimum over the periods answers "does a smaller period reach behind my end".
    order = np.lexsort((out["period"], -out["end"].astype(np.int64), out["start"].astype(np.int64)))
    keep = np.ones(len(out), dtype=bool)
    reach = {}                                                  # period -> the largest end of the groups in front
    for at, p, b in zip(order.tolist(), out["period"][order].tolist(), out["end"][order].tolist()):
        if any(e >= b for q, e in reach.items() if q < p):
            keep[at] = False
        if reach.get(p, 0) < b:
            reach[p] = b
    return (out[keep], np.flatnonzero(keep)) if with_index else out[keep]


def tandem_rows(chains, drop_multiples=True):
    """The repeats of a list of period_chains, one row of TANDEM_DTYPE each, in the list's order: start, end = start + len + k (the
    positions the repeat covers), k, copies = (len + k) / k, identity = matches / len, matches, seeds.  A repeat of period 3 is
    also periodic at 6, 9, ...: drop_multiples removes a row (k, [a, b)) iff another row (k', [a', b')) of the list has k' < k,
    k % k' == 0, a' <= a and b' >= b.  Host numpy."""
    import numpy as np
    out = np.zeros(len(chains), dtype=TANDEM_DTYPE)
    k = chains["k"].astype(np.uint64)
    out["start"], out["k"], out["matches"], out["seeds"] = chains["start"], chains["k"], chains["matches"], chains["seeds"]
    out["end"] = chains["start"] + chains["len"] + k
    out["copies"] = (chains["len"] + k).astype(np.float64) / np.maximum(k, 1).astype(np.float64)
    out["identity"] = chains["matches"].astype(np.float64) / np.maximum(chains["len"], 1).astype(np.float64)
    if not drop_multiples or len(out) < 2:
        return out
    # by start, longest first: a row can only lie inside a row in front of it; the rows in front that can still hold a later one
    # are kept per period, as the largest end seen so far
    order = np.lexsort((out["k"], -out["end"].astype(np.int64), out["start"].astype(np.int64)))
    keep = np.ones(len(out), dtype=bool)
    reach, divisors = {}, {}                                    # period -> the largest end of the rows in front; -> its proper divisors
    for at, kk, b in zip(order.tolist(), out["k"][order].tolist(), out["end"][order].tolist()):
        if kk not in divisors:
            small = [q for q in range(1, int(kk ** 0.5) + 1) if kk % q == 0]
            divisors[kk] = sorted({q for d in small for q in (d, kk // d) if q < kk})
        if any(reach.get(q, 0) >= b for q in divisors[kk]):
            keep[at] = False
        if reach.get(kk, 0) < b:
            reach[kk] = b
    return out[keep]


def join_chains(chains, links, nb=None):
    """The gapped repeats of a window: the chains of dotpair_chains (fetched at min_len = 0) joined along the links of
    dotpair_links of the same window, min_seed and max_gap.  Every chain has at most one link in and one out, so the links form
    paths; one row of DOTGROUP_DTYPE per path (a chain without links is a path of one), in the order of the paths' first chains:
    row, col, dir of the first chain; end_row, end_col: the last chain's last cell; span_a, span_b: the rows and the columns from
    the first to the last cell; matches: the chains' matches minus the overlaps of the links inside the group (the cells of a
    successor's first seed that lie in front of its predecessor's end count once); chains, seeds; indel: the sum of |shift|;
    gap_cells: the sum of the links' gaps; open: a link into the group's first chain names a predecessor that is not in
    `chains`, so the group begins outside the window.  nb (the columns of the rectangle) is not needed: both lists hold columns."""
    import numpy as np
    n = len(chains)
    length = chains["len"].astype(np.int64)
    first = {key: k for k, key in enumerate(zip(chains["row"].tolist(), chains["col"].tolist(), chains["dir"].tolist()))}
    last_col = chains["col"].astype(np.int64) + np.where(chains["dir"] == 2, -(length - 1), length - 1)
    last_row = chains["row"].astype(np.int64) + length - 1
    last = {key: k for k, key in enumerate(zip(last_row.tolist(), last_col.tolist(), chains["dir"].tolist()))}
    nxt, link_of, has_in, is_open = [-1] * n, [-1] * n, [False] * n, [False] * n
    for k, (row, col, from_row, from_col, d) in enumerate(zip(*(links[f].tolist() for f in ("row", "col", "from_row", "from_col", "dir")))):
        y = first.get((row, col, d))
        if y is None:
            raise ValueError(f"the link into ({row}, {col}, dir {d}) names a successor that is not in the list of chains: "
                             "join_chains needs the chains of the same window, min_seed and max_gap, fetched at min_len = 0")
        x = last.get((from_row, from_col, d))
        if x is None:
            is_open[y] = True
        else:
            nxt[x], link_of[x], has_in[y] = y, k, True
    out = np.zeros(n - sum(has_in), dtype=DOTGROUP_DTYPE)
    matches, seeds = chains["matches"].tolist(), chains["seeds"].tolist()
    shift, gap, overlap = (links[f].tolist() for f in ("shift", "gap", "overlap"))
    at = 0
    for k in range(n):
        if has_in[k]:
            continue
        g = out[at]
        g["row"], g["col"], g["dir"], g["open"] = chains["row"][k], chains["col"][k], chains["dir"][k], is_open[k]
        total = n_seeds = n_chains = indel = gap_cells = 0
        while True:
            total, n_seeds, n_chains = total + matches[k], n_seeds + seeds[k], n_chains + 1
            if nxt[k] < 0:
                break
            via = link_of[k]
            total, indel, gap_cells = total - overlap[via], indel + abs(shift[via]), gap_cells + gap[via]
            k = nxt[k]
        g["end_row"], g["end_col"] = last_row[k], last_col[k]
        g["span_a"], g["span_b"] = last_row[k] - int(g["row"]) + 1, abs(int(last_col[k]) - int(g["col"])) + 1
        g["matches"], g["seeds"], g["chains"], g["indel"], g["gap_cells"] = total, n_seeds, n_chains, indel, gap_cells
        at += 1
    return out


def group_identity(groups):
    """matches / max(span_a, span_b) of every group of join_chains (float64)."""
    import numpy as np
    return groups["matches"].astype(np.float64) / np.maximum(np.maximum(groups["span_a"], groups["span_b"]), 1).astype(np.float64)


def chain_identity(chains):
    """matches / len of every chain of a list: the share of matching cells between the first seed's first and the last seed's
    last cell (float64; 1.0 for a single exact run)."""
    import numpy as np
    return chains["matches"].astype(np.float64) / np.maximum(chains["len"], 1).astype(np.float64)


def unique_chains(chains, strand="+"):
    """The chains of a range compared with ITSELF, each repeat once, by unique_runs' rule on (row, col, len): raw is symmetric
    there, so every chain has a mirror image across the main diagonal with the same len, matches and seeds.  Drops the trivial
    diagonal on the plus strand."""
    return unique_runs(chains, strand)


def run_cells(runs, na, nb):
    """bool[na, nb]: the cells of a list of runs (fields row, col, len, dir; dir 1: (row + s, col + s), 2: (row + s, col - s))."""
    import numpy as np
    out = np.zeros((na, nb), dtype=bool)
    length = runs["len"].astype(np.int64)
    which = np.repeat(np.arange(len(runs)), length)                            # the run of every cell
    s = np.arange(int(length.sum()), dtype=np.int64) - np.repeat(np.cumsum(length) - length, length)
    step = np.where(runs["dir"] == DOTRUN_MAIN, 1, -1).astype(np.int64)
    out[runs["row"].astype(np.int64)[which] + s, runs["col"].astype(np.int64)[which] + step[which] * s] = True
    return out


def unique_runs(runs, strand="+"):
    """The runs of a range compared with ITSELF, each repeat once: raw is symmetric there on both strands, so every run has a
    mirror image across the main diagonal.  Drops the trivial run (row == col, main, on the plus strand); of each mirror pair of
    main runs keeps the one with col > row; of each mirror pair of anti runs -- the mirror of (i, j, L) is (j - L + 1, i + L - 1,
    L) -- keeps the one with row <= col - len + 1, so that a run that is its own mirror stays."""
    import numpy as np
    row, col, length = (runs[f].astype(np.int64) for f in ("row", "col", "len"))
    main = runs["dir"] == DOTRUN_MAIN
    keep = np.where(main, col > row if strand == "+" else col >= row, row <= col - length + 1)
    return runs[keep]


class Genome:
    """Contigs packed and resident in HBM (prf_genome)."""

    def __init__(self, ctx, handle, n_contigs, lens=None):
        self.ctx = ctx
        self._h = handle
        self.n_contigs = n_contigs
        self.lens = None if lens is None else [int(n) for n in lens]   # contig lengths (period_counts / period_bits clip by them)

    def period_counts(self, contig, kmin, kmax, window, begin=0, end=None, with_stats=False):
        """The periodicity profile of positions [begin, end) of a contig (prf_period_counts): numpy uint32[kmax - kmin + 1,
        ceil(length / window)]; entry (k - kmin, w) = the positions i of window w with seq[i] == seq[i + k], i + k < end (N == N
        matches).  window: a multiple of 64.  end None or beyond the contig: its length.  with_stats: (array, ScanStats)."""
        return _matrix(self.ctx, (self, contig), begin, end, with_stats, period=(kmin, kmax, window))

    def period_bits(self, contig, kmin, kmax, begin=0, end=None, with_stats=False):
        """The periodicity matrix itself (prf_period_bits): numpy uint64[kmax - kmin + 1, ceil(length / 64)]; bit j of word w of
        row k - kmin = seq[i] == seq[i + k] for i = begin + 64 w + j, i + k < end."""
        return _matrix(self.ctx, (self, contig), begin, end, with_stats, period=(kmin, kmax, None))

    def dotplot_bits(self, contig, min_diagonal_run=3, begin=0, end=None, rows=None, cols=None, with_stats=False, launch_cells=0):
        """The exact dot plot of positions [begin, end) of a contig (prf_dotplot_bits): numpy uint64[rows, ceil(columns / 64)] for
        the window rows = (row0, row1) x cols = (col0, col1), relative to begin (None: all); bit j of word w of row r = kept(row0
        + r, col0 + 64 w + j): s[i] == s[j] (N == N matches) on a diagonal or anti-diagonal run of the whole matrix that the
        reference's filter_out_noise(min_diagonal_run) keeps.  unpack_bits() gives one byte per cell.  launch_cells: cells per
        launch (0: DOT_LAUNCH_CELLS)."""
        return _matrix(self.ctx, (self, contig), begin, end, with_stats, dot=(min_diagonal_run, None, rows, cols, launch_cells))

    def dotplot_counts(self, contig, block, min_diagonal_run=3, begin=0, end=None, rows=None, cols=None, with_stats=False,
                       launch_cells=0):
        """Kept cells per block of block x block cells of the window (prf_dotplot_counts): numpy uint32[ceil(rows / block),
        ceil(columns / block)].  block: a multiple of 64, 64 .. 32768."""
        return _matrix(self.ctx, (self, contig), begin, end, with_stats, dot=(min_diagonal_run, block, rows, cols, launch_cells))

    def dotpair_bits(self, a, b, strand="+", min_diagonal_run=3, rows=None, cols=None, with_stats=False, launch_cells=0):
        """The exact dot plot of two ranges of this genome (prf_dotpair_bits): a = (contig, begin, end) gives the rows, b the
        columns (end None: the contig's end).  numpy uint64[rows, ceil(columns / 64)] as dotplot_bits; bit = A[i] == B[j] on
        strand "+", A[i] == complement(B[j]) on strand "-" (columns in B's forward coordinates: an inverted repeat is an
        anti-diagonal), on a diagonal or anti-diagonal run of the whole na x nb rectangle that min_diagonal_run keeps."""
        return _matrix(self.ctx, (self, a[0]), a[1], a[2], with_stats, dot=(min_diagonal_run, None, rows, cols, launch_cells),
                       versus=((self, b[0]), b[1], b[2], strand))

    def dotpair_counts(self, a, b, block, strand="+", min_diagonal_run=3, rows=None, cols=None, with_stats=False, launch_cells=0):
        """Kept cells per block of block x block cells of the window of dotpair_bits (prf_dotpair_counts): numpy
        uint32[ceil(rows / block), ceil(columns / block)]."""
        return _matrix(self.ctx, (self, a[0]), a[1], a[2], with_stats, dot=(min_diagonal_run, block, rows, cols, launch_cells),
                       versus=((self, b[0]), b[1], b[2], strand))

    def dotpair_runs(self, a, b, strand="+", directions="both", min_len=DOTRUN_PROBE, rows=None, cols=None, with_stats=False,
                     launch_cells=0):
        """The maximal diagonal ("main": cells (row + s, col + s)) and anti-diagonal ("anti": (row + s, col - s)) runs of matching
        cells of the dot plot of dotpair_bits whose start cell (the one with the smallest row) lies in the window rows x cols and
        that have at least min_len cells (prf_dotpair_runs): a numpy structured array with the fields row, col, len, dir (1 main,
        2 anti), sorted by (row, col, dir).  len is never clipped by the window: the lists of a partition into windows add up to
        the whole list.  run_cells() rasterises a list; unique_runs() halves the list of a range against itself."""
        return _runs(self.ctx, (self, a[0]), a[1:], (self, b[0]), b[1:], strand, directions, min_len, rows, cols, with_stats, launch_cells)

    def dotpair_chains(self, a, b, strand="+", directions="both", min_seed=DOTRUN_PROBE, max_gap=0, min_len=0, rows=None, cols=None,
                       with_stats=False, launch_cells=0):
        """The diagonal repeats WITH MISMATCHES of the dot plot of dotpair_bits (prf_dotpair_chains): the runs of dotpair_runs at
        min_len = min_seed (the seeds), joined along their diagonal or anti-diagonal wherever at most max_gap cells lie between
        two of them.  A numpy structured array with the fields row, col (the first seed's start cell), len (up to the last seed's
        last cell), matches (matching cells among those), dir and seeds, sorted by (row, col, dir); the chains whose start cell
        lies in the window rows x cols and that have at least min_len cells.  Seeds and links are judged in the whole rectangle:
        the lists of a partition into windows add up.  chain_identity() gives matches / len; unique_chains() halves the list of
        a range against itself."""
        return _chains(self.ctx, (self, a[0]), a[1:], (self, b[0]), b[1:], strand, directions, min_seed, max_gap, min_len, rows, cols,
                       with_stats, launch_cells)

    def dotpair_links(self, a, b, strand="+", directions="both", min_seed=DOTRUN_PROBE, max_gap=0, max_shift=1, rows=None, cols=None,
                      with_stats=False, launch_cells=0):
        """The INDEL JUNCTIONS between the chains of dotpair_chains at the same min_seed and max_gap (prf_dotpair_links): chain
        X ends, chain Y starts 1 .. max_shift lines away, at most max_gap cells behind (or up to min(min_seed - 1, 16) cells in
        front), and each is the other's best such neighbour.  A numpy structured array with the fields row, col (Y's first cell:
        the key of Y's row in the list of chains), from_row, from_col (X's last cell), dir, shift (positive: bases only B has),
        gap and overlap, sorted by (row, col, dir); the links whose (row, col) lies in the window rows x cols.  Links are judged
        in the whole rectangle: the lists of a partition into windows add up.  join_chains() folds the two lists into gapped
        repeats."""
        return _links(self.ctx, (self, a[0]), a[1:], (self, b[0]), b[1:], strand, directions, min_seed, max_gap, max_shift, rows, cols,
                      with_stats, launch_cells)

    def period_chains(self, contig, begin, end, kmin, kmax, min_seed, max_gap, min_len=0, n_matches=False, positions=None,
                      with_stats=False, launch_cells=0):
        """The DIVERGED TANDEM REPEATS of positions [begin, end) of a contig (prf_period_chains): on every period line k = kmin ..
        kmax of the range (cell t: seq[t] == seq[t + k], t + k < end) the exact runs of at least min_seed cells, joined wherever
        at most max_gap cells lie between two of them.  A numpy structured array with the fields start (relative to begin), len,
        matches, k and seeds, sorted by (start, k): the chains that start in positions = (pos0, pos1) (None: all) and have at least
        min_len cells; the repeat covers [start, start + len + k).  n_matches: N == N is a match, as in period_bits; False: N
        never matches, as in the scans.  Chains are judged on the whole line: the lists of a partition in positions or in k add
        up.  end None: the contig's end.  tandem_rows() turns the list into repeats."""
        return _period_chains(self.ctx, (self, contig), begin, end, kmin, kmax, min_seed, max_gap, min_len, n_matches, positions,
                              with_stats, launch_cells)

    def period_links(self, contig, begin, end, kmin, kmax, min_seed, max_gap, max_shift, n_matches=False, positions=None,
                     with_stats=False, launch_cells=0):
        """The INDEL JUNCTIONS between the chains of period_chains at the same min_seed and max_gap (prf_period_links): chain X
        ends on line k - shift, chain Y starts on line k, 1 .. max_shift lines away, at most max_gap cells behind (or up to
        min(min_seed - 1, 16) cells in front), and each is the other's best such neighbour.  A numpy structured array with the
        fields start, k (the key of Y's row in the list of chains), from_end (X's last cell), shift, gap and overlap, sorted by
        (start, k): the links whose Y starts in positions = (pos0, pos1) (None: all) on a line kmin .. kmax.  Links are judged
        against every line 1 .. n - 1 of the range: the lists of a partition in positions or in k add up, and X may lie on a line
        outside kmin .. kmax.  join_period_chains() folds the two lists into gapped tandem repeats."""
        return _period_links(self.ctx, (self, contig), begin, end, kmin, kmax, min_seed, max_gap, max_shift, n_matches, positions,
                             with_stats, launch_cells)

    def period_consensus(self, contig, begin, end, repeats, counts=False, with_stats=False, slice_positions=0):
        """The CONSENSUS MOTIFS of repeats of positions [begin, end) of a contig (prf_period_consensus).  repeats: any structured
        array with the fields start, end (relative to begin) and k, such as the rows of tandem_rows().  Column p of a repeat holds
        the positions start + p + j k; its letter is the most frequent of A, C, G, T there (ties to the first in that order, 'N'
        for a column without any).  Returns (rows, motifs) in the order of the repeats: a numpy structured array with the fields
        offset, agree (positions that carry their column's letter), acgt (positions that are A, C, G or T) and k, and the motifs
        as a list of str; with counts=True also the counts, an array of (sum of k, 4) at the rows' offsets.  end None: the
        contig's end.  slice_positions: positions per work item (0: the default), for the tests.  consensus_rows() joins the
        result to the repeats."""
        return _period_consensus(self.ctx, (self, contig), begin, end, repeats, counts, with_stats, slice_positions)

    def phased_consensus(self, contig, begin, end, ks, segments, counts=False, with_stats=False, slice_positions=0):
        """The CONSENSUS MOTIFS of rows whose positions come as SEGMENTS WITH A PHASE, of positions [begin, end) of a contig
        (prf_phased_consensus): the consensus of a gapped repeat.  ks: one k per row.  segments: any structured array with the
        fields start, end (relative to begin), row and phase, such as group_segments() returns; position q of a segment lies in
        column (phase + q - start) mod k of its row.  Segments may come in any order, overlap and interleave; a row without
        segments is all 'N'.  Returns what period_consensus returns, one row per k.  group_consensus_rows() joins the result to
        the groups."""
        return _phased_consensus(self.ctx, (self, contig), begin, end, ks, segments, counts, with_stats, slice_positions)

    def motif_align(self, contig, begin, end, repeats, motifs, with_stats=False):
        """The ALIGNMENT of repeats of positions [begin, end) of a contig to their motifs (prf_motif_align): each repeat's
        positions against the endless repetition of its motif, free at both ends of the motif, unit costs.  repeats: any
        structured array with the fields start, end (relative to begin) and k <= ALIGN_MAX_K, of at most ALIGN_MAX_LEN positions
        each.  motifs: a list of str over A C G T N, one of k letters per repeat, or the letters a consensus call returned, in
        one str or bytes.  Returns a numpy structured array in the order of the repeats with the fields edits (substitutions +
        insertions + deletions, the least possible), indels (the least among those), consumed (motif letters the alignment runs
        over, the least among those), start_column and end_column.  alignment_rows() derives the rest."""
        return _motif_align(self.ctx, (self, contig), begin, end, repeats, motifs, with_stats)

    def motif_align_path(self, contig, begin, end, repeats, motifs, with_counts=False, with_stats=False, trace_bytes=0):
        """motif_align WITH ITS PATH (prf_motif_align_path): the same rows, and per repeat one uint16 per position: the motif
        column in PATH_COLUMN; PATH_INS: the position is an insertion behind that column; PATH_SUB: it is aligned to the column
        and does not match it.  Deleted motif letters are read from the path (path_deletions, path_cigar).  Returns (rows, list
        of paths), then with_counts an array of (sum of k, 6) per motif letter: the aligned positions that are A, C, G, T, the
        deletions and the insertions of the column (aligned_consensus re-estimates the motifs from it), then the ScanStats
        with_stats.  trace_bytes bounds the device scratch of one batch of repeats (0: the library's default); the results do
        not depend on it."""
        return _motif_align_path(self.ctx, (self, contig), begin, end, repeats, motifs, with_counts, with_stats, trace_bytes)

    def motif_align_local(self, contig, begin, end, repeats, motifs, match=2, mismatch=7, indel=7, with_stats=False):
        """The best LOCAL alignment of windows of positions [begin, end) of a contig against the endless repetition of their
        motifs (prf_motif_align_local), scored match * matches - mismatch * substitutions - indel * (insertions + deletions),
        each weight 1 .. ALIGNLOCAL_MAX_WEIGHT.  repeats: the windows, as motif_align takes its repeats (flank_repeats pads found
        repeats).  Returns a numpy structured array in the order of the windows with the fields score, first and end (relative
        to the window's start), start_column and end_column; of equal scores the alignment that ends first and begins last; all
        zeros where nothing matches.  motif_align on (start + first, start + end, k) with the same motif gives the refined
        interval's edits and copies; local_rows() puts the intervals beside their rows."""
        return _motif_align_local(self.ctx, (self, contig), begin, end, repeats, motifs, match, mismatch, indel, with_stats)

    @property
    def positions(self):
        return self.ctx.lib.prf_genome_positions(self._h)

    def scan(self, kmin, kmax, min_repeats, min_span, flags=SCAN_DEFAULT, fetch=True):
        """Returns (rows, stats): rows is a numpy record array (start, end, k, contig) sorted by
        (contig, start, end), or None when fetch=False."""
        lib = self.ctx.lib
        hits = _Hits()
        stats = ScanStats()
        f = flags | (0 if fetch else SCAN_NO_FETCH)
        _check(lib, lib.prf_scan_genome(self.ctx._h, self._h, kmin, kmax, min_repeats, min_span, f,
                                        ctypes.byref(hits), ctypes.byref(stats)))
        if not fetch:
            return None, stats
        try:
            return _rows(hits), stats
        finally:
            lib.prf_free_hits(ctypes.byref(hits))

    def select(self, parts):
        """Restrict the following scans of this genome to `parts`: (contig, begin, end) position ranges cut at multiples
        of tile_positions() (multi_gpu.plan_parts makes them).  None / []: the whole genome again."""
        parts = list(parts or [])
        arr = (_Part * max(1, len(parts)))()
        for i, (c, b, e) in enumerate(parts):
            arr[i].contig, arr[i].begin, arr[i].end = c, b, e
        _check(self.ctx.lib, self.ctx.lib.prf_genome_select(self._h, arr, len(parts)))

    def tile_classes(self, contig):
        """numpy uint8 array, one cost class per tile of the contig (0 ordinary, 1 not-ACGT in reach, 2 never scanned)."""
        import numpy as np
        n = ctypes.c_uint64(0)
        _check(self.ctx.lib, self.ctx.lib.prf_genome_tile_classes(self._h, contig, None, 0, ctypes.byref(n)))
        out = np.zeros(max(1, n.value), dtype=np.uint8)
        _check(self.ctx.lib, self.ctx.lib.prf_genome_tile_classes(self._h, contig, out.ctypes.data_as(ctypes.c_void_p), n.value,
                                                                  ctypes.byref(n)))
        return out[:n.value]

    def contig_bases(self):
        """First position of every contig in the genome's coordinate space (numpy uint64)."""
        import numpy as np
        n = ctypes.c_uint64(0)
        _check(self.ctx.lib, self.ctx.lib.prf_genome_contig_bases(self._h, None, 0, ctypes.byref(n)))
        out = (ctypes.c_uint64 * max(1, n.value))()
        _check(self.ctx.lib, self.ctx.lib.prf_genome_contig_bases(self._h, out, n.value, ctypes.byref(n)))
        return np.array(out[:n.value], dtype=np.uint64)

    def footprint(self):
        """(device bytes the resident genome holds, positions of its coordinate space): prf_genome_footprint."""
        b, n = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(self.ctx.lib, self.ctx.lib.prf_genome_footprint(self._h, ctypes.byref(b), ctypes.byref(n)))
        return b.value, n.value

    def scan_async(self, kmin, kmax, min_repeats, min_span):
        """Enqueue a scan (at most two in flight); returns its serial number for Context.scan_wait()."""
        seq = ctypes.c_uint64(0)
        _check(self.ctx.lib, self.ctx.lib.prf_scan_genome_async(self.ctx._h, self._h, kmin, kmax, min_repeats, min_span,
                                                                 ctypes.byref(seq)))
        return seq.value

    def scan_async_packed(self, kmin, kmax, min_repeats, min_span, dst_ptr, capacity_rows, side_capacity):
        """scan_async() whose rows also leave as 8-byte wire words in caller-owned device memory (capacity_rows + 1 +
        3 * side_capacity words), packed on the library's stream behind the scan: no host step in between."""
        seq = ctypes.c_uint64(0)
        _check(self.ctx.lib, self.ctx.lib.prf_scan_genome_async_packed(self.ctx._h, self._h, kmin, kmax, min_repeats, min_span,
                                                                        ctypes.c_void_p(dst_ptr), capacity_rows, side_capacity,
                                                                        ctypes.byref(seq)))
        return seq.value

    def free(self):
        if self._h is not None:
            self.ctx.lib.prf_genome_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One GPU, one HIP stream (prf_ctx)."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = ctypes.c_void_p()
        _check(self.lib, self.lib.prf_open(device, ctypes.byref(h)))
        self._h = h
        self.device = device

    def load(self, seqs, kmax_hint):
        arr, _keep = _contig_array(seqs)
        g = ctypes.c_void_p()
        _check(self.lib, self.lib.prf_genome_load(self._h, arr, len(seqs), kmax_hint, ctypes.byref(g)))
        return Genome(self, g, len(seqs), [s[1] if isinstance(s, tuple) else len(s) for s in seqs])

    def synth(self, lens, seeds, kmax_hint):
        """Contigs generated on the device (SURVEY 8(d) generator): nothing crosses PCIe."""
        n = len(lens)
        la = (ctypes.c_uint64 * max(1, n))(*lens)
        sa = (ctypes.c_uint64 * max(1, n))(*seeds)
        g = ctypes.c_void_p()
        _check(self.lib, self.lib.prf_genome_synth(self._h, la, sa, n, kmax_hint, ctypes.byref(g)))
        return Genome(self, g, n, lens)

    def standin(self, lens, seeds, kmax_hint):
        """Contigs of the stand-in recipe 2 (synth.standin2) generated on the device."""
        n = len(lens)
        la = (ctypes.c_uint64 * max(1, n))(*lens)
        sa = (ctypes.c_uint64 * max(1, n))(*seeds)
        g = ctypes.c_void_p()
        _check(self.lib, self.lib.prf_genome_standin(self._h, la, sa, n, kmax_hint, ctypes.byref(g)))
        return Genome(self, g, n, lens)

    def scan(self, seqs, kmin, kmax, min_repeats, min_span, flags=SCAN_DEFAULT):
        arr, _keep = _contig_array(seqs)
        hits = _Hits()
        stats = ScanStats()
        _check(self.lib, self.lib.prf_scan(self._h, arr, len(seqs), kmin, kmax, min_repeats, min_span, flags,
                                           ctypes.byref(hits), ctypes.byref(stats)))
        try:
            return _rows(hits), stats
        finally:
            self.lib.prf_free_hits(ctypes.byref(hits))

    def scan_interrupted(self, seqs, kmin, kmax, min_repeats, min_span, max_interruptions, memo_stride=None, memo_slots=None,
                         counters=False, chunk=None, max_interruptions_by_k=None):
        """Interrupted repeats of many whole sequences in one call (prf_scan_interrupted): (rows, stats[, counters]).  rows: numpy
        records (start, end, k, contig, nmask) sorted by (contig, start, end); bit i of nmask = phase i of the motif may vary.
        memo_stride / memo_slots: the walk's memo table (the rows do not depend on it); counters: also return a dict of the
        walk's steps, memo lookups, memo hits and recorded episodes.  chunk: None = one lane per (sequence, motif size)
        (prf_scan_interrupted_ex); an integer = prf_scan_interrupted_chunked with that many landing positions per lane (0: one
        lane again; INT_CHUNK: the library's default), and the counters then also hold `lanes` and `dropped_lanes`.  The rows
        do not depend on it.  max_interruptions_by_k: a budget per motif size (prf_scan_interrupted_by_k), see
        interruption_budgets(); every value >= 0 is served, all zeros included."""
        import numpy as np
        arr, _keep = _contig_array(list(seqs))
        hits, stats = _IHits(), ScanStats()
        ctr = (ctypes.c_uint64 * 6)()
        stride = MEMO_STRIDE if memo_stride is None else memo_stride
        slots = MEMO_SLOTS if memo_slots is None else memo_slots
        if max_interruptions_by_k is not None:
            by_k = interruption_budgets(kmin, kmax, max_interruptions, max_interruptions_by_k)
            _check(self.lib, self.lib.prf_scan_interrupted_by_k(
                self._h, arr, len(seqs), kmin, kmax, min_repeats, min_span, (ctypes.c_uint32 * len(by_k))(*by_k), stride, slots,
                chunk or 0, ctypes.byref(hits), ctypes.byref(stats), ctr))
        elif chunk is None:
            _check(self.lib, self.lib.prf_scan_interrupted_ex(
                self._h, arr, len(seqs), kmin, kmax, min_repeats, min_span, max_interruptions, stride, slots,
                ctypes.byref(hits), ctypes.byref(stats), ctr))
        else:
            _check(self.lib, self.lib.prf_scan_interrupted_chunked(
                self._h, arr, len(seqs), kmin, kmax, min_repeats, min_span, max_interruptions, stride, slots, chunk,
                ctypes.byref(hits), ctypes.byref(stats), ctr))
        try:
            n = hits.n
            if n == 0:
                rows = np.zeros(0, dtype=IHIT_DTYPE)
            else:
                buf = np.ctypeslib.as_array(ctypes.cast(hits.rows, ctypes.POINTER(ctypes.c_uint8)), shape=(n * ctypes.sizeof(_IHit),))
                rows = buf.view(np.dtype(IHIT_DTYPE)).copy()
        finally:
            self.lib.prf_free_ihits(ctypes.byref(hits))
        if counters:
            out = {"steps": ctr[0], "lookups": ctr[1], "hits": ctr[2], "episodes": ctr[3]}
            if chunk is not None:
                out.update(lanes=ctr[4], dropped_lanes=ctr[5])
            return rows, stats, out
        return rows, stats

    def dotplot_bits(self, seq, min_diagonal_run=3, begin=0, end=None, rows=None, cols=None, with_stats=False):
        """Genome.dotplot_bits for one sequence (str or bytes) in one call: load, compute, free (prf_dotplot_bits_seq)."""
        return _matrix(self, seq, begin, end, with_stats, dot=(min_diagonal_run, None, rows, cols, 0))

    def dotplot_counts(self, seq, block, min_diagonal_run=3, begin=0, end=None, rows=None, cols=None, with_stats=False):
        """Genome.dotplot_counts for one sequence (str or bytes) in one call (prf_dotplot_counts_seq)."""
        return _matrix(self, seq, begin, end, with_stats, dot=(min_diagonal_run, block, rows, cols, 0))

    def dotpair_bits(self, seq_a, seq_b, strand="+", min_diagonal_run=3, a=(0, None), b=(0, None), rows=None, cols=None,
                     with_stats=False):
        """Genome.dotpair_bits for two sequences (str or bytes; rows from seq_a, columns from seq_b) in one call: load, compute,
        free (prf_dotpair_bits_seq).  a, b: (begin, end) of the range of each sequence."""
        return _matrix(self, seq_a, a[0], a[1], with_stats, dot=(min_diagonal_run, None, rows, cols, 0),
                       versus=(seq_b, b[0], b[1], strand))

    def dotpair_counts(self, seq_a, seq_b, block, strand="+", min_diagonal_run=3, a=(0, None), b=(0, None), rows=None, cols=None,
                       with_stats=False):
        """Genome.dotpair_counts for two sequences in one call (prf_dotpair_counts_seq)."""
        return _matrix(self, seq_a, a[0], a[1], with_stats, dot=(min_diagonal_run, block, rows, cols, 0),
                       versus=(seq_b, b[0], b[1], strand))

    def dotpair_runs(self, seq_a, seq_b, strand="+", directions="both", min_len=DOTRUN_PROBE, a=(0, None), b=(0, None), rows=None,
                     cols=None, with_stats=False):
        """Genome.dotpair_runs for two sequences (str or bytes) in one call: load, list, free (prf_dotpair_runs_seq)."""
        return _runs(self, seq_a, a, seq_b, b, strand, directions, min_len, rows, cols, with_stats, 0)

    def dotpair_chains(self, seq_a, seq_b, strand="+", directions="both", min_seed=DOTRUN_PROBE, max_gap=0, min_len=0, a=(0, None),
                       b=(0, None), rows=None, cols=None, with_stats=False):
        """Genome.dotpair_chains for two sequences (str or bytes) in one call: load, list, free (prf_dotpair_chains_seq)."""
        return _chains(self, seq_a, a, seq_b, b, strand, directions, min_seed, max_gap, min_len, rows, cols, with_stats, 0)

    def dotpair_links(self, seq_a, seq_b, strand="+", directions="both", min_seed=DOTRUN_PROBE, max_gap=0, max_shift=1, a=(0, None),
                      b=(0, None), rows=None, cols=None, with_stats=False):
        """Genome.dotpair_links for two sequences (str or bytes) in one call: load, list, free (prf_dotpair_links_seq)."""
        return _links(self, seq_a, a, seq_b, b, strand, directions, min_seed, max_gap, max_shift, rows, cols, with_stats, 0)

    def period_chains(self, seq, kmin, kmax, min_seed, max_gap, min_len=0, n_matches=False, begin=0, end=None, positions=None,
                      with_stats=False):
        """Genome.period_chains for one sequence (str or bytes) in one call: load, list, free (prf_period_chains_seq)."""
        return _period_chains(self, seq, begin, end, kmin, kmax, min_seed, max_gap, min_len, n_matches, positions, with_stats, 0)

    def period_consensus(self, seq, repeats, begin=0, end=None, counts=False, with_stats=False):
        """Genome.period_consensus for one sequence (str or bytes) in one call: load, count, free (prf_period_consensus_seq)."""
        return _period_consensus(self, seq, begin, end, repeats, counts, with_stats, 0)

    def phased_consensus(self, seq, ks, segments, begin=0, end=None, counts=False, with_stats=False):
        """Genome.phased_consensus for one sequence (str or bytes) in one call: load, count, free (prf_phased_consensus_seq)."""
        return _phased_consensus(self, seq, begin, end, ks, segments, counts, with_stats, 0)

    def motif_align(self, seq, repeats, motifs, begin=0, end=None, with_stats=False):
        """Genome.motif_align for one sequence (str or bytes) in one call: load, align, free (prf_motif_align_seq)."""
        return _motif_align(self, seq, begin, end, repeats, motifs, with_stats)

    def motif_align_path(self, seq, repeats, motifs, begin=0, end=None, with_counts=False, with_stats=False):
        """Genome.motif_align_path for one sequence (str or bytes) in one call: load, align, free (prf_motif_align_path_seq)."""
        return _motif_align_path(self, seq, begin, end, repeats, motifs, with_counts, with_stats, 0)

    def motif_align_local(self, seq, repeats, motifs, begin=0, end=None, match=2, mismatch=7, indel=7, with_stats=False):
        """Genome.motif_align_local for one sequence (str or bytes) in one call: load, align, free (prf_motif_align_local_seq)."""
        return _motif_align_local(self, seq, begin, end, repeats, motifs, match, mismatch, indel, with_stats)

    def period_links(self, seq, kmin, kmax, min_seed, max_gap, max_shift, n_matches=False, begin=0, end=None, positions=None,
                     with_stats=False):
        """Genome.period_links for one sequence (str or bytes) in one call: load, list, free (prf_period_links_seq)."""
        return _period_links(self, seq, begin, end, kmin, kmax, min_seed, max_gap, max_shift, n_matches, positions, with_stats, 0)

    def period_counts(self, seq, kmin, kmax, window, begin=0, end=None, with_stats=False):
        """Genome.period_counts for one sequence (str or bytes) in one call: load, count, free (prf_period_counts_seq)."""
        return _matrix(self, seq, begin, end, with_stats, period=(kmin, kmax, window))

    def period_bits(self, seq, kmin, kmax, begin=0, end=None, with_stats=False):
        """Genome.period_bits for one sequence (str or bytes) in one call (prf_period_bits_seq)."""
        return _matrix(self, seq, begin, end, with_stats, period=(kmin, kmax, None))

    def scan_literal(self, seq, kmin, kmax, min_repeats, min_span, stop=None):
        """The literal lane on one sequence (prf_scan_literal); stop: lock-step iterations performed, default all."""
        arr, _keep = _contig_array([seq])
        hits = _Hits()
        stats = ScanStats()
        _check(self.lib, self.lib.prf_scan_literal(self._h, arr, kmin, kmax, min_repeats, min_span,
                                                   arr[0].len if stop is None else stop, ctypes.byref(hits), ctypes.byref(stats)))
        try:
            return _rows(hits), stats
        finally:
            self.lib.prf_free_hits(ctypes.byref(hits))

    def last_hits_to_device(self, dst_ptr, capacity_rows, count_row=False):
        """D2D copy of the last scan's rows into caller-owned device memory; returns the row count.
        count_row: record number capacity_rows of the buffer receives (rows copied, 0, 0)."""
        n = ctypes.c_uint64(0)
        _check(self.lib, self.lib.prf_last_hits_to_device(self._h, ctypes.c_void_p(dst_ptr), capacity_rows,
                                                          1 if count_row else 0, ctypes.byref(n)))
        return n.value

    def last_hits_packed_to_device(self, genome, dst_ptr, capacity_rows, side_capacity):
        """The last scan's rows as 8-byte wire words (+ count word + side list of long rows) in caller-owned device memory of
        capacity_rows + 1 + 3 * side_capacity words; returns the row count.  multi_gpu.unpack_rows() decodes."""
        n = ctypes.c_uint64(0)
        _check(self.lib, self.lib.prf_last_hits_packed_to_device(self._h, genome._h, ctypes.c_void_p(dst_ptr), capacity_rows,
                                                                 side_capacity, ctypes.byref(n)))
        return n.value

    def stream_wait_for(self, other_stream):
        """What has been enqueued on the library's stream happens before what `other_stream` (a raw hipStream_t, e.g.
        torch.cuda.Stream().cuda_stream) runs from now on."""
        _check(self.lib, self.lib.prf_stream_wait_for(self._h, ctypes.c_void_p(other_stream)))

    def scan_wait(self, seq):
        """Collect a scan enqueued with Genome.scan_async(); returns its ScanStats (row and candidate counts)."""
        stats = ScanStats()
        _check(self.lib, self.lib.prf_scan_wait(self._h, seq, ctypes.byref(stats)))
        return stats

    def set_row_sink(self, dst_ptr, capacity_rows):
        """Following scans compact their rows into caller-owned device memory (capacity_rows + 1 records, the last
        one receives the row count); dst_ptr None/0 switches back to the library's own array."""
        _check(self.lib, self.lib.prf_set_row_sink(self._h, ctypes.c_void_p(dst_ptr or None), capacity_rows))

    def scan_timings(self, first_seq, n):
        """HIP-event kernel times (ms) of n fused scans from serial number first_seq (ScanStats.seq) on."""
        out = (ctypes.c_float * max(1, n))()
        _check(self.lib, self.lib.prf_scan_timings(self._h, first_seq, n, out))
        return [float(out[i]) for i in range(n)]

    def scan_timings_split(self, first_seq, n):
        """(scan kernel ms, gather kernel ms) lists of n fused scans from serial number first_seq on."""
        a = (ctypes.c_float * max(1, n))()
        b = (ctypes.c_float * max(1, n))()
        _check(self.lib, self.lib.prf_scan_timings_split(self._h, first_seq, n, a, b))
        return [float(a[i]) for i in range(n)], [float(b[i]) for i in range(n)]

    def measure_hbm_read(self, nbytes=1 << 30, iters=5):
        out = ctypes.c_double(0)
        _check(self.lib, self.lib.prf_measure_hbm_read(self._h, nbytes, iters, ctypes.byref(out)))
        return out.value

    def close(self):
        if self._h is not None:
            self.lib.prf_close(self._h)
            self._h = None


class Fasta:
    """FASTA file read by libprf (plain or gzip): entries in file order; the sequence bytes stay in native memory."""

    class Entry:
        def __init__(self, name, addr, length):
            self.name, self.addr, self.length = name, addr, length

        def __len__(self):
            return self.length

        @property
        def seq(self):
            return ctypes.string_at(self.addr, self.length).decode("ascii", "replace") if self.length else ""

    def __init__(self, path, only=None):
        """only: read just that record (by seeking, if `path`.fai exists and the file is not compressed)."""
        self.lib = load_library()
        h = ctypes.c_void_p()
        if only is None:
            _check(self.lib, self.lib.prf_fasta_open(os.fsencode(path), ctypes.byref(h)))
        else:
            _check(self.lib, self.lib.prf_fasta_open_contig(os.fsencode(path), only.encode(), ctypes.byref(h)))
        self._h = h
        self.entries = []
        for i in range(self.lib.prf_fasta_count(h)):
            name, seq, n = ctypes.c_char_p(), ctypes.c_void_p(), ctypes.c_uint64()
            _check(self.lib, self.lib.prf_fasta_entry(h, i, ctypes.byref(name), ctypes.byref(seq), ctypes.byref(n)))
            self.entries.append(Fasta.Entry(name.value.decode(), seq.value or 0, n.value))
        self._by_name = {}
        for e in self.entries:
            self._by_name.setdefault(e.name, e)

    def __iter__(self):
        return iter(self.entries)

    def __len__(self):
        return len(self.entries)

    def __contains__(self, name):
        return name in self._by_name

    def __getitem__(self, key):
        return self.entries[key] if isinstance(key, int) else self._by_name[key]

    def close(self):
        if self._h is not None:
            self.lib.prf_fasta_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fasta_index(path):
    """([(name, length), ...] in file order, whole).  Read from the samtools-style index `path`.fai if it lies next to an
    uncompressed file (then `whole` is None and single records are read by seeking, Fasta(path, only=name)); otherwise the
    file is parsed once and `whole` is the Fasta object that holds every record."""
    fai = os.fspath(path) + ".fai"
    if os.path.exists(fai) and not os.fspath(path).endswith(".gz"):
        index = []
        with open(fai) as f:
            for line in f:
                cols = line.rstrip("\n").split("\t")
                if len(cols) >= 5:
                    index.append((cols[0], int(cols[1])))
        if index:
            return index, None
    whole = Fasta(path)
    return [(e.name, len(e)) for e in whole], whole


def scan_fasta_to_bed(ctx, fasta, bed_path, kmin, kmax, min_repeats, min_span, on_contig=None):
    """All contigs of a FASTA in ONE resident genome and one scan; BED written by libprf.  Returns rows per contig.
    on_contig(entry, n_rows) is called per contig in file order (the CLI prints the reference's lines there)."""
    lib = ctx.lib
    entries = list(fasta)
    arr, _keep = _contig_array([(e.addr, e.length) for e in entries])
    hits, stats = _Hits(), ScanStats()
    _check(lib, lib.prf_scan(ctx._h, arr, len(entries), kmin, kmax, min_repeats, min_span, SCAN_DEFAULT, ctypes.byref(hits),
                             ctypes.byref(stats)))
    try:
        names = (ctypes.c_char_p * max(1, len(entries)))(*[e.name.encode() for e in entries])
        written = ctypes.c_uint64(0)
        _check(lib, lib.prf_write_bed(os.fsencode(bed_path), 0, names, arr, len(entries), ctypes.byref(hits), ctypes.byref(written)))
        import numpy as np
        counts = np.bincount(_rows(hits)["contig"], minlength=len(entries)) if hits.n else np.zeros(len(entries), dtype=np.int64)
    finally:
        lib.prf_free_hits(ctypes.byref(hits))
    if on_contig:
        for e, c in zip(entries, counts):
            on_contig(e, int(c))
    return [int(c) for c in counts], stats


def write_bed(bed_path, entries, rows):
    """BED through libprf's writer (host code) from a numpy row array (start, end, k, contig: 24-byte records, contig =
    index into entries, sorted as the file should be); returns rows per contig."""
    import numpy as np
    lib = load_library()
    rows = np.ascontiguousarray(rows)
    assert rows.dtype.itemsize == ctypes.sizeof(_Hit)
    arr, _keep = _contig_array([(e.addr, e.length) for e in entries])
    hits = _Hits()
    hits.rows = ctypes.cast(rows.ctypes.data, ctypes.POINTER(_Hit))
    hits.n = len(rows)
    names = (ctypes.c_char_p * max(1, len(entries)))(*[e.name.encode() for e in entries])
    written = ctypes.c_uint64(0)
    _check(lib, lib.prf_write_bed(os.fsencode(bed_path), 0, names, arr, len(entries), ctypes.byref(hits), ctypes.byref(written)))
    counts = np.bincount(rows["contig"], minlength=len(entries)) if len(rows) else np.zeros(len(entries), dtype=np.int64)
    return [int(c) for c in counts]


def tile_positions():
    return int(load_library().prf_tile_positions())


def plan_describe(kmin, kmax, min_repeats, min_span):
    """Host-only: the fused kernel's work plan for these parameters, as a dict (no GPU needed)."""
    import json
    lib = load_library()
    buf = ctypes.create_string_buffer(1 << 16)
    rc = lib.prf_plan_describe(kmin, kmax, min_repeats, min_span, buf, len(buf))
    if rc < 0:
        raise PrfError(rc, lib.prf_last_error().decode("utf-8", "replace"))
    return json.loads(buf.value.decode())


_default_ctx = {}


def default_context(device=None):
    """Process-wide context for detect_repeats(); device from PRF_DEVICE / LOCAL_RANK / 0."""
    if device is None:
        device = int(os.environ.get("PRF_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]
