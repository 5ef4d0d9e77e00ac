"""ctypes binding of the C-ABI library seeq_amd/lib/libseeq_amd.so.

The declarations mirror include/libseeq.h, include/seeq.h and
include/seeq_amd.h one to one.  There is no fallback: if the library is not
built, or it finds no GPU, the calls raise.
"""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libseeq_amd.so")
CLI_PATH = os.path.join(HERE, "bin", "seeq")
CSRC = os.path.join(HERE, "csrc")

# libseeq.h option bits
SQ_FIRST, SQ_BEST, SQ_ALL, SQ_COUNT = 0x00, 0x01, 0x02, 0x03
SQ_FAIL, SQ_CONVERT, SQ_IGNORE = 0x00, 0x04, 0x08
SQ_LINES, SQ_STREAM = 0x00, 0x10
# seeq.h file options
SQ_ANY, SQ_MATCH, SQ_NOMATCH, SQ_COUNTLINES, SQ_COUNTMATCH = 0, 1, 2, 3, 4
# seeq_amd.h
WANT_COUNTLINES, WANT_COUNTMATCH, WANT_RECORDS = 0, 1, 2
SEEQDEV_FASTA, SEEQDEV_SINGLELINE, SEEQDEV_FASTQ = 0x100, 0x200, 0x400
SEEQDEV_HIT_MINUS = 0x80000000      # bit 31 of a both-strands record's dist: the minus strand


class match_t(C.Structure):
    _fields_ = [("start", C.c_size_t), ("end", C.c_size_t), ("dist", C.c_size_t)]


class seeq_t(C.Structure):
    _fields_ = [("hits", C.c_size_t), ("stacksize", C.c_size_t), ("match", C.POINTER(match_t)),
                ("bufsz", C.c_size_t), ("string", C.c_void_p), ("tau", C.c_int), ("wlen", C.c_int),
                ("keys", C.POINTER(C.c_char)), ("rkeys", C.POINTER(C.c_char)),
                ("dfa", C.c_void_p), ("rdfa", C.c_void_p)]


class seeqdev_packed_t(C.Structure):
    _fields_ = [("bases", C.c_void_p), ("nmask", C.c_void_p), ("nreads", C.c_uint64), ("read_len", C.c_uint32),
                ("stride", C.c_uint32), ("nstride", C.c_uint32)]


class seeqfile_t(C.Structure):
    _fields_ = [("flags", C.c_int), ("line", C.c_size_t), ("info", C.c_char_p), ("fdi", C.c_void_p)]


class seeqdev_hit_t(C.Structure):
    _fields_ = [("line", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32), ("dist", C.c_uint32)]


class seeqdev_counts_t(C.Structure):
    _fields_ = [("nlines", C.c_uint64), ("nmatchlines", C.c_uint64), ("nhits", C.c_uint64),
                ("nrecords", C.c_uint64), ("nheaders", C.c_uint64)]


class seeqdev_textinfo_t(C.Structure):
    _fields_ = [("probe_ms", C.c_float * 12), ("nprobed", C.c_int), ("chosen", C.c_int), ("allocated_bytes", C.c_size_t),
                ("probe_peak_bytes", C.c_size_t)]


class seeqdev_demux_t(C.Structure):
    _fields_ = [("line", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32), ("dist", C.c_uint16), ("pattern", C.c_uint8),
                ("margin", C.c_uint8)]


class seeqdev_demux_counts_t(C.Structure):
    _fields_ = [("nlines", C.c_uint64), ("nassigned", C.c_uint64), ("nambiguous", C.c_uint64)]


class seeqdev_insert_t(C.Structure):
    _fields_ = [("line", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32), ("ldist", C.c_uint16), ("rdist", C.c_uint16)]


class seeqdev_insert_counts_t(C.Structure):
    _fields_ = [("nlines", C.c_uint64), ("nleft", C.c_uint64), ("nright", C.c_uint64), ("nboth", C.c_uint64), ("ninserts", C.c_uint64),
                ("text_bytes", C.c_uint64)]


class seeqdev_tally_t(C.Structure):
    _fields_ = [("key", C.c_uint64), ("count", C.c_uint64)]


class seeqdev_tally_counts_t(C.Structure):
    _fields_ = [("nspans", C.c_uint64), ("ntallied", C.c_uint64), ("nlong", C.c_uint64), ("nforeign", C.c_uint64), ("ndistinct", C.c_uint64),
                ("max_len", C.c_uint32), ("passes", C.c_uint32)]


SEEQDEV_TALLY_INSERTS, SEEQDEV_TALLY_HITS, SEEQDEV_TALLY_MAX_LEN = 0, 1, 31
SEEQDEV_TALLY_DEMUX = 2             # seeqdevScanTallyHold only


class seeqdev_tally_pair_t(C.Structure):
    _fields_ = [("group", C.c_uint64), ("member", C.c_uint64), ("count", C.c_uint64)]


class seeqdev_tally_group_t(C.Structure):
    _fields_ = [("group", C.c_uint64), ("count", C.c_uint64), ("first", C.c_uint32), ("ndistinct", C.c_uint32)]


class seeqdev_tally_hold_counts_t(C.Structure):
    _fields_ = [("nspans", C.c_uint64), ("nheld", C.c_uint64), ("nlong", C.c_uint64), ("nforeign", C.c_uint64), ("nambiguous", C.c_uint64),
                ("max_len", C.c_uint32), ("key_bits", C.c_uint32)]


class seeqdev_tally_grouped_counts_t(C.Structure):
    _fields_ = [("nspans", C.c_uint64), ("npaired", C.c_uint64), ("nlong", C.c_uint64), ("nforeign", C.c_uint64), ("nungrouped", C.c_uint64),
                ("npairs", C.c_uint64), ("ngroups", C.c_uint64), ("max_len", C.c_uint32), ("passes", C.c_uint32)]


SEEQDEV_COLLAPSE_DIRECTIONAL, SEEQDEV_COLLAPSE_ANY = 0, 1


class seeqdev_tally_collapse_t(C.Structure):
    _fields_ = [("nroots", C.c_uint32), ("nabsorbed", C.c_uint32), ("absorbed_reads", C.c_uint64)]


class seeqdev_tally_collapse_counts_t(C.Structure):
    _fields_ = [("npairs", C.c_uint64), ("ngroups", C.c_uint64), ("nroots", C.c_uint64), ("nabsorbed", C.c_uint64), ("absorbed_reads", C.c_uint64),
                ("rule", C.c_uint32), ("max_len", C.c_uint32)]


class seeqdev_tally_library_counts_t(C.Structure):
    _fields_ = [("nspans", C.c_uint64), ("nassigned", C.c_uint64), ("nexact", C.c_uint64), ("ncorrected", C.c_uint64), ("nambiguous", C.c_uint64),
                ("nunknown", C.c_uint64), ("nlong", C.c_uint64), ("nforeign", C.c_uint64), ("ndistinct", C.c_uint64), ("key_bits", C.c_uint32),
                ("passes", C.c_uint32)]


SEEQDEV_LIBRARY_EXACT, SEEQDEV_LIBRARY_SUBST, SEEQDEV_LIBRARY_EDIT = 0, 1, 2


class seeqdev_tally_library_edits_t(C.Structure):
    _fields_ = [("nsubstituted", C.c_uint64), ("ninserted", C.c_uint64), ("ndeleted", C.c_uint64), ("reserved", C.c_uint64)]


class seeqdev_tally_append_counts_t(C.Structure):
    _fields_ = [("nrecords", C.c_uint64), ("nbefore", C.c_uint64), ("nheld", C.c_uint64), ("ndropped", C.c_uint64), ("width", C.c_uint32),
                ("key_bits", C.c_uint32), ("ncolumns", C.c_uint32), ("reserved", C.c_uint32)]


SEEQDEV_TALLY_COLUMNS = 8           # columns of a held key, the hold's own included


class seeqdev_tally_held_counts_t(C.Structure):
    _fields_ = [("nrecords", C.c_uint64), ("ncounted", C.c_uint64), ("nkeyless", C.c_uint64), ("nrepeat", C.c_uint64), ("ndistinct", C.c_uint64),
                ("nrows", C.c_uint64), ("key_bits", C.c_uint32), ("shift", C.c_uint32), ("passes", C.c_uint32), ("member_columns", C.c_uint32)]


class seeqdev_tally_dense_counts_t(C.Structure):
    _fields_ = [("ninside", C.c_uint64), ("noutside", C.c_uint64), ("inside_reads", C.c_uint64), ("outside_reads", C.c_uint64)]


SEEQDEV_TALLY_DENSE_MAX = 1 << 28   # cells of a dense matrix (seeqdevScanTallyHeldDense)
SEEQDEV_TALLY_GATED = 4             # the spans the context's last quality gate passed
SEEQDEV_QGATE_PASS, SEEQDEV_QGATE_LOW, SEEQDEV_QGATE_LONG, SEEQDEV_QGATE_FAR, SEEQDEV_QGATE_MISFIT = 0, 1, 2, 3, 4


class seeqdev_qgate_counts_t(C.Structure):
    _fields_ = [("nspans", C.c_uint64), ("npassed", C.c_uint64), ("nlow", C.c_uint64), ("nlong", C.c_uint64), ("nfar", C.c_uint64),
                ("nmisfit", C.c_uint64), ("low_bases", C.c_uint64)]


SEEQDEV_TALLY_ANCHORED = 5          # the spans of the context's last anchor call
SEEQDEV_ANCHOR_AFTER, SEEQDEV_ANCHOR_BEFORE, SEEQDEV_ANCHOR_LINE = 0, 1, 2
SEEQDEV_ANCHOR_KEPT, SEEQDEV_ANCHOR_SHORT, SEEQDEV_ANCHOR_FAR = 0, 1, 2


class seeqdev_anchor_counts_t(C.Structure):
    _fields_ = [("nspans", C.c_uint64), ("nkept", C.c_uint64), ("nshort", C.c_uint64), ("nfar", C.c_uint64), ("span_bytes", C.c_uint64)]


# Every symbol the three public headers declare (tests check the .so exports all of them).
EXPORTS = [
    # libseeq.h
    "seeqNew", "seeqFree", "seeqMatchIter", "seeqGetString", "seeqStringMatch", "seeqPrintError",
    "seeqAddMatch", "stackNew", "stackAddMatch", "recursive_merge", "seeqerr",
    # seeq.h
    "seeq", "seeqFileMatch", "seeqOpen", "seeqClose",
    # seeq_amd.h
    "seeqdevDeviceCount", "seeqdevSetDevice", "seeqdevLastError", "seeqdevPatternNew", "seeqdevPatternFree",
    "seeqdevPatternOf", "seeqdevScanNew", "seeqdevScanFree", "seeqdevScanReserve", "seeqdevScanRun",
    "seeqdevScanFetch", "seeqdevScanRecordsDevice", "seeqdevScanCopyRecords", "seeqdevScanHost",
    "seeqdevScanSetProfiling", "seeqdevScanLastTimes", "seeqdevScanLastLaunches", "seeqdevScanLastLaunchTimes", "seeqdevScanLastClockMHz", "seeqdevSynthReads",
    "seeqdevScanSetLineHint", "seeqdevScanLastPath", "seeqdevScanLastFilter", "seeqdevScanLastPackedQuad", "seeqdevScanCopyOffsets", "seeqdevHostAlloc", "seeqdevTextAlloc", "seeqdevTextAllocInfo", "seeqdevTextAllocFor", "seeqdevTextFree",
    "seeqdevHostFree", "seeqdevStringMatch", "seeqdevScanHostBegin", "seeqdevScanLastCopyMs", "seeqdevPatternDevice",
    "seeqdevScanRunMulti", "seeqdevScanHostMulti", "seeqdevScanMultiRecords", "seeqdevScanLastMulti", "seeqdevScanPacked", "seeqdevPackReads", "seeqdevPackReadsDevice",
    "seeqdevScanRunDemux", "seeqdevScanHostDemux", "seeqdevScanDemuxDevice", "seeqdevScanCopyDemux",
    "seeqdevPatternRevComp", "seeqdevScanRunStrands", "seeqdevScanHostStrands", "seeqdevScanLastStrandsMs",
    "seeqdevScanRunInserts", "seeqdevScanHostInserts", "seeqdevScanInsertsDevice", "seeqdevScanCopyInserts", "seeqdevScanCopyInsertOffsets",
    "seeqdevScanInsertText", "seeqdevScanLastInsertsMs",
    "seeqdevScanTally", "seeqdevScanTallyDevice", "seeqdevScanCopyTally", "seeqdevScanLastTallyMs", "seeqdevTallyKey", "seeqdevTallyDecode",
    "seeqdevScanTallyHold", "seeqdevScanTallyGrouped", "seeqdevScanTallyPairsDevice", "seeqdevScanTallyGroupsDevice", "seeqdevScanCopyTallyPairs",
    "seeqdevScanCopyTallyGroups", "seeqdevScanLastTallyGroupedMs",
    "seeqdevScanTallyCollapse", "seeqdevScanTallyParentsDevice", "seeqdevScanTallyCollapseDevice", "seeqdevScanCopyTallyParents",
    "seeqdevScanCopyTallyCollapse", "seeqdevScanLastTallyCollapseMs",
    "seeqdevScanSetLibrary", "seeqdevScanTallyLibrary", "seeqdevScanTallyHoldLibrary", "seeqdevScanSetLibraryMode", "seeqdevScanLastLibraryEdits",
    "seeqdevScanTallyHoldAppend", "seeqdevScanTallyHoldAppendLibrary", "seeqdevScanTallyHoldColumns", "seeqdevScanCopyHeld", "seeqdevTallySplit",
    "seeqdevScanTallyHeld", "seeqdevScanTallyHeldRowsDevice", "seeqdevScanCopyTallyHeldRows", "seeqdevScanTallyHeldDense", "seeqdevScanLastTallyHeldMs",
    "seeqdevTallyHeldCell",
    "seeqdevScanQualityGate", "seeqdevScanGatedDevice", "seeqdevScanCopyGated", "seeqdevScanCopyGatedOffsets", "seeqdevScanCopyGateKinds",
    "seeqdevScanLastQualityGateMs",
    "seeqdevScanAnchor", "seeqdevScanAnchoredDevice", "seeqdevScanCopyAnchored", "seeqdevScanCopyAnchoredOffsets", "seeqdevScanCopyAnchorKinds",
    "seeqdevScanLastAnchorMs",
    "seeqdevScanLastRuns", "seeqdevScanFallback", "seeqdevScanLastPlan",
]


def build(verbose=False):
    """Compile the library and the CLI in-tree (hipcc --offload-arch=gfx950)."""
    cmd = ["make", "-C", CSRC, "all"]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)


_lib = None


def _share_torch_hip_runtime():
    """torch wheels bundle their own libamdhip64.so.7; /opt/rocm has another with the same
    soname.  One process must use ONE HIP runtime, so when torch is installed its copy is
    loaded first (without importing torch) and libseeq_amd.so binds to it; C callers such as
    seeq_amd/bin/seeq simply use /opt/rocm's.  SEEQ_AMD_SYSTEM_HIP=1 disables this."""
    if os.environ.get("SEEQ_AMD_SYSTEM_HIP") == "1":
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(path):
        C.CDLL(path, mode=C.RTLD_GLOBAL)


def lib():
    """Load libseeq_amd.so (raises OSError with a clear message if it is not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError("%s is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "or `make -C seeq_amd/csrc`; seeq_amd has no fallback matcher" % LIB_PATH)
    _share_torch_hip_runtime()
    L = C.CDLL(LIB_PATH, use_errno=True)      # (C.get_errno(): the errno a failed call left -- device failures are errno's, seeqerr = 0)
    P = C.POINTER
    L.seeqNew.argtypes = [C.c_char_p, C.c_int, C.c_size_t]
    L.seeqNew.restype = P(seeq_t)
    L.seeqFree.argtypes = [P(seeq_t)]
    L.seeqFree.restype = None
    L.seeqMatchIter.argtypes = [P(seeq_t)]
    L.seeqMatchIter.restype = P(match_t)
    L.seeqGetString.argtypes = [P(seeq_t)]
    L.seeqGetString.restype = C.c_char_p
    L.seeqStringMatch.argtypes = [C.c_char_p, P(seeq_t), C.c_int]
    L.seeqStringMatch.restype = C.c_long
    L.seeqPrintError.argtypes = []
    L.seeqPrintError.restype = C.c_char_p
    L.seeqAddMatch.argtypes = [P(seeq_t), match_t]
    L.seeqAddMatch.restype = C.c_int
    L.seeqOpen.argtypes = [C.c_char_p]
    L.seeqOpen.restype = P(seeqfile_t)
    L.seeqClose.argtypes = [P(seeqfile_t)]
    L.seeqClose.restype = C.c_int
    L.seeqFileMatch.argtypes = [P(seeqfile_t), P(seeq_t), C.c_int, C.c_int]
    L.seeqFileMatch.restype = C.c_long
    L.seeqdevDeviceCount.argtypes = []
    L.seeqdevDeviceCount.restype = C.c_int
    L.seeqdevSetDevice.argtypes = [C.c_int]
    L.seeqdevSetDevice.restype = C.c_int
    L.seeqdevLastError.argtypes = []
    L.seeqdevLastError.restype = C.c_char_p
    L.seeqdevPatternNew.argtypes = [C.c_char_p, C.c_int, C.c_int]
    L.seeqdevPatternNew.restype = C.c_void_p
    L.seeqdevPatternFree.argtypes = [C.c_void_p]
    L.seeqdevPatternFree.restype = None
    L.seeqdevPatternOf.argtypes = [P(seeq_t)]
    L.seeqdevPatternOf.restype = C.c_void_p
    L.seeqdevScanNew.argtypes = [C.c_void_p]
    L.seeqdevScanNew.restype = C.c_void_p
    L.seeqdevScanFree.argtypes = [C.c_void_p]
    L.seeqdevScanFree.restype = None
    L.seeqdevScanReserve.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]
    L.seeqdevScanReserve.restype = C.c_int
    L.seeqdevScanRun.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    L.seeqdevScanRun.restype = C.c_int
    L.seeqdevScanFetch.argtypes = [C.c_void_p, P(seeqdev_counts_t)]
    L.seeqdevScanFetch.restype = C.c_int
    L.seeqdevScanRecordsDevice.argtypes = [C.c_void_p]
    L.seeqdevScanRecordsDevice.restype = C.c_void_p
    L.seeqdevScanCopyRecords.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
    L.seeqdevScanCopyRecords.restype = C.c_int
    L.seeqdevScanCopyOffsets.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
    L.seeqdevScanCopyOffsets.restype = C.c_int
    L.seeqdevScanHost.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_int,
                                  P(seeqdev_counts_t)]
    L.seeqdevScanHost.restype = C.c_int
    L.seeqdevScanSetProfiling.argtypes = [C.c_void_p, C.c_int]
    L.seeqdevScanSetProfiling.restype = C.c_int
    L.seeqdevScanLastTimes.argtypes = [C.c_void_p, P(C.c_float)]
    L.seeqdevScanLastTimes.restype = C.c_int
    L.seeqdevScanLastLaunches.argtypes = [C.c_void_p]
    L.seeqdevScanLastLaunches.restype = C.c_int
    L.seeqdevScanLastLaunchTimes.argtypes = [C.c_void_p, P(C.c_float), C.c_int]
    L.seeqdevScanLastLaunchTimes.restype = C.c_int
    L.seeqdevScanLastClockMHz.argtypes = [C.c_void_p]
    L.seeqdevScanLastClockMHz.restype = C.c_float
    L.seeqdevScanSetLineHint.argtypes = [C.c_void_p, C.c_double]
    L.seeqdevScanSetLineHint.restype = C.c_int
    L.seeqdevScanLastPath.argtypes = [C.c_void_p]
    L.seeqdevScanLastPath.restype = C.c_int
    L.seeqdevScanLastFilter.argtypes = [C.c_void_p]
    L.seeqdevScanLastFilter.restype = C.c_int
    L.seeqdevScanLastPlan.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.seeqdevScanLastPlan.restype = C.c_int
    L.seeqdevScanLastPackedQuad.argtypes = [C.c_void_p]
    L.seeqdevScanLastPackedQuad.restype = C.c_int
    L.seeqdevScanLastRuns.argtypes = [C.c_void_p]
    L.seeqdevScanLastRuns.restype = C.c_int
    L.seeqdevScanFallback.argtypes = [C.c_void_p, P(C.c_uint), P(C.c_int)]
    L.seeqdevScanFallback.restype = C.c_int
    L.seeqdevScanRunMulti.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    L.seeqdevScanRunMulti.restype = C.c_int
    L.seeqdevScanHostMulti.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    L.seeqdevScanHostMulti.restype = C.c_int
    L.seeqdevScanMultiRecords.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.seeqdevScanMultiRecords.restype = C.c_int
    L.seeqdevScanLastMulti.argtypes = [C.c_void_p]
    L.seeqdevScanLastMulti.restype = C.c_int
    L.seeqdevScanRunDemux.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_size_t, C.c_int, P(seeqdev_demux_counts_t),
                                      C.POINTER(C.c_uint64)]
    L.seeqdevScanRunDemux.restype = C.c_int
    L.seeqdevScanHostDemux.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.c_size_t, C.c_int, P(seeqdev_demux_counts_t),
                                       C.POINTER(C.c_uint64)]
    L.seeqdevScanHostDemux.restype = C.c_int
    L.seeqdevScanDemuxDevice.argtypes = [C.c_void_p]
    L.seeqdevScanDemuxDevice.restype = C.c_void_p
    L.seeqdevScanCopyDemux.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
    L.seeqdevScanCopyDemux.restype = C.c_int
    L.seeqdevPatternRevComp.argtypes = [C.c_void_p]
    L.seeqdevPatternRevComp.restype = C.c_void_p
    L.seeqdevScanRunStrands.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, P(seeqdev_counts_t), C.POINTER(C.c_uint64)]
    L.seeqdevScanRunStrands.restype = C.c_int
    L.seeqdevScanHostStrands.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_int, P(seeqdev_counts_t), C.POINTER(C.c_uint64)]
    L.seeqdevScanHostStrands.restype = C.c_int
    L.seeqdevScanLastStrandsMs.argtypes = [C.c_void_p, P(C.c_float)]
    L.seeqdevScanLastStrandsMs.restype = C.c_int
    L.seeqdevScanRunInserts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32,
                                        P(seeqdev_insert_counts_t)]
    L.seeqdevScanRunInserts.restype = C.c_int
    L.seeqdevScanHostInserts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32,
                                         P(seeqdev_insert_counts_t)]
    L.seeqdevScanHostInserts.restype = C.c_int
    L.seeqdevScanInsertsDevice.argtypes = [C.c_void_p]
    L.seeqdevScanInsertsDevice.restype = C.c_void_p
    L.seeqdevScanCopyInserts.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
    L.seeqdevScanCopyInserts.restype = C.c_int
    L.seeqdevScanCopyInsertOffsets.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
    L.seeqdevScanCopyInsertOffsets.restype = C.c_int
    L.seeqdevScanInsertText.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, P(C.c_uint64)]
    L.seeqdevScanInsertText.restype = C.c_int
    L.seeqdevScanLastInsertsMs.argtypes = [C.c_void_p, P(C.c_float)]
    L.seeqdevScanLastInsertsMs.restype = C.c_int
    L.seeqdevScanTally.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, P(seeqdev_tally_counts_t)]
    L.seeqdevScanTally.restype = C.c_int
    L.seeqdevScanTallyDevice.argtypes = [C.c_void_p]
    L.seeqdevScanTallyDevice.restype = C.c_void_p
    L.seeqdevScanCopyTally.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
    L.seeqdevScanCopyTally.restype = C.c_int
    L.seeqdevScanLastTallyMs.argtypes = [C.c_void_p, P(C.c_float)]
    L.seeqdevScanLastTallyMs.restype = C.c_int
    L.seeqdevTallyKey.argtypes = [C.c_char_p, C.c_size_t, P(C.c_uint64)]
    L.seeqdevTallyKey.restype = C.c_int
    L.seeqdevTallyDecode.argtypes = [C.c_uint64, C.c_char_p]
    L.seeqdevTallyDecode.restype = C.c_int
    L.seeqdevScanTallyHold.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, P(seeqdev_tally_hold_counts_t)]
    L.seeqdevScanTallyHold.restype = C.c_int
    L.seeqdevScanTallyGrouped.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, P(seeqdev_tally_grouped_counts_t)]
    L.seeqdevScanTallyGrouped.restype = C.c_int
    for name in ("seeqdevScanTallyPairsDevice", "seeqdevScanTallyGroupsDevice"):
        getattr(L, name).argtypes = [C.c_void_p]
        getattr(L, name).restype = C.c_void_p
    for name in ("seeqdevScanCopyTallyPairs", "seeqdevScanCopyTallyGroups"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
        getattr(L, name).restype = C.c_int
    L.seeqdevScanLastTallyGroupedMs.argtypes = [C.c_void_p, P(C.c_float)]
    L.seeqdevScanLastTallyGroupedMs.restype = C.c_int
    L.seeqdevScanTallyCollapse.argtypes = [C.c_void_p, C.c_int, P(seeqdev_tally_collapse_counts_t)]
    L.seeqdevScanTallyCollapse.restype = C.c_int
    for name in ("seeqdevScanTallyParentsDevice", "seeqdevScanTallyCollapseDevice"):
        getattr(L, name).argtypes = [C.c_void_p]
        getattr(L, name).restype = C.c_void_p
    for name in ("seeqdevScanCopyTallyParents", "seeqdevScanCopyTallyCollapse"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
        getattr(L, name).restype = C.c_int
    L.seeqdevScanLastTallyCollapseMs.argtypes = [C.c_void_p, P(C.c_float)]
    L.seeqdevScanLastTallyCollapseMs.restype = C.c_int
    L.seeqdevScanSetLibrary.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.seeqdevScanSetLibrary.restype = C.c_int
    L.seeqdevScanSetLibraryMode.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.seeqdevScanSetLibraryMode.restype = C.c_int
    L.seeqdevScanLastLibraryEdits.argtypes = [C.c_void_p, P(seeqdev_tally_library_edits_t)]
    L.seeqdevScanLastLibraryEdits.restype = C.c_int
    for name in ("seeqdevScanTallyLibrary", "seeqdevScanTallyHoldLibrary"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, P(seeqdev_tally_library_counts_t)]
        getattr(L, name).restype = C.c_int
    L.seeqdevScanTallyHoldAppend.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, P(seeqdev_tally_hold_counts_t), P(seeqdev_tally_append_counts_t)]
    L.seeqdevScanTallyHoldAppend.restype = C.c_int
    L.seeqdevScanTallyHoldAppendLibrary.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, P(seeqdev_tally_library_counts_t), P(seeqdev_tally_append_counts_t)]
    L.seeqdevScanTallyHoldAppendLibrary.restype = C.c_int
    L.seeqdevScanTallyHoldColumns.argtypes = [C.c_void_p, P(C.c_uint32), C.c_int]
    L.seeqdevScanTallyHoldColumns.restype = C.c_int
    L.seeqdevScanCopyHeld.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
    L.seeqdevScanCopyHeld.restype = C.c_int
    L.seeqdevTallySplit.argtypes = [C.c_uint64, P(C.c_uint32), C.c_int, P(C.c_uint64)]
    L.seeqdevTallySplit.restype = C.c_int
    L.seeqdevScanTallyHeld.argtypes = [C.c_void_p, C.c_int, P(seeqdev_tally_held_counts_t)]
    L.seeqdevScanTallyHeld.restype = C.c_int
    L.seeqdevScanTallyHeldRowsDevice.argtypes = [C.c_void_p]
    L.seeqdevScanTallyHeldRowsDevice.restype = C.c_void_p
    L.seeqdevScanCopyTallyHeldRows.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
    L.seeqdevScanCopyTallyHeldRows.restype = C.c_int
    L.seeqdevScanTallyHeldDense.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, P(seeqdev_tally_dense_counts_t)]
    L.seeqdevScanTallyHeldDense.restype = C.c_int
    L.seeqdevScanLastTallyHeldMs.argtypes = [C.c_void_p, P(C.c_float)]
    L.seeqdevScanLastTallyHeldMs.restype = C.c_int
    L.seeqdevTallyHeldCell.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, P(C.c_uint64)]
    L.seeqdevTallyHeldCell.restype = C.c_int
    L.seeqdevScanQualityGate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(seeqdev_qgate_counts_t)]
    L.seeqdevScanQualityGate.restype = C.c_int
    L.seeqdevScanGatedDevice.argtypes = [C.c_void_p]
    L.seeqdevScanGatedDevice.restype = C.c_void_p
    for name in ("seeqdevScanCopyGated", "seeqdevScanCopyGatedOffsets", "seeqdevScanCopyGateKinds"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
        getattr(L, name).restype = C.c_int
    L.seeqdevScanLastQualityGateMs.argtypes = [C.c_void_p, P(C.c_float)]
    L.seeqdevScanLastQualityGateMs.restype = C.c_int
    L.seeqdevScanAnchor.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, P(seeqdev_anchor_counts_t)]
    L.seeqdevScanAnchor.restype = C.c_int
    L.seeqdevScanAnchoredDevice.argtypes = [C.c_void_p]
    L.seeqdevScanAnchoredDevice.restype = C.c_void_p
    for name in ("seeqdevScanCopyAnchored", "seeqdevScanCopyAnchoredOffsets", "seeqdevScanCopyAnchorKinds"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
        getattr(L, name).restype = C.c_int
    L.seeqdevScanLastAnchorMs.argtypes = [C.c_void_p, P(C.c_float)]
    L.seeqdevScanLastAnchorMs.restype = C.c_int
    L.seeqdevScanPacked.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(seeqdev_packed_t), C.c_int, C.c_int]
    L.seeqdevScanPacked.restype = C.c_int
    L.seeqdevPackReads.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.seeqdevPackReads.restype = C.c_long
    L.seeqdevPackReadsDevice.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.seeqdevPackReadsDevice.restype = C.c_int
    L.seeqdevHostAlloc.argtypes = [C.c_size_t]
    L.seeqdevHostAlloc.restype = C.c_void_p
    L.seeqdevHostFree.argtypes = [C.c_void_p]
    L.seeqdevHostFree.restype = None
    L.seeqdevTextAlloc.argtypes = [C.c_size_t, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.seeqdevTextAlloc.restype = C.c_void_p
    L.seeqdevTextAllocInfo.argtypes = [C.c_size_t, C.c_int, C.POINTER(seeqdev_textinfo_t)]
    L.seeqdevTextAllocInfo.restype = C.c_void_p
    L.seeqdevTextAllocFor.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(seeqdev_textinfo_t)]
    L.seeqdevTextAllocFor.restype = C.c_void_p
    L.seeqdevTextFree.argtypes = [C.c_void_p]
    L.seeqdevTextFree.restype = None
    L.seeqdevSynthReads.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_char_p, C.c_int, C.c_int,
                                    C.c_uint64, C.c_void_p]
    L.seeqdevSynthReads.restype = C.c_int
    _lib = L
    return L


def seeqerr():
    return C.c_int.in_dll(lib(), "seeqerr").value


def error_text():
    L = lib()
    msg = L.seeqPrintError().decode(errors="replace")
    dev = L.seeqdevLastError().decode(errors="replace")
    return msg + (" [" + dev + "]" if dev and seeqerr() == 0 else "")
