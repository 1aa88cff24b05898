"""ctypes loader for libbella_hip.so (the C ABI of include/bella_hip.h).

There is no fallback: if the library is missing or no gfx950 device is present the product path raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.path.join(HERE, "libbella_hip.so")

PAIR_DT = np.dtype([("rid", "<u4"), ("cid", "<u4"), ("count", "<u2"), ("seedH", "<u2"), ("seedV", "<u2"), ("flags", "<u2")])
EXT_DT = np.dtype([("nbins", "<u2"), ("support", "<u2"), ("binov", "<u2"), ("pad", "<u2")])
ALN_DT = np.dtype([("score", "<i4"), ("begH", "<i4"), ("endH", "<i4"), ("begV", "<i4"), ("endV", "<i4"), ("ov", "<u2"),
                   ("strand", "u1"), ("passed", "u1"), ("steps", "<u4"), ("flagged", "<u4")])
SEED_DT = np.dtype([("rid", "<u4"), ("cid", "<u4"), ("seedH", "<u2"), ("seedV", "<u2")])
TRACE_DT = np.dtype([("op_off", "<u8"), ("nops", "<u4"), ("band", "<u4"), ("score", "<i4"), ("tbegH", "<i4"), ("tendH", "<i4"), ("tbegV", "<i4"),
                     ("tendV", "<i4"), ("n_eq", "<u4"), ("n_x", "<u4"), ("n_ins", "<u4"), ("n_del", "<u4"), ("widened", "<u4")])
assert TRACE_DT.itemsize == 56
CONS_DT = np.dtype([("len_before", "<u4"), ("len_after", "<u4"), ("substituted", "<u4"), ("deleted", "<u4"), ("inserted", "<u4"), ("covered", "<u4"),
                    ("depth_sum", "<u8")])
assert CONS_DT.itemsize == 32
OVL_DT = np.dtype([("cid", "<u4"), ("rid", "<u4"), ("begV", "<i4"), ("endV", "<i4"), ("begH", "<i4"), ("endH", "<i4"), ("score", "<i4"),
                   ("strand", "u1"), ("pad", "u1", (3,))])
EDGE_DT = np.dtype([("src", "<u4"), ("dst", "<u4"), ("len", "<u4"), ("ovl", "<u4"), ("rec", "<u4"), ("flags", "<u4")])
assert OVL_DT.itemsize == 32 and EDGE_DT.itemsize == 24
LINK_DT = np.dtype([("a", "<u4"), ("b", "<u4"), ("ovl", "<u4"), ("rec", "<u4"), ("flags", "<u4"), ("edge", "<u4")])
assert LINK_DT.itemsize == 24
LINK_A_MINUS, LINK_B_MINUS, MAX_TIP_ROUNDS = 1, 2, 16
POLISH_DT = np.dtype([("len_before", "<u8"), ("len_after", "<u8"), ("substituted", "<u8"), ("deleted", "<u8"), ("inserted", "<u8"), ("covered", "<u8"),
                      ("depth_sum", "<u8")])
assert POLISH_DT.itemsize == 56
PLACE_DT = np.dtype([("unitig", "<u4"), ("orient", "<u4"), ("s", "<i8"), ("e", "<i8"), ("anchor", "<u4"), ("status", "<u4"), ("band", "<u4"), ("n_eq", "<u4"), ("n_x", "<u4"),
                     ("n_ins", "<u4"), ("n_del", "<u4"), ("score", "<i4"), ("q_begin", "<i8"), ("q_end", "<i8"), ("op_off", "<u8"), ("nops", "<u4"), ("pad", "<u4")])
assert PLACE_DT.itemsize == 88
LINK_ALN_DT = np.dtype([("status", "<u4"), ("band", "<u4"), ("score", "<i4"), ("ovl_a", "<u4"), ("ovl_b", "<u4"), ("n_eq", "<u4"), ("n_x", "<u4"), ("n_ins", "<u4"),
                        ("n_del", "<u4"), ("mate", "<u4"), ("op_off", "<u8"), ("nops", "<u4"), ("derived", "<u4")])
assert LINK_ALN_DT.itemsize == 56
LINK_ALIGNED, LINK_EMPTY, LINK_BAND_CAPPED, LINK_LOW_IDENTITY, LINK_SELF = range(5)
LINK_NO_MATE = 0xFFFFFFFF
REALIGN_NONE, REALIGN_VOTED, REALIGN_UNPLACED, REALIGN_OUTSIDE, REALIGN_BAND_CAPPED, REALIGN_LOW_IDENTITY = range(6)
TRACE_PASSED_ONLY, TRACE_DROP_OPS, TRACE_PILEUP, TRACE_NORMALIZE = 1, 2, 4, 8
VOTE_PAIR_DT = np.dtype([("rid", "<u4"), ("cid", "<u4"), ("tbegV", "<i4"), ("tbegH", "<i4"), ("op_off", "<u8"), ("nops", "<u4"), ("strand", "u1"), ("pad", "u1", (3,))])
assert VOTE_PAIR_DT.itemsize == 32
CLIP_DEFAULT_IDENTITY = 650
CLIP_RES_DT = np.dtype([("first_run", "<u4"), ("nruns", "<u4"), ("begV", "<i4"), ("endV", "<i4"), ("begH", "<i4"), ("endH", "<i4"), ("n_eq", "<u4"), ("n_x", "<u4"),
                        ("n_ins", "<u4"), ("n_del", "<u4"), ("score", "<i4"), ("pad", "<u4"), ("clip_score", "<i8")])
assert CLIP_RES_DT.itemsize == 56
PILEUP_COUNTERS = 9      # per base: votes for A C G T, del, one inserted A C G T in the junction before the base
assert PAIR_DT.itemsize == 16 and EXT_DT.itemsize == 8 and ALN_DT.itemsize == 32 and SEED_DT.itemsize == 12


class Params(C.Structure):
    _fields_ = [("kmer_size", C.c_uint16), ("bin_size", C.c_uint16), ("xdrop", C.c_uint16), ("skip_alignment", C.c_uint16),
                ("error_rate", C.c_double), ("delta_chernoff", C.c_double)]


class WriteStats(C.Structure):
    _fields_ = [("lines", C.c_uint64), ("bytes", C.c_uint64), ("aligned_pairs", C.c_uint64), ("aligned_bases", C.c_uint64),
                ("total_read_len", C.c_uint64), ("bases_passed", C.c_uint64), ("bases_failed", C.c_uint64), ("seconds", C.c_double),
                ("format_seconds", C.c_double), ("threads", C.c_uint32), ("pad", C.c_uint32)]


class IngestStats(C.Structure):
    _fields_ = [("file_bytes", C.c_uint64), ("bases", C.c_uint64), ("reads", C.c_uint32), ("threads", C.c_uint32),
                ("index_ms", C.c_double), ("upload_ms", C.c_double)]


class Timings(C.Structure):
    _fields_ = [("assemble_ms", C.c_float), ("symbolic_ms", C.c_float), ("spgemm_ms", C.c_float), ("fold_ms", C.c_float),
                ("compact_ms", C.c_float), ("xdrop_ms", C.c_float), ("overlap_total_ms", C.c_float), ("spgemm_launches", C.c_uint32),
                ("kcount_ms", C.c_float), ("retry_columns", C.c_uint32), ("overflow_pairs", C.c_uint32), ("layout_ms", C.c_float),
                ("rows_ms", C.c_float), ("lane_order", C.c_uint32), ("expand_ms", C.c_float), ("numeric_passes", C.c_uint32),
                ("symbolic_passes", C.c_uint32), ("wide_batches", C.c_uint32), ("numeric_columns", C.c_uint64)]


class Memory(C.Structure):
    _fields_ = [("reads_bytes", C.c_uint64), ("matrix_bytes", C.c_uint64), ("layout_A_bytes", C.c_uint64), ("layout_B_bytes", C.c_uint64),
                ("rowlist_bytes", C.c_uint64), ("pass_bytes", C.c_uint64), ("other_bytes", C.c_uint64), ("owned_nnz", C.c_uint64),
                ("layout_shared", C.c_uint64), ("live_nnz", C.c_uint64)]


class TraceStats(C.Structure):
    _fields_ = [("dp_ms", C.c_double), ("walk_ms", C.c_double), ("total_ms", C.c_double), ("pairs", C.c_uint64), ("extensions", C.c_uint64),
                ("widened_extensions", C.c_uint64), ("repeated_pairs", C.c_uint64), ("dp_cells", C.c_uint64), ("dir_bytes", C.c_uint64), ("dir_bytes_peak", C.c_uint64),
                ("ops", C.c_uint64), ("batches", C.c_uint32), ("band0", C.c_uint32), ("vote_ms", C.c_double), ("votes", C.c_uint64),
                ("ops_host_bytes", C.c_uint64)]


class VoteStats(C.Structure):
    _fields_ = [("pairs", C.c_uint64), ("runs", C.c_uint64), ("gap_runs", C.c_uint64), ("shifted_runs", C.c_uint64), ("shifted_columns", C.c_uint64),
                ("votes", C.c_uint64), ("vote_ms", C.c_double), ("normalized", C.c_uint32), ("pad", C.c_uint32)]


class ClipParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("identity", C.c_uint32)]


class ClipStats(C.Structure):
    _fields_ = [("pairs", C.c_uint64), ("clipped", C.c_uint64), ("emptied", C.c_uint64), ("runs_before", C.c_uint64), ("runs_after", C.c_uint64),
                ("columns_before", C.c_uint64), ("columns_after", C.c_uint64), ("bases_v_removed", C.c_uint64), ("bases_h_removed", C.c_uint64),
                ("identity", C.c_uint32), ("pad", C.c_uint32), ("clip_ms", C.c_double)]


class ConsensusParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_depth", C.c_uint32)]


class GraphParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_overlap", C.c_uint32), ("max_overhang", C.c_uint32), ("overhang_permille", C.c_uint32),
                ("fuzz", C.c_uint32)]


class GraphStats(C.Structure):
    _fields_ = [("records", C.c_uint64), ("n_short", C.c_uint64), ("n_internal", C.c_uint64), ("contained_reads", C.c_uint64),
                ("edges_all", C.c_uint64), ("edges_kept", C.c_uint64), ("edges_reduced", C.c_uint64), ("edges_final", C.c_uint64),
                ("max_degree", C.c_uint32), ("overcap_vertices", C.c_uint32), ("classify_ms", C.c_double), ("sort_ms", C.c_double),
                ("reduce_ms", C.c_double), ("host_ms", C.c_double)]


class GraphCleanParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_tip_reads", C.c_uint32), ("tip_rounds", C.c_uint32)]


class UnitigStats(C.Structure):
    _fields_ = [("unitigs", C.c_uint64), ("vertices", C.c_uint64), ("links", C.c_uint64), ("total_bases", C.c_uint64), ("circular", C.c_uint64),
                ("largest", C.c_uint64), ("n50", C.c_uint64), ("reads_removed", C.c_uint64), ("edges_removed", C.c_uint64), ("rounds", C.c_uint32),
                ("rank_rounds", C.c_uint32), ("tips_per_round", C.c_uint32 * MAX_TIP_ROUNDS), ("reads_per_round", C.c_uint32 * MAX_TIP_ROUNDS),
                ("cycle_vertices", C.c_uint64), ("gather_bytes", C.c_uint64), ("clean_ms", C.c_double), ("rank_ms", C.c_double), ("gather_ms", C.c_double)]


MAX_BUBBLE_READS = 255
MAX_BUBBLE_ROUNDS = 16


class GraphBubbleParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_bubble_reads", C.c_uint32), ("max_bubble_dist", C.c_uint32), ("bubble_rounds", C.c_uint32)]


class BubbleStats(C.Structure):
    _fields_ = [("reads_removed", C.c_uint64), ("edges_removed", C.c_uint64), ("rounds", C.c_uint32), ("pad", C.c_uint32),
                ("sources", C.c_uint32 * MAX_BUBBLE_ROUNDS), ("found", C.c_uint32 * MAX_BUBBLE_ROUNDS), ("popped", C.c_uint32 * MAX_BUBBLE_ROUNDS),
                ("reads_per_round", C.c_uint32 * MAX_BUBBLE_ROUNDS), ("edges_per_round", C.c_uint32 * MAX_BUBBLE_ROUNDS), ("pop_ms", C.c_double)]


class GraphWeakParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("ratio_permille", C.c_uint32)]


class WeakStats(C.Structure):
    _fields_ = [("forks", C.c_uint64), ("weak", C.c_uint64), ("edges_removed", C.c_uint64), ("ratio_permille", C.c_uint32), ("cut_ms", C.c_double)]


class PolishParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_depth", C.c_uint32)]


class RealignParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("band0", C.c_uint32), ("band_max", C.c_uint32), ("min_identity", C.c_uint32), ("min_depth", C.c_uint32),
                ("keep_ops", C.c_uint32)]


class RealignStats(C.Structure):
    _fields_ = [("round", C.c_uint32), ("batches", C.c_uint32), ("backbone", C.c_uint64), ("contained", C.c_uint64), ("unplaced", C.c_uint64), ("outside", C.c_uint64),
                ("band_capped", C.c_uint64), ("low_identity", C.c_uint64), ("voted", C.c_uint64), ("repeated", C.c_uint64), ("dp_cells", C.c_uint64),
                ("dir_bytes_peak", C.c_uint64), ("votes", C.c_uint64), ("bases_before", C.c_uint64), ("bases_after", C.c_uint64), ("substituted", C.c_uint64),
                ("deleted", C.c_uint64), ("inserted", C.c_uint64), ("place_ms", C.c_double), ("dp_ms", C.c_double), ("walk_ms", C.c_double), ("vote_ms", C.c_double),
                ("decide_ms", C.c_double)]


class LinkParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("band0", C.c_uint32), ("band_max", C.c_uint32), ("min_identity", C.c_uint32)]


class LinkStats(C.Structure):
    _fields_ = [("links", C.c_uint64), ("aligned", C.c_uint64), ("empty", C.c_uint64), ("band_capped", C.c_uint64), ("low_identity", C.c_uint64), ("self", C.c_uint64),
                ("derived", C.c_uint64), ("overlap_before", C.c_uint64), ("overlap_after", C.c_uint64), ("jobs", C.c_uint64), ("dp_cells", C.c_uint64), ("ops", C.c_uint64),
                ("batches", C.c_uint32), ("pad", C.c_uint32), ("pack_ms", C.c_double), ("dp_ms", C.c_double), ("walk_ms", C.c_double)]


ALIGN_GLOBAL, ALIGN_SEMIGLOBAL, ALIGN_DOVETAIL = range(3)
ALIGN_MODES = {"global": ALIGN_GLOBAL, "semiglobal": ALIGN_SEMIGLOBAL, "dovetail": ALIGN_DOVETAIL}
ALIGN_ALIGNED, ALIGN_BAND_CAPPED, ALIGN_TOO_LARGE = range(3)
ALIGN_PAIR_RC = 1
ALIGN_PAIR_DT = np.dtype([("q_off", "<u8"), ("t_off", "<u8"), ("q_len", "<u4"), ("t_len", "<u4"), ("flags", "<u4"), ("centre", "<i4")])
ALIGN_RES_DT = np.dtype([("status", "<u4"), ("band", "<u4"), ("widened", "<u4"), ("score", "<i4"), ("q_begin", "<u4"), ("q_end", "<u4"), ("t_begin", "<u4"), ("t_end", "<u4"),
                         ("n_eq", "<u4"), ("n_x", "<u4"), ("n_ins", "<u4"), ("n_del", "<u4"), ("op_off", "<u8"), ("nops", "<u4"), ("pad", "<u4")])
assert ALIGN_PAIR_DT.itemsize == 32 and ALIGN_RES_DT.itemsize == 64


class AlignParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_uint32), ("band0", C.c_uint32), ("band_max", C.c_uint32)]


class AlignPair(C.Structure):
    _fields_ = [("q_off", C.c_uint64), ("t_off", C.c_uint64), ("q_len", C.c_uint32), ("t_len", C.c_uint32), ("flags", C.c_uint32), ("centre", C.c_int32)]


class AlignResult(C.Structure):
    _fields_ = [("status", C.c_uint32), ("band", C.c_uint32), ("widened", C.c_uint32), ("score", C.c_int32), ("q_begin", C.c_uint32), ("q_end", C.c_uint32),
                ("t_begin", C.c_uint32), ("t_end", C.c_uint32), ("n_eq", C.c_uint32), ("n_x", C.c_uint32), ("n_ins", C.c_uint32), ("n_del", C.c_uint32),
                ("op_off", C.c_uint64), ("nops", C.c_uint32), ("pad", C.c_uint32)]


class AlignStats(C.Structure):
    _fields_ = [("pairs", C.c_uint64), ("aligned", C.c_uint64), ("band_capped", C.c_uint64), ("too_large", C.c_uint64), ("repeated", C.c_uint64), ("dp_cells", C.c_uint64),
                ("ops", C.c_uint64), ("batches", C.c_uint32), ("mode", C.c_uint32), ("pack_ms", C.c_double), ("dp_ms", C.c_double), ("walk_ms", C.c_double),
                ("total_ms", C.c_double)]


class AlignScoring(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("match", C.c_uint32), ("mismatch", C.c_uint32), ("gap_open", C.c_uint32), ("gap_extend", C.c_uint32), ("reserved", C.c_uint32)]


assert C.sizeof(AlignPair) == ALIGN_PAIR_DT.itemsize and C.sizeof(AlignResult) == ALIGN_RES_DT.itemsize and C.sizeof(AlignStats) == 96 and C.sizeof(AlignScoring) == 24


class RecorrectParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("band0", C.c_uint32), ("band_max", C.c_uint32), ("min_identity", C.c_uint32), ("min_depth", C.c_uint32),
                ("keep_ops", C.c_uint32)]


class RecorrectStats(C.Structure):
    _fields_ = [("round", C.c_uint32), ("batches", C.c_uint32), ("jobs", C.c_uint64), ("none", C.c_uint64), ("band_capped", C.c_uint64), ("low_identity", C.c_uint64),
                ("voted", C.c_uint64), ("dp_cells", C.c_uint64), ("dir_bytes_peak", C.c_uint64), ("votes", C.c_uint64), ("bases_before", C.c_uint64),
                ("bases_after", C.c_uint64), ("substituted", C.c_uint64), ("deleted", C.c_uint64), ("inserted", C.c_uint64), ("place_ms", C.c_double),
                ("dp_ms", C.c_double), ("walk_ms", C.c_double), ("vote_ms", C.c_double), ("decide_ms", C.c_double)]


RECJOB_DT = np.dtype([("record", "<u4"), ("side", "<u4"), ("target", "<u4"), ("query", "<u4"), ("orient", "<u4"), ("status", "<u4"), ("qbeg", "<u4"), ("qend", "<u4"),
                      ("s", "<i8"), ("e", "<i8"), ("band", "<u4"), ("n_eq", "<u4"), ("n_x", "<u4"), ("n_ins", "<u4"), ("n_del", "<u4"), ("score", "<i4"), ("q_begin", "<i8"),
                      ("q_end", "<i8"), ("op_off", "<u8"), ("nops", "<u4"), ("pad", "<u4")])
assert RECJOB_DT.itemsize == 104 and C.sizeof(RecorrectStats) == 152
RECORRECT_ANCHOR_STEP = 256


class PolishStats(C.Structure):
    _fields_ = [("unitigs", C.c_uint64), ("vertices", C.c_uint64), ("bases_before", C.c_uint64), ("bases_after", C.c_uint64), ("substituted", C.c_uint64),
                ("deleted", C.c_uint64), ("inserted", C.c_uint64), ("covered", C.c_uint64), ("depth_sum", C.c_uint64), ("table_bytes", C.c_uint64),
                ("min_depth", C.c_uint32), ("tiles", C.c_uint32), ("decide_ms", C.c_double), ("write_ms", C.c_double)]


class GraphTrimParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_depth", C.c_uint32), ("end_clip", C.c_uint32), ("min_span", C.c_uint32)]


class ReadClip(C.Structure):
    _fields_ = [("beg", C.c_uint32), ("end", C.c_uint32), ("nregions", C.c_uint32), ("max_depth", C.c_uint32)]


CLIP_DT = np.dtype([("beg", "<u4"), ("end", "<u4"), ("nregions", "<u4"), ("max_depth", "<u4")])
assert CLIP_DT.itemsize == 16 == C.sizeof(ReadClip)


class TrimStats(C.Structure):
    _fields_ = [("intervals", C.c_uint64), ("reads_clipped", C.c_uint64), ("reads_uncovered", C.c_uint64), ("reads_multi", C.c_uint64),
                ("bases_before", C.c_uint64), ("bases_after", C.c_uint64), ("records_outside", C.c_uint64), ("events_ms", C.c_double),
                ("sort_ms", C.c_double), ("sweep_ms", C.c_double), ("host_ms", C.c_double)]


# every symbol include/bella_hip.h declares: (name, restype, argtypes)
vp = C.c_void_p
SIGNATURES = [
    ("bella_hip_abi_version", C.c_int, []),
    ("bella_hip_device_count", C.c_int, []),
    ("bella_hip_init", C.c_int, [C.c_int, C.POINTER(vp)]),
    ("bella_hip_destroy", None, [vp]),
    ("bella_hip_strerror", C.c_char_p, [C.c_int]),
    ("bella_hip_last_error", C.c_char_p, [vp]),
    ("bella_hip_set_reads", C.c_int, [vp, vp, vp, C.c_uint32]),
    ("bella_hip_load_fastq", C.c_int, [vp, C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    ("bella_hip_load_fastq_list", C.c_int, [vp, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    ("bella_hip_get_ingest_stats", C.c_int, [vp, C.c_void_p]),
    ("bella_hip_get_read_names", C.c_int, [vp, vp, C.c_uint64, vp, C.POINTER(C.c_uint64)]),
    ("bella_hip_get_read_lengths", C.c_int, [vp, vp]),
    ("bella_hip_count_kmers", C.c_int, [vp, C.c_uint16, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_uint64)]),
    ("bella_hip_count_syncmers", C.c_int, [vp, C.c_uint16, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint64)]),
    ("bella_hip_count_minimizers", C.c_int, [vp, C.c_uint16, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("bella_hip_get_dictionary", C.c_int, [vp, vp, vp]),
    ("bella_hip_get_tuples", C.c_int, [vp, vp, vp, vp]),
    ("bella_hip_get_count_stats", C.c_int, [vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("bella_hip_get_assemble_stats", C.c_int, [vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("bella_hip_assemble_counted", C.c_int, [vp]),
    ("bella_hip_assemble_counted_panel", C.c_int, [vp, C.c_uint32, C.c_uint32]),
    ("bella_hip_assemble_tuples", C.c_int, [vp, C.c_uint16, C.c_uint32, C.c_uint64, vp, vp, vp]),
    ("bella_hip_set_B", C.c_int, [vp, C.c_uint16, C.c_uint32, vp, vp, vp]),
    ("bella_hip_assemble_panel", C.c_int, [vp, C.c_uint16, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp, vp]),
    ("bella_hip_set_B_panel", C.c_int, [vp, C.c_uint16, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]),
    ("bella_hip_comm_id", C.c_int, [vp]),
    ("bella_hip_comm_init", C.c_int, [vp, C.c_int, C.c_int, vp]),
    ("bella_hip_comm_destroy", C.c_int, [vp]),
    ("bella_hip_comm_available", C.c_int, []),
    ("bella_hip_comm_id_local", C.c_int, [vp]),
    ("bella_hip_comm_init_local", C.c_int, [vp, C.c_int, C.c_int, vp]),
    ("bella_hip_allgather_panels", C.c_int, [vp]),
    ("bella_hip_count_kmers_dist", C.c_int, [vp, C.c_uint16, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("bella_hip_panel_device_ptrs", C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(vp),
                                               C.POINTER(vp), C.POINTER(vp)]),
    ("bella_hip_set_B_device", C.c_int, [vp, C.c_uint16, C.c_uint32, vp, vp, vp, C.c_uint64]),
    ("bella_hip_get_B", C.c_int, [vp, C.POINTER(C.c_uint64), vp, vp, vp]),
    ("bella_hip_set_partition", C.c_int, [vp, C.c_uint32, C.c_uint32]),
    ("bella_hip_set_column_range", C.c_int, [vp, C.c_uint32, C.c_uint32]),
    ("bella_hip_overlap", C.c_int, [vp, C.POINTER(Params), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("bella_hip_count_pairs", C.c_int, [vp, C.POINTER(Params), vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("bella_hip_get_pairs", C.c_int, [vp, vp, vp, vp]),
    ("bella_hip_align_pairs", C.c_int, [vp, C.POINTER(Params), C.POINTER(C.c_uint64)]),
    ("bella_hip_get_alignments", C.c_int, [vp, vp]),
    ("bella_hip_xdrop_batch", C.c_int, [vp, vp, C.c_uint64, C.POINTER(Params), vp]),
    ("bella_hip_align_pairs_exact", C.c_int, [vp, C.POINTER(Params), C.POINTER(C.c_uint64)]),
    ("bella_hip_xdrop_batch_exact", C.c_int, [vp, vp, C.c_uint64, C.POINTER(Params), vp]),
    ("bella_hip_write_output", C.c_int, [C.c_char_p, C.POINTER(Params), C.c_int, C.c_uint32, vp, vp, vp, vp, C.c_uint64, C.c_int,
                                         C.POINTER(WriteStats)]),
    ("bella_hip_trace_pairs", C.c_int, [vp, C.POINTER(Params), C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("bella_hip_get_traces", C.c_int, [vp, vp, vp]),
    ("bella_hip_trace_batch", C.c_int, [vp, vp, vp, C.c_uint64, C.POINTER(Params), C.c_uint32, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("bella_hip_get_batch_ops", C.c_int, [vp, vp, C.c_uint64]),
    ("bella_hip_get_trace_stats", C.c_int, [vp, vp, C.c_uint64]),
    ("bella_hip_write_output_traced", C.c_int, [C.c_char_p, C.POINTER(Params), C.c_uint32, vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_int,
                                                C.POINTER(WriteStats)]),
    ("bella_hip_pileup_reset", C.c_int, [vp]),
    ("bella_hip_trace_pairs_pileup", C.c_int, [vp, C.POINTER(Params), C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("bella_hip_get_vote_stats", C.c_int, [vp, vp, C.c_uint64]),
    ("bella_hip_trace_pairs_clip", C.c_int, [vp, C.POINTER(Params), C.c_uint32, C.c_uint32, C.POINTER(ClipParams), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("bella_hip_clip_ops", C.c_int, [vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(ClipParams), vp]),
    ("bella_hip_get_clip_stats", C.c_int, [vp, vp, C.c_uint64]),
    ("bella_hip_pileup_vote", C.c_int, [vp, vp, C.c_uint64, vp, C.c_uint64, C.c_uint32]),
    ("bella_hip_get_pileup", C.c_int, [vp, C.c_uint32, C.c_uint32, vp]),
    ("bella_hip_add_pileup", C.c_int, [vp, C.c_uint32, C.c_uint32, vp]),
    ("bella_hip_get_pileup_bytes", C.c_int, [vp, C.POINTER(C.c_uint64)]),
    ("bella_hip_consensus", C.c_int, [vp, C.POINTER(ConsensusParams), C.POINTER(C.c_uint64)]),
    ("bella_hip_get_consensus", C.c_int, [vp, vp, vp, vp]),
    ("bella_hip_write_fasta", C.c_int, [C.c_char_p, C.c_uint32, vp, vp, vp, C.c_int]),
    ("bella_hip_graph_reset", C.c_int, [vp]),
    ("bella_hip_graph_add_overlaps", C.c_int, [vp, vp, C.c_uint64]),
    ("bella_hip_graph_add_traced", C.c_int, [vp, C.POINTER(C.c_uint64)]),
    ("bella_hip_graph_get_overlaps", C.c_int, [vp, vp, C.POINTER(C.c_uint64)]),
    ("bella_hip_graph_build", C.c_int, [vp, C.POINTER(GraphParams)]),
    ("bella_hip_graph_get", C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), vp, vp, vp]),
    ("bella_hip_graph_get_stats", C.c_int, [vp, vp, C.c_uint64]),
    ("bella_hip_trace_pairs_flags", C.c_int, [vp, C.POINTER(Params), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("bella_hip_get_read_bases", C.c_int, [vp, vp, vp]),
    ("bella_hip_write_gfa", C.c_int, [C.c_char_p, C.c_uint32, vp, vp, vp, vp, vp, vp, vp]),
    ("bella_hip_graph_clean", C.c_int, [vp, C.POINTER(GraphCleanParams)]),
    ("bella_hip_graph_get_removed", C.c_int, [vp, vp]),
    ("bella_hip_graph_unitigs", C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("bella_hip_graph_get_unitigs", C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp]),
    ("bella_hip_graph_get_unitig_bases", C.c_int, [vp, vp, vp]),
    ("bella_hip_graph_get_unitig_stats", C.c_int, [vp, vp, C.c_uint64]),
    ("bella_hip_graph_pop_bubbles", C.c_int, [vp, C.POINTER(GraphBubbleParams)]),
    ("bella_hip_graph_get_bubble_stats", C.c_int, [vp, vp, C.c_uint64]),
    ("bella_hip_graph_cut_weak", C.c_int, [vp, C.POINTER(GraphWeakParams)]),
    ("bella_hip_graph_get_weak_stats", C.c_int, [vp, vp, C.c_uint64]),
    ("bella_hip_graph_polish_unitigs", C.c_int, [vp, C.POINTER(PolishParams), C.POINTER(C.c_uint64)]),
    ("bella_hip_graph_get_polished", C.c_int, [vp, vp, vp, vp, vp, vp]),
    ("bella_hip_graph_get_polish_stats", C.c_int, [vp, vp, C.c_uint64]),
    ("bella_hip_graph_realign_unitigs", C.c_int, [vp, C.POINTER(RealignParams), C.POINTER(C.c_uint64)]),
    ("bella_hip_graph_realign_unitigs_circular", C.c_int, [vp, C.POINTER(RealignParams), C.POINTER(C.c_uint64)]),
    ("bella_hip_graph_get_realign_wrapped", C.c_int, [vp, C.POINTER(C.c_uint64)]),
    ("bella_hip_graph_get_realigned", C.c_int, [vp, vp, vp, vp, vp, vp]),
    ("bella_hip_graph_get_realign_placements", C.c_int, [vp, vp]),
    ("bella_hip_graph_get_realign_ops", C.c_int, [vp, C.POINTER(C.c_uint64), vp, vp]),
    ("bella_hip_graph_get_realign_stats", C.c_int, [vp, vp, C.c_uint64]),
    ("bella_hip_graph_align_links", C.c_int, [vp, C.POINTER(LinkParams), C.POINTER(C.c_uint64)]),
    ("bella_hip_graph_get_link_alignments", C.c_int, [vp, vp, C.POINTER(C.c_uint64), vp]),
    ("bella_hip_graph_get_link_stats", C.c_int, [vp, vp, C.c_uint64]),
    ("bella_hip_write_unitig_gfa_links", C.c_int, [C.c_char_p, C.c_uint32, vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, vp, vp, vp]),
    ("bella_hip_align_sequences", C.c_int, [vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(AlignParams), vp, C.POINTER(C.c_uint64)]),
    ("bella_hip_align_sequences_affine", C.c_int, [vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(AlignParams), C.POINTER(AlignScoring), vp, C.POINTER(C.c_uint64)]),
    ("bella_hip_get_align_ops", C.c_int, [vp, vp, C.c_uint64]),
    ("bella_hip_get_align_stats", C.c_int, [vp, vp, C.c_uint64]),
    ("bella_hip_recorrect", C.c_int, [vp, C.POINTER(RecorrectParams), C.POINTER(C.c_uint64)]),
    ("bella_hip_get_recorrected", C.c_int, [vp, vp, vp, vp]),
    ("bella_hip_get_recorrect_jobs", C.c_int, [vp, C.POINTER(C.c_uint64), vp]),
    ("bella_hip_get_recorrect_ops", C.c_int, [vp, C.POINTER(C.c_uint64), vp, vp]),
    ("bella_hip_get_recorrect_stats", C.c_int, [vp, vp, C.c_uint64]),
    ("bella_hip_get_recorrect_anchors", C.c_int, [vp, vp, vp]),
    ("bella_hip_graph_trim", C.c_int, [vp, C.POINTER(GraphTrimParams)]),
    ("bella_hip_graph_get_trim", C.c_int, [vp, vp]),
    ("bella_hip_graph_get_trim_stats", C.c_int, [vp, vp, C.c_uint64]),
    ("bella_hip_graph_untrim", C.c_int, [vp]),
    ("bella_hip_write_unitig_gfa", C.c_int, [C.c_char_p, C.c_uint32, vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, vp]),
    ("bella_hip_get_timings", C.c_int, [vp, C.POINTER(Timings)]),
    ("bella_hip_get_memory", C.c_int, [vp, C.POINTER(Memory)]),
    ("bella_hip_get_memory_sized", C.c_int, [vp, vp, C.c_uint64]),
    ("bella_hip_set_debug", C.c_int, [vp, C.c_uint32]),
    ("bella_hip_reserve", C.c_int, [vp, C.c_uint64, C.POINTER(C.c_double)]),
    ("bella_hip_trim", C.c_int, [vp]),
    ("bella_hip_set_tuning", C.c_int, [vp, C.c_uint32, vp, C.c_uint32]),
]

_lib = None


def load():
    """Loads the HIP library; raises (never falls back) if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIBPATH):
            raise RuntimeError("libbella_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        lib = C.CDLL(LIBPATH)
        for name, res, args in SIGNATURES:
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib
