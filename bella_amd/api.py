"""Host-side mirror of the reference's call surface for the overlap hot path, over the C ABI.

`Engine` wraps one `bella_ctx` (one GPU).  `hash_spgemm(...)` is shaped like the reference's
`HashSpGEMM(A, B, multop, addop, reads, getvaluetype, filename, bpars, ratiophi)`
(include/overlap.hpp:650-652): operands + reads + BELLApars in, results delivered as the output file in
BELLA / PAF format and the stdout protocol numbers."""
from __future__ import annotations

import ctypes as C
import os
import dataclasses
import sys

import numpy as np

from . import _lib
from ._lib import CLIP_DT, GraphTrimParams, TrimStats
from ._lib import ALIGN_PAIR_DT, ALIGN_RES_DT, AlignParams, AlignScoring, AlignStats
from ._lib import ALN_DT, CONS_DT, EDGE_DT, EXT_DT, LINK_ALN_DT, LINK_DT, LinkParams, LinkStats, OVL_DT, PAIR_DT, PLACE_DT, POLISH_DT, PolishParams, PolishStats, RealignParams, RealignStats, BubbleStats, GraphBubbleParams, GraphCleanParams, GraphWeakParams, WeakStats, GraphParams, GraphStats, UnitigStats, PILEUP_COUNTERS, SEED_DT, TRACE_DT, ConsensusParams, Memory, Params, Timings, TraceStats, WriteStats


class BellaHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("bella_hip error %d: %s" % (code, msg))
        self.code = code


@dataclasses.dataclass
class BellaPars:
    """BELLApars (include/common/common.h:46-74): the fields of the hot path, reference defaults."""
    kmerSize: int = 17
    binSize: int = 500
    xDrop: int = 7
    skipAlignment: bool = False
    outputPaf: bool = False
    errorRate: float = 0.15
    deltaChernoff: float = 0.10

    def c(self) -> Params:
        return Params(self.kmerSize, self.binSize, self.xDrop, int(self.skipAlignment), self.errorRate, self.deltaChernoff)


def _p(a):
    return a.ctypes.data if a is not None and a.size else None


def _over(defaults, params, what):
    """`params` over a copy of `defaults`, as ints"""
    p = dict(defaults)
    for k, v in params.items():
        if k not in p:
            raise TypeError("unknown %s parameter %r" % (what, k))
        p[k] = int(v)
    return p


def _names(names):
    """(how many, char*[] of the encoded names for the C ABI: it keeps the strings alive)"""
    enc = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    return len(enc), C.cast((C.c_char_p * max(len(enc), 1))(*enc), C.c_void_p)


_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


class Engine:
    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        h = C.c_void_p()
        rc = self.lib.bella_hip_init(device, C.byref(h))
        if rc:
            raise BellaHipError(rc, self.lib.bella_hip_strerror(rc).decode() + " (bella_hip_init; no CPU fallback exists)")
        self.h = h
        self.nreads = 0
        self.lengths = None
        self.names = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.bella_hip_destroy(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc):
        if rc:
            raise BellaHipError(rc, self.lib.bella_hip_last_error(self.h).decode() or self.lib.bella_hip_strerror(rc).decode())

    def _stats(self, getter, struct) -> dict:
        """one of the ABI's sized result structs as a dict of its fields"""
        st = struct()
        self._chk(getter(self.h, C.byref(st), C.sizeof(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    # ---- reads (readVector_) ----
    def set_reads(self, rs):
        asc = np.ascontiguousarray(_ACGT[rs.codes])       # the C ABI takes ASCII bases, as the reference's readVector_ holds them
        offs = np.ascontiguousarray(rs.offsets, dtype=np.uint64)
        self._chk(self.lib.bella_hip_set_reads(self.h, _p(asc), offs.ctypes.data, rs.nreads))
        self.nreads = rs.nreads
        self.lengths = rs.lengths
        self.names = rs.names

    def load_fastq(self, path):
        """ParallelFASTQ + get_fq_name (kmercode/fq_reader.c) + 2-bit packing: the file goes straight into the library.
        `path` may be a list of files (the reference's -f list, kmercount.hpp:82-105): read ids continue from file to file."""
        n, nb = C.c_uint32(0), C.c_uint64(0)
        if isinstance(path, (list, tuple)):
            arr = (C.c_char_p * max(len(path), 1))(*[os.fsencode(x) for x in path])
            self._chk(self.lib.bella_hip_load_fastq_list(self.h, arr, len(path), C.byref(n), C.byref(nb)))
        else:
            self._chk(self.lib.bella_hip_load_fastq(self.h, os.fsencode(path), C.byref(n), C.byref(nb)))
        self.nreads = n.value
        need = C.c_uint64(0)
        self._chk(self.lib.bella_hip_get_read_names(self.h, None, 0, None, C.byref(need)))
        buf = C.create_string_buffer(max(need.value, 1))
        offs = np.zeros(self.nreads + 1, np.uint64)
        self._chk(self.lib.bella_hip_get_read_names(self.h, buf, need.value, offs.ctypes.data, None))
        raw = buf.raw
        self.names = [raw[int(offs[i]):int(offs[i + 1]) - 1].decode() for i in range(self.nreads)]
        lens = np.zeros(max(self.nreads, 1), np.uint32)
        self._chk(self.lib.bella_hip_get_read_lengths(self.h, lens.ctypes.data))
        self.lengths = lens[:self.nreads]
        return self.nreads, nb.value

    def ingest_stats(self):
        """what the last load_fastq did: file bytes, bases, reads, host threads, index_ms, upload_ms"""
        st = _lib.IngestStats()
        self._chk(self.lib.bella_hip_get_ingest_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def set_reads_raw(self, ascii_bases: np.ndarray, offsets: np.ndarray, names=None):
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        asc = np.ascontiguousarray(ascii_bases, dtype=np.uint8)
        self._chk(self.lib.bella_hip_set_reads(self.h, _p(asc), offs.ctypes.data, len(offs) - 1))
        self.nreads = len(offs) - 1
        self.lengths = np.diff(offs).astype(np.uint32)
        self.names = names

    # ---- SplitCount + tuple generation (kmercount.hpp:467-677, main.cpp:393-416) ----
    def count_kmers(self, k=17, lower=2, upper=8, syncmer=False, window=0):
        """reliable dictionary and tuples of the reads on the device (syncmer=True: the reference's -s mode);
        returns (nkmers, ntuples, ndistinct)"""
        nk, nt, nd = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        if window and not syncmer:                      # main.cpp:165-171: -w selects minimizers unless -s is given
            self._chk(self.lib.bella_hip_count_minimizers(self.h, k, window, lower, upper, C.byref(nk), C.byref(nt), C.byref(nd)))
        else:
            fn = self.lib.bella_hip_count_syncmers if syncmer else self.lib.bella_hip_count_kmers
            self._chk(fn(self.h, k, lower, upper, C.byref(nk), C.byref(nt), C.byref(nd)))
        self.nkmers_counted, self.ntuples_counted = nk.value, nt.value
        return nk.value, nt.value, nd.value

    def get_dictionary(self):
        codes = np.zeros(max(self.nkmers_counted, 1), np.uint64)
        counts = np.zeros(max(self.nkmers_counted, 1), np.uint16)
        self._chk(self.lib.bella_hip_get_dictionary(self.h, codes.ctypes.data, counts.ctypes.data))
        return codes[:self.nkmers_counted], counts[:self.nkmers_counted]

    def get_tuples(self):
        n = self.ntuples_counted
        tk, tr, tp = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint16)
        self._chk(self.lib.bella_hip_get_tuples(self.h, tk.ctypes.data, tr.ctypes.data, tp.ctypes.data))
        return tk[:n], tr[:n], tp[:n]

    def count_stats(self):
        """what the host decided for the last count: dict(fast, pb, gb, slots, mode, positions, budget,
        passes=[(first bin, end bin, words, tiles)])"""
        n = C.c_uint32(0)
        self._chk(self.lib.bella_hip_get_count_stats(self.h, None, 0, C.byref(n)))
        v = np.zeros(max(n.value, 1), np.uint64)
        self._chk(self.lib.bella_hip_get_count_stats(self.h, v.ctypes.data, n.value, C.byref(n)))
        v = [int(x) for x in v[:n.value]]
        assert len(v) == 8 + 4 * v[3], v
        return dict(fast=bool(v[0]), pb=v[1], gb=v[2], slots=v[4], mode=v[5], positions=v[6], budget=v[7],
                    passes=[tuple(v[8 + 4 * p:12 + 4 * p]) for p in range(v[3])])

    def assemble_counted(self):
        self._chk(self.lib.bella_hip_assemble_counted(self.h))

    def assemble_counted_panel(self, first_read, nreads_panel):
        self._chk(self.lib.bella_hip_assemble_counted_panel(self.h, first_read, nreads_panel))

    # ---- operands ----
    def assemble_tuples(self, k, nkmers, tk, tr, tp):
        tk = np.ascontiguousarray(tk, np.uint32); tr = np.ascontiguousarray(tr, np.uint32); tp = np.ascontiguousarray(tp, np.uint16)
        self._chk(self.lib.bella_hip_assemble_tuples(self.h, k, nkmers, len(tk), _p(tk), _p(tr), _p(tp)))

    def set_B(self, k, nkmers, colptr, rowids, values):
        colptr = np.ascontiguousarray(colptr, np.uint32); rowids = np.ascontiguousarray(rowids, np.uint32)
        values = np.ascontiguousarray(values, np.uint16)
        self._chk(self.lib.bella_hip_set_B(self.h, k, nkmers, colptr.ctypes.data, _p(rowids), _p(values)))

    # ---- multi-GPU assembly: row-block panels ----
    def set_B_panel(self, k, nkmers, first_read, nreads_panel, colptr, rowids, values):
        """bella_hip_set_B_panel: this context's row block of the reference's CSC of B (whole arrays given, the slice is uploaded)"""
        colptr = np.ascontiguousarray(colptr, np.uint32); rowids = np.ascontiguousarray(rowids, np.uint32); values = np.ascontiguousarray(values, np.uint16)
        self._chk(self.lib.bella_hip_set_B_panel(self.h, k, nkmers, first_read, nreads_panel, _p(colptr), _p(rowids), _p(values)))

    def assemble_panel(self, k, nkmers, first_read, nreads_panel, tk, tr, tp):
        tk = np.ascontiguousarray(tk, np.uint32); tr = np.ascontiguousarray(tr, np.uint32); tp = np.ascontiguousarray(tp, np.uint16)
        self._chk(self.lib.bella_hip_assemble_panel(self.h, k, nkmers, first_read, nreads_panel, len(tk), _p(tk), _p(tr), _p(tp)))

    def panel_tensors(self, device_index=0):
        """(rowcnt int32[rows], rowids int32[nnz], values int16[nnz]) torch tensors ALIASING the library's device buffers
        (valid until the next assembly call) -- what goes into the all-gather."""
        import torch
        first, rows, nnz = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        pc, pr, pv = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk(self.lib.bella_hip_panel_device_ptrs(self.h, C.byref(first), C.byref(rows), C.byref(nnz), C.byref(pc), C.byref(pr),
                                                       C.byref(pv)))

        class _Alias:
            def __init__(self, ptr, n, typestr):
                self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}

        dev = torch.device("cuda", device_index)

        def t(ptr, n, typestr, dt):
            return torch.as_tensor(_Alias(ptr, n, typestr), device=dev) if n else torch.zeros(0, dtype=dt, device=dev)
        return (t(pc.value, rows.value, "<i4", torch.int32), t(pr.value, nnz.value, "<i4", torch.int32),
                t(pv.value, nnz.value, "<i2", torch.int16))

    # ---- multi-GPU: the library's own RCCL communicator (include/bella_hip.h) ----
    def comm_available(self) -> bool:
        """librccl can be loaded in this process (check on every rank BEFORE the collective comm_init)"""
        return bool(self.lib.bella_hip_comm_available())

    def comm_id(self, local: bool = False) -> bytes:
        """the 128-byte id rank 0 hands to every rank; local=True: the in-process transport (contexts of one process)"""
        buf = C.create_string_buffer(128)
        rc = (self.lib.bella_hip_comm_id_local if local else self.lib.bella_hip_comm_id)(buf)
        if rc:
            raise BellaHipError(rc, "librccl could not be loaded")
        return buf.raw

    def comm_init(self, nranks: int, rank: int, comm_id: bytes, local: bool = False):
        buf = C.create_string_buffer(bytes(comm_id), 128)
        self._chk((self.lib.bella_hip_comm_init_local if local else self.lib.bella_hip_comm_init)(self.h, nranks, rank, buf))

    def comm_destroy(self):
        self._chk(self.lib.bella_hip_comm_destroy(self.h))

    def count_kmers_dist(self, first_read, nreads_block, k=17, lower=2, upper=8, syncmer=False, window=0):
        """collective (needs comm_init): the dictionary is counted across the ranks, tuples only for this rank's read block"""
        nk, nt, nd = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        sel = 1 if syncmer else (2 if window else 0)
        self._chk(self.lib.bella_hip_count_kmers_dist(self.h, k, lower, upper, sel, window, first_read, nreads_block, C.byref(nk), C.byref(nt),
                                                      C.byref(nd)))
        self.nkmers_counted, self.ntuples_counted = nk.value, nt.value
        return nk.value, nt.value, nd.value

    def allgather_panels(self):
        """collective: every rank's row block of B -> the whole matrix on every rank, device layout built"""
        self._chk(self.lib.bella_hip_allgather_panels(self.h))

    def set_B_device(self, k, nkmers, colptr_t, rowids_t, values_t):
        """full B from torch device tensors (int32 colptr[nreads+1], int32 rowids, int16 values)"""
        nnz = int(rowids_t.numel())
        self._chk(self.lib.bella_hip_set_B_device(self.h, k, nkmers, colptr_t.data_ptr(), rowids_t.data_ptr() if nnz else None,
                                                  values_t.data_ptr() if nnz else None, nnz))

    def get_B(self):
        nnz = C.c_uint64(0)
        self._chk(self.lib.bella_hip_get_B(self.h, C.byref(nnz), None, None, None))
        colptr = np.zeros(self.nreads + 1, np.uint32)
        rowids = np.zeros(max(nnz.value, 1), np.uint32)
        values = np.zeros(max(nnz.value, 1), np.uint16)
        self._chk(self.lib.bella_hip_get_B(self.h, C.byref(nnz), colptr.ctypes.data, rowids.ctypes.data, values.ctypes.data))
        return colptr, rowids[:nnz.value], values[:nnz.value]

    def assemble_stats(self):
        """which path the last assembly took: dict(classes=(reads per table class of the row assembly), inline, products,
        first_appearance, place_sorted)"""
        n = C.c_uint32(0)
        v = np.zeros(16, np.uint64)
        self._chk(self.lib.bella_hip_get_assemble_stats(self.h, v.ctypes.data, len(v), C.byref(n)))
        assert n.value == 9, n.value
        v = [int(x) for x in v[:9]]
        return dict(classes=tuple(v[:5]), inline=bool(v[5]), products=bool(v[6]), first_appearance=bool(v[7]), place_sorted=bool(v[8]))

    def set_partition(self, first, stride):
        self._chk(self.lib.bella_hip_set_partition(self.h, first, stride))

    def set_column_range(self, first, count):
        self._chk(self.lib.bella_hip_set_column_range(self.h, first, count))

    def set_debug(self, flags):
        self._chk(self.lib.bella_hip_set_debug(self.h, flags))

    # ---- HashSpGEMM ----
    TUNE = {"lds_tiers": 0, "kcount_budget": 1, "wide_budget": 2, "xdrop_variant": 3, "row_lists": 4, "xdrop_class_min": 5,
            "layout_order": 6, "inline_entries": 7, "row_path": 8, "cache_bytes": 9, "dist_layout": 10, "compact_b": 11, "product_entries": 12,
            "order_split": 13, "round_budget": 14, "xdrop_batch": 15}

    def reserve(self, nbytes: int) -> float:
        """bella_hip_reserve: one slab of device memory up front (the stages then allocate nothing from the driver); returns the ms it took"""
        ms = C.c_double(0.0)
        self._chk(self.lib.bella_hip_reserve(self.h, int(nbytes), C.byref(ms)))
        return ms.value

    def trim(self):
        """bella_hip_trim: released buffers the context keeps for reuse go back to the driver"""
        self._chk(self.lib.bella_hip_trim(self.h))

    def set_tuning(self, what: str, *values):
        """bella_hip_set_tuning: per-context tuning parameters (tests, A/B measurements); no values = the default"""
        v = np.asarray(values, dtype=np.uint64)
        self._chk(self.lib.bella_hip_set_tuning(self.h, self.TUNE[what], v.ctypes.data if len(v) else None, len(v)))

    def overlap(self, pars: BellaPars):
        n, f = C.c_uint64(0), C.c_uint64(0)
        cp = pars.c()
        self._chk(self.lib.bella_hip_overlap(self.h, C.byref(cp), C.byref(n), C.byref(f)))
        self.npairs, self.flops = n.value, f.value
        return n.value, f.value

    def count_pairs(self, pars: BellaPars):
        """bella_hip_count_pairs: the symbolic phase alone (estimateFLOP + estimateNNZ_Hash + prefixsum) -> colptrC, nnz(C), products"""
        n, f = C.c_uint64(0), C.c_uint64(0)
        cp = pars.c()
        colptrC = np.zeros(self.nreads + 1, np.uint64)
        self._chk(self.lib.bella_hip_count_pairs(self.h, C.byref(cp), colptrC.ctypes.data, C.byref(n), C.byref(f)))
        return colptrC, n.value, f.value

    def count_flops(self, pars: BellaPars):
        """estimateFLOP alone (bella_hip_count_pairs without the pair outputs): the products of the context's columns"""
        f = C.c_uint64(0)
        cp = pars.c()
        self._chk(self.lib.bella_hip_count_pairs(self.h, C.byref(cp), None, None, C.byref(f)))
        return f.value

    def get_pairs(self, ext=True):
        pairs = np.zeros(self.npairs, PAIR_DT)
        ex = np.zeros(self.npairs, EXT_DT) if ext else None
        colptrC = np.zeros(self.nreads + 1, np.uint64)
        self._chk(self.lib.bella_hip_get_pairs(self.h, _p(pairs), _p(ex) if ext else None, colptrC.ctypes.data))
        return pairs, ex, colptrC

    # ---- RunPairWiseAlignments ----
    def align_pairs(self, pars: BellaPars, exact: bool = False):
        """exact=True: the growing-band gapped X-drop of the reference's CUDA build (LOGAN / SeqAn extendSeed) instead of Xavier"""
        n = C.c_uint64(0)
        cp = pars.c()
        fn = self.lib.bella_hip_align_pairs_exact if exact else self.lib.bella_hip_align_pairs
        self._chk(fn(self.h, C.byref(cp), C.byref(n)))
        return n.value

    def get_alignments(self):
        out = np.zeros(self.npairs, ALN_DT)
        if self.npairs:
            self._chk(self.lib.bella_hip_get_alignments(self.h, out.ctypes.data))
        return out

    def xdrop_batch(self, seeds: np.ndarray, pars: BellaPars, exact: bool = False):
        seeds = np.ascontiguousarray(seeds, SEED_DT)
        out = np.zeros(len(seeds), ALN_DT)
        cp = pars.c()
        fn = self.lib.bella_hip_xdrop_batch_exact if exact else self.lib.bella_hip_xdrop_batch
        self._chk(fn(self.h, _p(seeds), len(seeds), C.byref(cp), _p(out)))
        return out

    # ---- traced alignments (base-level: run-length ops, len << 4 | op, op 0 '=' 1 'X' 2 'I' 3 'D') ----
    def trace_pairs(self, pars: BellaPars, band0: int = 0, passed_only: bool = True, pileup: bool = False, keep_ops: bool = True, normalize: bool = False,
                    clip: int = None):
        """Traces the pairs of the last align_pairs.  Returns (traces[npairs] of TRACE_DT, untraced: nops == 0; ops uint32).
        pileup=True (needs pileup_reset, passed pairs only): every traced pair also votes into the pileup table on the device; with
        keep_ops=False the runs never reach the host and `ops` comes back empty (the records are the same).  normalize=True (with
        pileup): every gap run votes at its canonical position; records and runs are the same.  clip=<identity in permille> (DESIGN.md
        section 24): every traced alignment is cut to its maximum-scoring segment at that identity on the device before anything reads
        it; the records are the clipped ones (an emptied pair: nops == 0), `ops` is the array of the call without it."""
        nt, no = C.c_uint64(0), C.c_uint64(0)
        cp = pars.c()
        if normalize and not pileup:
            raise ValueError("normalize=True normalises the votes: it needs pileup=True")
        if pileup and not passed_only:
            raise ValueError("pileup=True traces the passed pairs only")
        if clip is not None:
            flags = (_lib.TRACE_PASSED_ONLY if passed_only else 0) | (_lib.TRACE_PILEUP if pileup else 0) | (_lib.TRACE_NORMALIZE if normalize else 0) \
                | (_lib.TRACE_DROP_OPS if pileup and not keep_ops else 0)
            kp = _lib.ClipParams(C.sizeof(_lib.ClipParams), int(clip))
            self._chk(self.lib.bella_hip_trace_pairs_clip(self.h, C.byref(cp), band0, flags, C.byref(kp), C.byref(nt), C.byref(no)))
        elif pileup:
            if normalize:
                flags = _lib.TRACE_PASSED_ONLY | _lib.TRACE_PILEUP | _lib.TRACE_NORMALIZE | (0 if keep_ops else _lib.TRACE_DROP_OPS)
                self._chk(self.lib.bella_hip_trace_pairs_flags(self.h, C.byref(cp), band0, flags, C.byref(nt), C.byref(no)))
            else:
                self._chk(    self.lib.bella_hip_trace_pairs_pileup(self.h, C.byref(cp), band0, 1 if keep_ops else 0, C.byref(nt), C.byref(no)))
        else:
            self._chk(self.lib.bella_hip_trace_pairs(self.h, C.byref(cp), band0, 1 if passed_only else 0, C.byref(nt), C.byref(no)))
        tr = np.zeros(self.npairs, TRACE_DT)
        ops = np.zeros(no.value if (keep_ops or not pileup) else 0, np.uint32)
        self._chk(self.lib.bella_hip_get_traces(self.h, _p(tr), _p(ops)))
        return tr, ops

    # ---- read correction: pileup of the traced alignments, consensus ----
    def pileup_reset(self):
        """allocates (first use) and zeroes the pileup table of the loaded reads: 9 uint32 per base"""
        self._chk(self.lib.bella_hip_pileup_reset(self.h))

    def pileup_vote(self, pairs: np.ndarray, ops: np.ndarray, normalize: bool = False):
        """votes caller-supplied traced pairs (VOTE_PAIR_DT; runs len << 4 | op in `ops`) into the table; normalize=True: with every gap
        run at its canonical position.  Everything is validated before anything is voted."""
        pr = np.ascontiguousarray(pairs, _lib.VOTE_PAIR_DT)
        op = np.ascontiguousarray(ops, np.uint32)
        self._chk(self.lib.bella_hip_pileup_vote(self.h, _p(pr), len(pr), _p(op), len(op), _lib.TRACE_NORMALIZE if normalize else 0))

    def vote_stats(self) -> dict:
        """what the last voting call did: the fields of bella_vote_stats"""
        return self._stats(self.lib.bella_hip_get_vote_stats, _lib.VoteStats)

    # ---- clipped ends ----
    def clip_ops(self, pairs: np.ndarray, ops: np.ndarray, identity: int = 650) -> np.ndarray:
        """the clip of caller-supplied traced pairs (VOTE_PAIR_DT, of which op_off, nops, tbegV and tbegH are read; runs len << 4 | op in
        `ops`): CLIP_RES_DT[len(pairs)].  Everything is validated before anything is launched; no reads need to be loaded."""
        pr = np.ascontiguousarray(pairs, _lib.VOTE_PAIR_DT)
        op = np.ascontiguousarray(ops, np.uint32)
        out = np.zeros(len(pr), _lib.CLIP_RES_DT)
        kp = _lib.ClipParams(C.sizeof(_lib.ClipParams), int(identity))
        self._chk(self.lib.bella_hip_clip_ops(self.h, _p(pr), len(pr), _p(op), len(op), C.byref(kp), _p(out)))
        return out

    def clip_stats(self) -> dict:
        """what the last clipping call (trace_pairs / trace_pairs_records with clip=, clip_ops) did: the fields of bella_clip_stats"""
        return self._stats(self.lib.bella_hip_get_clip_stats, _lib.ClipStats)

    def _range_bases(self, first, n):
        if first < 0 or n < 0 or first + n > self.nreads:
            raise ValueError("reads [%d, %d) out of range" % (first, first + n))
        return int(np.asarray(self.lengths[first:first + n], np.int64).sum())

    def get_pileup(self, first: int = 0, n: int = None) -> np.ndarray:
        """(bases of the reads [first, first + n), 9) uint32: votes for A C G T, del, inserted A C G T before the base"""
        n = self.nreads - first if n is None else n
        out = np.zeros((self._range_bases(first, n), PILEUP_COUNTERS), np.uint32)
        self._chk(self.lib.bella_hip_get_pileup(self.h, first, n, _p(out)))
        return out

    def add_pileup(self, first: int, n: int, counters: np.ndarray):
        """adds a (bases, 9) uint32 array (another context's get_pileup of the same reads) into the table"""
        a = np.ascontiguousarray(counters, np.uint32)
        if a.shape != (self._range_bases(first, n), PILEUP_COUNTERS):
            raise ValueError("counters must have shape (bases of the reads, 9)")
        self._chk(self.lib.bella_hip_add_pileup(self.h, first, n, _p(a)))

    def pileup_bytes(self) -> int:
        b = C.c_uint64(0)
        self._chk(self.lib.bella_hip_get_pileup_bytes(self.h, C.byref(b)))
        return b.value

    def consensus(self, min_depth: int = 3):
        """majority-vote consensus of every read from the table: (offsets uint64[nreads + 1], bases uint8 ASCII, stats of CONS_DT)"""
        cp = ConsensusParams(C.sizeof(ConsensusParams), min_depth)
        tot = C.c_uint64(0)
        self._chk(self.lib.bella_hip_consensus(self.h, C.byref(cp), C.byref(tot)))
        offs = np.zeros(self.nreads + 1, np.uint64)
        bases = np.zeros(tot.value, np.uint8)
        stats = np.zeros(self.nreads, CONS_DT)
        self._chk(self.lib.bella_hip_get_consensus(self.h, offs.ctypes.data, _p(bases), _p(stats)))
        return offs, bases, stats

    # ---- read correction rounds ----
    RECORRECT_DEFAULTS = dict(band0=512, band_max=4096, min_identity=700, min_depth=3, keep_ops=0)

    def recorrect(self, **params):
        """one correction round on the device: for every accumulated overlap record each read's raw clip is aligned against the newest
        corrected sequence of the other read (consensus()'s, or the last round's), the votes decide every corrected read again:
        (offsets uint64[nreads + 1], bases uint8 ASCII, stats of CONS_DT relative to the round's input)"""
        p = _over(self.RECORRECT_DEFAULTS, params, "recorrect")
        rp = _lib.RecorrectParams(C.sizeof(_lib.RecorrectParams), *(p[k] for k in ("band0", "band_max", "min_identity", "min_depth", "keep_ops")))
        tot = C.c_uint64(0)
        self._chk(self.lib.bella_hip_recorrect(self.h, C.byref(rp), C.byref(tot)))
        return self.recorrected()

    def recorrected(self):
        st = self.recorrect_stats()
        offs, bases, stats = np.zeros(self.nreads + 1, np.uint64), np.zeros(st["bases_after"], np.uint8), np.zeros(self.nreads, CONS_DT)
        self._chk(self.lib.bella_hip_get_recorrected(self.h, offs.ctypes.data, _p(bases), _p(stats)))
        return offs, bases, stats

    def recorrect_jobs(self) -> np.ndarray:
        """two records of RECJOB_DT per overlap record of the last round: job 2 x targets V, job 2 x + 1 targets H"""
        n = C.c_uint64(0)
        self._chk(self.lib.bella_hip_get_recorrect_jobs(self.h, C.byref(n), None))
        out = np.zeros(n.value, _lib.RECJOB_DT)
        self._chk(self.lib.bella_hip_get_recorrect_jobs(self.h, C.byref(n), _p(out)))
        return out

    def recorrect_ops(self):
        """tests: (runs, table) of a round that ran with keep_ops -- the voters' runs (a job's op_off / nops index them) and the round's
        counters, (bases_before, 9) uint32"""
        n = C.c_uint64(0)
        self._chk(self.lib.bella_hip_get_recorrect_ops(self.h, C.byref(n), None, None))
        ops, table = np.zeros(n.value, np.uint32), np.zeros((self.recorrect_stats()["bases_before"], PILEUP_COUNTERS), np.uint32)
        self._chk(self.lib.bella_hip_get_recorrect_ops(self.h, C.byref(n), _p(ops), _p(table)))
        return ops, table

    def recorrect_stats(self) -> dict:
        return self._stats(self.lib.bella_hip_get_recorrect_stats, _lib.RecorrectStats)

    def recorrect_anchors(self):
        """tests: (offsets uint64[nreads + 1], anchors uint64) of the newest corrected sequences: where every 256th raw base of a read lies"""
        offs = np.zeros(self.nreads + 1, np.uint64)
        self._chk(self.lib.bella_hip_get_recorrect_anchors(self.h, offs.ctypes.data, None))
        a = np.zeros(int(offs[-1]), np.uint64)
        self._chk(self.lib.bella_hip_get_recorrect_anchors(self.h, None, _p(a)))
        return offs, a

    # ---- string graph: overlap classes, containment, transitive reduction ----
    GRAPH_DEFAULTS = dict(min_overlap=1000, max_overhang=1000, overhang_permille=800, fuzz=1000)

    def trace_pairs_records(self, pars: BellaPars, band0: int = 0, passed_only: bool = True, clip: int = None):
        """bella_hip_trace_pairs_flags with the runs dropped: traces[npairs] of TRACE_DT only -- no run is written or staged (what the
        graph needs: graph_add_traced reads the end points).  clip=<identity in permille>: the clipped records of DESIGN.md section 24
        (the runs are then written on the device, where the clip reads them, and still not staged)."""
        nt, no = C.c_uint64(0), C.c_uint64(0)
        cp = pars.c()
        flags = _lib.TRACE_DROP_OPS | (_lib.TRACE_PASSED_ONLY if passed_only else 0)
        if clip is not None:
            kp = _lib.ClipParams(C.sizeof(_lib.ClipParams), int(clip))
            self._chk(self.lib.bella_hip_trace_pairs_clip(self.h, C.byref(cp), band0, flags, C.byref(kp), C.byref(nt), C.byref(no)))
        else:
            self._chk(self.lib.bella_hip_trace_pairs_flags(self.h, C.byref(cp), band0, flags, C.byref(nt), C.byref(no)))
        tr = np.zeros(self.npairs, TRACE_DT)
        self._chk(self.lib.bella_hip_get_traces(self.h, _p(tr), None))
        return tr

    def graph_reset(self):
        self._chk(self.lib.bella_hip_graph_reset(self.h))

    def graph_add_overlaps(self, recs: np.ndarray):
        """appends explicit overlap records (OVL_DT); they accumulate until graph_reset or other reads"""
        recs = np.ascontiguousarray(recs, OVL_DT)
        self._chk(self.lib.bella_hip_graph_add_overlaps(self.h, _p(recs), len(recs)))

    def graph_add_traced(self) -> int:
        """appends one record per passed, traced pair of the last align_pairs + trace_pairs; returns how many"""
        n = C.c_uint64(0)
        self._chk(self.lib.bella_hip_graph_add_traced(self.h, C.byref(n)))
        return n.value

    def graph_overlaps(self) -> np.ndarray:
        n = C.c_uint64(0)
        self._chk(self.lib.bella_hip_graph_get_overlaps(self.h, None, C.byref(n)))
        out = np.zeros(n.value, OVL_DT)
        self._chk(self.lib.bella_hip_graph_get_overlaps(self.h, _p(out), C.byref(n)))
        return out

    def graph_build(self, **params):
        """classifies the accumulated records, drops contained reads, reduces transitively (on the device); min_overlap, max_overhang,
        overhang_permille, fuzz default to 1000, 1000, 800, 1000"""
        p = _over(self.GRAPH_DEFAULTS, params, "graph")
        gp = GraphParams(C.sizeof(GraphParams), p["min_overlap"], p["max_overhang"], p["overhang_permille"], p["fuzz"])
        self._chk(self.lib.bella_hip_graph_build(self.h, C.byref(gp)))

    def graph(self):
        """(offsets uint64[2 nreads + 1], edges of EDGE_DT in list order, contained uint8[nreads]) of the last graph_build"""
        nv, ne = C.c_uint32(0), C.c_uint64(0)
        self._chk(self.lib.bella_hip_graph_get(self.h, C.byref(nv), C.byref(ne), None, None, None))
        offs = np.zeros(nv.value + 1, np.uint64)
        edges = np.zeros(ne.value, EDGE_DT)
        cont = np.zeros(nv.value // 2, np.uint8)
        self._chk(self.lib.bella_hip_graph_get(self.h, None, None, offs.ctypes.data, _p(edges), _p(cont)))
        return offs, edges, cont

    def graph_stats(self) -> dict:
        return self._stats(self.lib.bella_hip_graph_get_stats, GraphStats)

    # ---- unitigs: tip clipping, compaction, sequences ----
    CLEAN_DEFAULTS = dict(max_tip_reads=4, tip_rounds=3)

    def graph_clean(self, **params):
        """clips tips off the current graph (on the device) and replaces it: graph() then returns the cleaned one.  max_tip_reads
        (0 = off) and tip_rounds default to 4 and 3"""
        p = _over(self.CLEAN_DEFAULTS, params, "clean")
        cp = GraphCleanParams(C.sizeof(GraphCleanParams), p["max_tip_reads"], p["tip_rounds"])
        self._chk(self.lib.bella_hip_graph_clean(self.h, C.byref(cp)))

    def graph_removed(self) -> np.ndarray:
        """uint8[nreads]: the reads graph_clean and graph_pop_bubbles took out since the last graph_build"""
        out = np.zeros(self.nreads, np.uint8)
        self._chk(self.lib.bella_hip_graph_get_removed(self.h, _p(out)))
        return out

    # ---- bubble popping ----
    BUBBLE_DEFAULTS = dict(max_bubble_reads=64, max_bubble_dist=50000, bubble_rounds=3)

    def graph_pop_bubbles(self, **params):
        """pops bubbles of the current graph (on the device) and replaces it, as graph_clean does; the popped reads show in
        graph_removed().  max_bubble_reads (0 = off, at most 255), max_bubble_dist and bubble_rounds default to 64, 50,000 and 3"""
        p = _over(self.BUBBLE_DEFAULTS, params, "bubble")
        bp = GraphBubbleParams(C.sizeof(GraphBubbleParams), p["max_bubble_reads"], p["max_bubble_dist"], p["bubble_rounds"])
        self._chk(self.lib.bella_hip_graph_pop_bubbles(self.h, C.byref(bp)))

    def bubble_stats(self) -> dict:
        """of the last graph_pop_bubbles: totals, and per round sources / found / popped / reads_per_round / edges_per_round"""
        st = self._stats(self.lib.bella_hip_graph_get_bubble_stats, BubbleStats)
        out = {k: st[k] for k in ("reads_removed", "edges_removed", "rounds", "pop_ms")}
        for k in ("sources", "found", "popped", "reads_per_round", "edges_per_round"):
            out[k] = list(st[k])[:st["rounds"]]
        return out

    # ---- weak-overlap removal ----
    WEAK_DEFAULTS = dict(ratio_permille=500)

    def graph_cut_weak(self, **params):
        """removes the weak edges of the current graph (on the device) and replaces it, as graph_clean does: an edge goes when its overlap,
        or its twin's, is below ratio_permille (default 500; 0 = off, at most 1000) thousandths of the best overlap of its source vertex.
        No read is removed"""
        p = _over(self.WEAK_DEFAULTS, params, "weak")
        wp = GraphWeakParams(C.sizeof(GraphWeakParams), p["ratio_permille"])
        self._chk(self.lib.bella_hip_graph_cut_weak(self.h, C.byref(wp)))

    def weak_stats(self) -> dict:
        """of the last graph_cut_weak: forks, weak, edges_removed, ratio_permille, cut_ms"""
        return self._stats(self.lib.bella_hip_graph_get_weak_stats, WeakStats)

    def graph_unitigs(self) -> dict:
        """unitigs of the current graph (on the device): voff uint64[n + 1] into verts uint32 / pos uint64 / nbases uint32, len uint64[n],
        circular uint8[n], links of LINK_DT"""
        n, nv, nl, tb = (C.c_uint64(0) for _ in range(4))
        self._chk(self.lib.bella_hip_graph_unitigs(self.h, C.byref(n), C.byref(nv), C.byref(nl), C.byref(tb)))
        u = dict(voff=np.zeros(n.value + 1, np.uint64), verts=np.zeros(nv.value, np.uint32), pos=np.zeros(nv.value, np.uint64), nbases=np.zeros(nv.value, np.uint32),
                 len=np.zeros(n.value, np.uint64), circular=np.zeros(n.value, np.uint8), links=np.zeros(nl.value, LINK_DT))
        self._chk(self.lib.bella_hip_graph_get_unitigs(self.h, *(_p(u[k]) for k in ("voff", "verts", "pos", "nbases", "len", "circular", "links"))))
        u["total_bases"] = tb.value
        return u

    def unitig_bases(self):
        """(offsets uint64[nunitigs + 1], bases uint8 ASCII) of the last graph_unitigs"""
        st = self.unitig_stats()
        offs = np.zeros(st["unitigs"] + 1, np.uint64)
        bases = np.zeros(st["total_bases"], np.uint8)
        self._chk(self.lib.bella_hip_graph_get_unitig_bases(self.h, offs.ctypes.data, _p(bases)))
        return offs, bases

    def unitig_stats(self) -> dict:
        out = self._stats(self.lib.bella_hip_graph_get_unitig_stats, UnitigStats)
        for k in ("tips_per_round", "reads_per_round"):
            out[k] = list(out[k])[:out["rounds"]]
        return out

    # ---- unitig consensus ----
    def graph_polish_unitigs(self, min_depth: int = 3) -> dict:
        """polishes the unitigs of the last graph_unitigs with the pileup table (on the device): offsets uint64[n + 1] into bases (uint8
        ASCII), pos uint64 / nbases uint32 per vertex in polished coordinates, stats of POLISH_DT per unitig"""
        pp = PolishParams(C.sizeof(PolishParams), min_depth)
        tot = C.c_uint64(0)
        self._chk(self.lib.bella_hip_graph_polish_unitigs(self.h, C.byref(pp), C.byref(tot)))
        st = self.polish_stats()
        out = dict(offsets=np.zeros(st["unitigs"] + 1, np.uint64), bases=np.zeros(tot.value, np.uint8), pos=np.zeros(st["vertices"], np.uint64),
                   nbases=np.zeros(st["vertices"], np.uint32), stats=np.zeros(st["unitigs"], POLISH_DT))
        self._chk(self.lib.bella_hip_graph_get_polished(self.h, *(_p(out[k]) for k in ("offsets", "bases", "pos", "nbases", "stats"))))
        return out

    def polish_stats(self) -> dict:
        return self._stats(self.lib.bella_hip_graph_get_polish_stats, PolishStats)

    # ---- realignment ----
    REALIGN_DEFAULTS = dict(band0=512, band_max=4096, min_identity=700, min_depth=3, keep_ops=0)

    def graph_realign_unitigs(self, circular: bool = False, **params) -> dict:
        """one realignment round against the newest sequence of the unitigs (the polish's, or the last round's), on the device: the
        result in the shape of graph_polish_unitigs -- pos / nbases are where the polish's segments begin in the new sequence.
        circular=True: the reads of circular unitigs are placed on the unrolled circle"""
        rp = RealignParams(C.sizeof(RealignParams), *(_over(self.REALIGN_DEFAULTS, params, "graph_realign_unitigs")[k] for k in ("band0", "band_max", "min_identity", "min_depth", "keep_ops")))
        tot = C.c_uint64(0)
        run = self.lib.bella_hip_graph_realign_unitigs_circular if circular else self.lib.bella_hip_graph_realign_unitigs
        self._chk(run(self.h, C.byref(rp), C.byref(tot)))
        return self.realigned()

    def realigned(self) -> dict:
        st, pst = self.realign_stats(), self.polish_stats()
        out = dict(offsets=np.zeros(pst["unitigs"] + 1, np.uint64), bases=np.zeros(st["bases_after"], np.uint8), pos=np.zeros(pst["vertices"], np.uint64),
                   nbases=np.zeros(pst["vertices"], np.uint32), stats=np.zeros(pst["unitigs"], POLISH_DT))
        self._chk(self.lib.bella_hip_graph_get_realigned(self.h, *(_p(out[k]) for k in ("offsets", "bases", "pos", "nbases", "stats"))))
        return out

    def realign_placements(self) -> np.ndarray:
        """one record of PLACE_DT per read"""
        out = np.zeros(self.nreads, PLACE_DT)
        self._chk(self.lib.bella_hip_graph_get_realign_placements(self.h, _p(out)))
        return out

    def realign_ops(self):
        """tests: (runs, table) of a round that ran with keep_ops -- the voters' runs (a placement's op_off / nops index them) and the
        round's counters, (bases_before, 9) uint32"""
        n = C.c_uint64(0)
        self._chk(self.lib.bella_hip_graph_get_realign_ops(self.h, C.byref(n), None, None))
        ops, table = np.zeros(n.value, np.uint32), np.zeros((self.realign_stats()["bases_before"], PILEUP_COUNTERS), np.uint32)
        self._chk(self.lib.bella_hip_graph_get_realign_ops(self.h, C.byref(n), _p(ops), _p(table)))
        return ops, table

    def realign_stats(self) -> dict:
        """bella_realign_stats as a dict, plus `wrapped` (its own getter: the voters that reach across an origin)"""
        st = self._stats(self.lib.bella_hip_graph_get_realign_stats, RealignStats)
        w = C.c_uint64(0)
        self._chk(self.lib.bella_hip_graph_get_realign_wrapped(self.h, C.byref(w)))
        st["wrapped"] = w.value
        return st

    # ---- link alignment ----
    LINK_DEFAULTS = dict(band0=512, band_max=4096, min_identity=700)

    def graph_align_links(self, **params) -> int:
        """aligns the ends of the unitigs that every link of the last graph_unitigs joins, on the device, against the newest sequence of
        the unitigs (the last realignment round's, else the polish's, else the raw bases); returns the number of ALIGNED links.  band0,
        band_max (powers of two, 256 .. 4096) and min_identity (permille) default to 512, 4096 and 700"""
        p = _over(self.LINK_DEFAULTS, params, "graph_align_links")
        lp = LinkParams(C.sizeof(LinkParams), p["band0"], p["band_max"], p["min_identity"])
        n = C.c_uint64(0)
        self._chk(self.lib.bella_hip_graph_align_links(self.h, C.byref(lp), C.byref(n)))
        return n.value

    def link_alignments(self):
        """(records of LINK_ALN_DT, one per link in the links' order; the runs of all links, uint32 op | len << 4)"""
        st = self.link_stats()
        alns, ops = np.zeros(st["links"], LINK_ALN_DT), np.zeros(st["ops"], np.uint32)
        n = C.c_uint64(0)
        self._chk(self.lib.bella_hip_graph_get_link_alignments(self.h, _p(alns), C.byref(n), _p(ops)))
        assert n.value == len(ops)
        return alns, ops

    def link_stats(self) -> dict:
        return self._stats(self.lib.bella_hip_graph_get_link_stats, LinkStats)

    # ---- coverage trimming ----
    TRIM_DEFAULTS = dict(min_depth=3, end_clip=500, min_span=1000)

    def graph_trim(self, **params):
        """clips every read to its longest stretch that at least min_depth accumulated records cover (on the device); graph_build then
        cuts the records to the clips, and everything downstream works in clipped coordinates, until graph_untrim, new records or
        new reads.  min_depth, end_clip and min_span default to 3, 500 and 1000"""
        p = _over(self.TRIM_DEFAULTS, params, "trim")
        tp = GraphTrimParams(C.sizeof(GraphTrimParams), p["min_depth"], p["end_clip"], p["min_span"])
        self._chk(self.lib.bella_hip_graph_trim(self.h, C.byref(tp)))

    def graph_clips(self) -> np.ndarray:
        """CLIP_DT[nreads] of the last graph_trim: beg, end (0, 0 = uncovered), nregions, max_depth"""
        out = np.zeros(self.nreads, CLIP_DT)
        self._chk(self.lib.bella_hip_graph_get_trim(self.h, _p(out)))
        return out

    def trim_stats(self) -> dict:
        return self._stats(self.lib.bella_hip_graph_get_trim_stats, TrimStats)

    def graph_untrim(self):
        self._chk(self.lib.bella_hip_graph_untrim(self.h))

    def read_bases(self):
        """(offsets uint64[nreads + 1], bases uint8 ASCII) of the loaded reads"""
        offs = np.zeros(self.nreads + 1, np.uint64)
        self._chk(self.lib.bella_hip_get_read_bases(self.h, offs.ctypes.data, None))
        bases = np.zeros(int(offs[-1]), np.uint8)
        self._chk(self.lib.bella_hip_get_read_bases(self.h, None, _p(bases)))
        return offs, bases

    def trace_batch(self, seeds: np.ndarray, alns: np.ndarray, pars: BellaPars, band0: int = 0):
        """The same on explicit seeds and their alignments (what xdrop_batch returned for them, or any rectangles)."""
        seeds = np.ascontiguousarray(seeds, SEED_DT)
        alns = np.ascontiguousarray(alns, ALN_DT)
        assert len(seeds) == len(alns)
        tr = np.zeros(len(seeds), TRACE_DT)
        cp = pars.c()
        no = C.c_uint64(0)
        self._chk(self.lib.bella_hip_trace_batch(self.h, _p(seeds), _p(alns), len(seeds), C.byref(cp), band0, _p(tr), None, 0, C.byref(no)))
        ops = np.zeros(no.value, np.uint32)           # the runs wait in the context: one trace, then the copy
        self._chk(self.lib.bella_hip_get_batch_ops(self.h, _p(ops), no.value))
        return tr, ops

    # ---- pair alignment ----
    def align_records(self, bases, records, mode="global", band0: int = 512, band_max: int = 4096, scoring=None):
        """bella_hip_align_sequences as it is: bases uint8 (upper-case ACGT), records of ALIGN_PAIR_DT -> (results of ALIGN_RES_DT in the
        records' order, the runs of all pairs as uint32 len << 4 | op).  scoring: None (+1 / -1 / -1, linear gaps), or (match, mismatch,
        gap_open, gap_extend) for bella_hip_align_sequences_affine."""
        bases = np.ascontiguousarray(bases, np.uint8)
        recs = np.ascontiguousarray(records, ALIGN_PAIR_DT)
        ap = AlignParams(C.sizeof(AlignParams), _lib.ALIGN_MODES[mode] if isinstance(mode, str) else int(mode), int(band0), int(band_max))
        out = np.zeros(len(recs), ALIGN_RES_DT)
        no = C.c_uint64(0)
        if scoring is None:
            self._chk(self.lib.bella_hip_align_sequences(self.h, _p(bases), bases.size, _p(recs), len(recs), C.byref(ap), _p(out), C.byref(no)))
        else:
            a, b, o, e = (int(x) for x in scoring)
            if min(a, b, o, e) < 0 or max(a, b, o, e) >= 1 << 32:
                raise ValueError("scoring is four non-negative numbers (match, mismatch, gap_open, gap_extend)")
            sc = AlignScoring(C.sizeof(AlignScoring), a, b, o, e, 0)
            self._chk(self.lib.bella_hip_align_sequences_affine(self.h, _p(bases), bases.size, _p(recs), len(recs), C.byref(ap), C.byref(sc), _p(out), C.byref(no)))
        ops = np.zeros(no.value, np.uint32)
        self._chk(self.lib.bella_hip_get_align_ops(self.h, _p(ops), no.value))
        return out, ops

    def align_sequences(self, seqs, pairs, mode="global", rc=None, centre=None, overlap=None, band0: int = 512, band_max: int = 4096, scoring=None):
        """Aligns pairs of caller-supplied sequences on the device.  seqs: a list of bytes (upper-case ACGT); pairs: (query, target)
        indices into it; rc (per pair, or one for all): the query is reverse-complemented first.  mode: "global" (both whole),
        "semiglobal" (the query whole, a window of the target) or "dovetail" (a suffix of the target against a prefix of the query).
        centre (per pair, or one for all): the diagonal target - query the band is centred on; the default is floor((m - n) / 2), and
        m - overlap for a dovetail with an expected `overlap`.  scoring: None for match +1, mismatch -1, gap -1 (linear), or a 4-tuple
        (match, mismatch, gap_open, gap_extend): match +a, mismatch -b, a gap of L bases -(o + e L) (affine gaps; section 29).  Returns
        (results of ALIGN_RES_DT in the pairs' order, the runs)."""
        lens = np.array([len(s) for s in seqs], np.uint64)
        offs = np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)])
        bases = np.frombuffer(b"".join(bytes(s) for s in seqs), np.uint8)
        pr = np.asarray(pairs, np.int64).reshape(-1, 2)
        recs = np.zeros(len(pr), ALIGN_PAIR_DT)
        recs["q_off"], recs["t_off"] = offs[pr[:, 0]], offs[pr[:, 1]]
        recs["q_len"], recs["t_len"] = lens[pr[:, 0]], lens[pr[:, 1]]
        if rc is not None:
            recs["flags"] = np.where(np.broadcast_to(np.asarray(rc, bool), len(pr)), _lib.ALIGN_PAIR_RC, 0)
        n, m = recs["q_len"].astype(np.int64), recs["t_len"].astype(np.int64)
        if centre is not None:
            recs["centre"] = np.broadcast_to(np.asarray(centre, np.int64), len(pr))
        elif overlap is not None:
            if mode != "dovetail":
                raise TypeError("overlap is the expected overlap of a dovetail")
            recs["centre"] = m - np.broadcast_to(np.asarray(overlap, np.int64), len(pr))
        elif mode == "dovetail":
            raise TypeError("a dovetail needs the expected overlap (or a centre)")
        else:
            recs["centre"] = (m - n) // 2
        return self.align_records(bases, recs, mode, band0, band_max, scoring)

    def align_stats(self) -> dict:
        return self._stats(self.lib.bella_hip_get_align_stats, AlignStats)

    def trace_stats(self) -> TraceStats:
        t = TraceStats()
        self._chk(self.lib.bella_hip_get_trace_stats(self.h, C.byref(t), C.sizeof(t)))
        return t

    def memory(self) -> Memory:
        m = Memory()
        self._chk(self.lib.bella_hip_get_memory(self.h, C.byref(m)))
        return m

    def timings(self) -> Timings:
        t = Timings()
        self._chk(self.lib.bella_hip_get_timings(self.h, C.byref(t)))
        return t


# ---------------------------------------------------------------------------------------------------
# output writers: overlap.hpp:472-473 (BELLA), :476-489 (PAF), :580-585 (--skip-alignment)
# ---------------------------------------------------------------------------------------------------
def overlap_of_seed(pairs, lengths, k):
    """chain.hpp:47-71 overlapop on the chosen seed (int, NOT truncated to u16) from the pair flags."""
    lenH = lengths[pairs["rid"]].astype(np.int64)
    lenV = lengths[pairs["cid"]].astype(np.int64)
    posH = pairs["seedH"].astype(np.int64)
    posV = pairs["seedV"].astype(np.int64)
    oriented = (pairs["flags"] & 1).astype(bool)
    begH = np.where(oriented, posH, (lenH - posH - k) & 0xFFFF)
    endH = (begH + k) & 0xFFFF
    endV = (posV + k) & 0xFFFF
    return np.minimum(begH, posV) + np.minimum(lenH - endH, lenV - endV) + k


def format_skip(names, lengths, pairs, k) -> bytes:
    ov = overlap_of_seed(pairs, lengths, k)
    l16 = lengths & 0xFFFF
    out = ["%s\t%s\t%d\t%d\t%d\t%d\n" % (names[c], names[r], cnt, o, l16[c], l16[r])
           for r, c, cnt, o in zip(pairs["rid"].tolist(), pairs["cid"].tolist(), pairs["count"].tolist(), ov.tolist())]
    return "".join(out).encode()


def format_aligned(names, lengths, pairs, alns, paf=False) -> bytes:
    l16 = (lengths & 0xFFFF).tolist()
    out = []
    for p, a in zip(pairs.tolist(), alns.tolist()):
        rid, cid, count = p[0], p[1], p[2]
        score, bH, eH, bV, eV, ov, strand, passed = a[:8]
        if not passed:
            continue
        r1, r2 = l16[rid], l16[cid]
        if not paf:
            out.append("%s\t%s\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (
                names[cid], names[rid], count, score, ov, "c" if strand else "n", bV, eV, r2, bH, eH, r1))
        else:
            if strand:
                bH, eH = r1 - eH, r1 - bH          # toOriginalCoordinates, overlap.hpp:149-154
            out.append("%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (
                names[cid], r2, bV, eV, "-" if strand else "+", names[rid], r1, bH, eH, score, ov, 255))
    return "".join(out).encode()


def write_output(filename: str, pars: BellaPars, names, lengths, pairs, alns=None, nthreads: int = 0) -> WriteStats:
    """bella_hip_write_output: the library's multi-threaded writer (overlap.hpp:603-642); APPENDS to `filename`."""
    lib = _lib.load()
    n, arr = _names(names)
    lens = np.ascontiguousarray(lengths, np.uint32)
    pairs = np.ascontiguousarray(pairs, PAIR_DT)
    st = WriteStats()
    cp = pars.c()
    if alns is not None:
        alns = np.ascontiguousarray(alns, ALN_DT)
    rc = lib.bella_hip_write_output(filename.encode(), C.byref(cp), 1 if pars.outputPaf else 0, n, arr,
                                    lens.ctypes.data, pairs.ctypes.data if len(pairs) else None,
                                    alns.ctypes.data if alns is not None and len(alns) else None, len(pairs), nthreads, C.byref(st))
    if rc:
        raise BellaHipError(rc, "bella_hip_write_output failed")
    return st


def cigar_strings(traces, ops, reverse=None):
    """CIGAR text (= X I D) of every trace; "" for an untraced pair.  reverse (bool per trace, e.g. alns["strand"] == 1): runs in
    reverse order, as the PAF writer prints a '-' strand line."""
    out = []
    for n, t in enumerate(traces):
        o = ops[int(t["op_off"]):int(t["op_off"]) + int(t["nops"])]
        if reverse is not None and reverse[n]:
            o = o[::-1]
        out.append("".join("%d%s" % (int(w) >> 4, "=XID"[int(w) & 3]) for w in o))
    return out


def write_output_traced(filename: str, pars: BellaPars, names, lengths, pairs, alns, traces, ops, nthreads: int = 0) -> WriteStats:
    """bella_hip_write_output_traced: true PAF (columns 10/11 = residue matches / block length, AS ov NM cg tags); APPENDS."""
    lib = _lib.load()
    n, arr = _names(names)
    lens = np.ascontiguousarray(lengths, np.uint32)
    pairs = np.ascontiguousarray(pairs, PAIR_DT)
    alns = np.ascontiguousarray(alns, ALN_DT)
    traces = np.ascontiguousarray(traces, TRACE_DT)
    ops = np.ascontiguousarray(ops, np.uint32)
    assert len(pairs) == len(alns) == len(traces)
    st = WriteStats()
    cp = pars.c()
    rc = lib.bella_hip_write_output_traced(filename.encode(), C.byref(cp), n, arr, lens.ctypes.data, _p(pairs), _p(alns),
                                           _p(traces), _p(ops), len(ops), len(pairs), nthreads, C.byref(st))
    if rc:
        raise BellaHipError(rc, "bella_hip_write_output_traced failed")
    return st


def write_fasta(filename: str, names, offsets, bases, append: bool = False) -> None:
    """bella_hip_write_fasta: '>name' + one sequence line per read (what Engine.consensus returned), reads in input order."""
    lib = _lib.load()
    n, arr = _names(names)
    offs = np.ascontiguousarray(offsets, np.uint64)
    b = np.ascontiguousarray(bases, np.uint8)
    assert len(offs) == n + 1
    rc = lib.bella_hip_write_fasta(os.fsencode(filename), n, arr, offs.ctypes.data, _p(b), 1 if append else 0)
    if rc:
        raise BellaHipError(rc, "bella_hip_write_fasta failed")


def write_gfa(filename: str, names, lengths, offsets, edges, contained, seqs=None) -> None:
    """bella_hip_write_gfa: GFA 1 of a graph (what Engine.graph returned): S lines of the non-contained reads in input order -- with the
    reads' own bases (seqs: one bytes per read) or '*' -- and one L line per edge in list order."""
    lib = _lib.load()
    n, arr = _names(names)
    lens = np.ascontiguousarray(lengths, np.uint32)
    offs = np.ascontiguousarray(offsets, np.uint64)
    edges = np.ascontiguousarray(edges, EDGE_DT)
    cont = np.ascontiguousarray(contained, np.uint8)
    assert len(offs) == 2 * n + 1 and len(cont) == n == len(lens) and int(offs[-1]) == len(edges)
    boffs = bases = None
    if seqs is not None:
        boffs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
        bases = np.frombuffer(b"".join(bytes(s) for s in seqs), np.uint8)
    rc = lib.bella_hip_write_gfa(os.fsencode(filename), n, arr, _p(lens), boffs.ctypes.data if boffs is not None else None,
                                 (bases.ctypes.data if len(bases) else boffs.ctypes.data) if bases is not None else None, offs.ctypes.data, _p(edges), _p(cont))
    if rc:
        raise BellaHipError(rc, "bella_hip_write_gfa failed")


def trimmed_reads(offsets, bases, clips):
    """(offsets uint64[nreads + 1], bases uint8) of the reads cut to their clips (what Engine.graph_clips returned), on the host: an
    uncovered read becomes empty.  Serves the S lines of the trimmed graph and the FASTA of the trimmed reads."""
    offs = np.asarray(offsets, np.int64)
    b = np.asarray(bases, np.uint8)
    clips = np.asarray(clips)
    assert len(clips) == len(offs) - 1
    beg, end = clips["beg"].astype(np.int64), clips["end"].astype(np.int64)
    assert np.all(beg <= end) and np.all(end <= np.diff(offs))
    n = end - beg
    out = np.zeros(len(clips) + 1, np.uint64)
    out[1:] = np.cumsum(n)
    first = out[:-1].astype(np.int64)
    idx = np.arange(int(out[-1]), dtype=np.int64) + np.repeat(offs[:-1] + beg - first, n)
    return out, b[idx]


def unitig_names(circular) -> list:
    return ["utg%06d%s" % (k + 1, "c" if c else "l") for k, c in enumerate(np.asarray(circular).tolist())]


def write_unitig_gfa(filename: str, names, unitigs: dict, offsets=None, bases=None, link_alns=None, link_ops=None) -> None:
    """bella_hip_write_unitig_gfa: GFA 1 of what Engine.graph_unitigs returned: S and a lines per unitig, L lines per link; with the
    unitigs' bases (what Engine.unitig_bases returned) or '*'.  link_alns / link_ops (what Engine.link_alignments returned): the
    ALIGNED links' lines carry their CIGAR, NM:i: and ol:i: (bella_hip_write_unitig_gfa_links)"""
    lib = _lib.load()
    n, arr = _names(names)
    u = unitigs
    a = {k: np.ascontiguousarray(u[k], dt) for k, dt in (("voff", np.uint64), ("verts", np.uint32), ("pos", np.uint64), ("nbases", np.uint32), ("len", np.uint64),
                                                         ("circular", np.uint8), ("links", LINK_DT))}
    boffs = b = None
    if bases is not None:
        boffs, b = np.ascontiguousarray(offsets, np.uint64), np.ascontiguousarray(bases, np.uint8)
        assert len(boffs) == len(a["len"]) + 1
        if not len(b):
            b = np.zeros(1, np.uint8)                                 # (no bases at all: still a pointer, NULL would mean '*')
    args = (os.fsencode(filename), n, arr, len(a["len"]), a["voff"].ctypes.data, _p(a["verts"]), _p(a["pos"]), _p(a["nbases"]), _p(a["len"]), _p(a["circular"]),
            boffs.ctypes.data if boffs is not None else None, b.ctypes.data if b is not None else None, len(a["links"]), _p(a["links"]))
    if link_alns is None:
        rc, who = lib.bella_hip_write_unitig_gfa(*args), "bella_hip_write_unitig_gfa"
    else:
        la = np.ascontiguousarray(link_alns, LINK_ALN_DT)
        lo = np.ascontiguousarray(link_ops if link_ops is not None else np.zeros(0, np.uint32), np.uint32)
        assert len(la) == len(a["links"])
        assert not len(la) or int((la["op_off"] + la["nops"]).max()) <= len(lo), "the links' runs lie outside link_ops"
        if not len(lo):
            lo = np.zeros(1, np.uint32)
        rc, who = lib.bella_hip_write_unitig_gfa_links(*args, _p(la), _p(lo)), "bella_hip_write_unitig_gfa_links"
    if rc:
        raise BellaHipError(rc, who + " failed")


def link_cigars(alns, ops) -> list:
    """the CIGAR (bytes; M / I / D, '=' and 'X' merged into M) of every ALIGNED link, None for the others: what the L lines carry"""
    out = []
    for a in np.asarray(alns):
        if int(a["status"]) != _lib.LINK_ALIGNED:
            out.append(None)
            continue
        text, run, last = [], 0, None
        for w in np.asarray(ops[int(a["op_off"]):int(a["op_off"]) + int(a["nops"])], np.uint32).tolist():
            ch = b"MMID"[w & 15:(w & 15) + 1]
            if ch != last and run:
                text.append(b"%d%s" % (run, last))
                run = 0
            last, run = ch, run + (w >> 4)
        if run:
            text.append(b"%d%s" % (run, last))
        out.append(b"".join(text))
    return out


def align_cigars(results, ops, eqx: bool = True) -> list:
    """the CIGAR (bytes) of every ALIGNED pair of Engine.align_sequences, None for the others: '=' / 'X' / 'I' / 'D', or with eqx False
    M / I / D ('=' and 'X' merged into M).  An ALIGNED pair without runs (a dovetail that ends in row 0) has the empty CIGAR."""
    letters = b"=XID" if eqx else b"MMID"
    out = []
    for a in np.asarray(results):
        if int(a["status"]) != _lib.ALIGN_ALIGNED:
            out.append(None)
            continue
        text, run, last = [], 0, None
        for w in np.asarray(ops[int(a["op_off"]):int(a["op_off"]) + int(a["nops"])], np.uint32).tolist():
            ch = letters[w & 15:(w & 15) + 1]
            if ch != last and run:
                text.append(b"%d%s" % (run, last))
                run = 0
            last, run = ch, run + (w >> 4)
        if run:
            text.append(b"%d%s" % (run, last))
        out.append(b"".join(text))
    return out


def hash_spgemm(engine: Engine, pars: BellaPars, filename: str, stdout=sys.stdout, stages: int = 1):
    """HashSpGEMM-shaped driver (include/overlap.hpp:650-789): the operands and reads are already in `engine`.
    Writes `filename` and the stdout protocol lines nnz(C) (:686) and, when aligning, outputted per stage (:771).
    stages > 1: the output is formed in stages of consecutive columns like the reference does under a memory budget
    (:682-789); the file is the same, every pass only holds its own columns."""
    nreads = engine.nreads
    bounds = [(nreads * b) // stages for b in range(stages + 1)]
    outputted, total = [], 0
    open(filename, "wb").close()
    try:
        for b in range(stages):
            if stages > 1:
                engine.set_column_range(bounds[b], bounds[b + 1] - bounds[b])
            npairs, _ = engine.overlap(pars)
            total += npairs
            pairs, _, _ = engine.get_pairs(ext=False)
            if pars.skipAlignment:
                write_output(filename, pars, engine.names, engine.lengths, pairs)
            else:
                outputted.append(engine.align_pairs(pars))
                write_output(filename, pars, engine.names, engine.lengths, pairs, engine.get_alignments())
    finally:
        if stages > 1:
            engine.set_column_range(0, 0xFFFFFFFF)
    print(total, file=stdout)
    for o in outputted:
        print(o, file=stdout)
    return total
