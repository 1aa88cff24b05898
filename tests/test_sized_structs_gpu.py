"""The sized-struct handshake of the C ABI (include/bella_hip.h), through bella_amd._lib on an Engine's handle: a getter writes at most
struct_size bytes; a parameter struct shorter than the library's is refused by name, a longer one is read up to the library's size, and
NULL means the defaults where the entry point has any.  Input: unitig_mirror.two_round_input (33 reads of 10 kb, explicit records),
run once per module through graph -> clean -> pop bubbles -> unitigs -> pileup -> polish."""
import ctypes as C

import numpy as np
import pytest

from bella_amd import Engine, _lib
from bella_testkit import synth
from bella_testkit import unitig_mirror as U

pytestmark = pytest.mark.gpu

BAD, STATE = -3, -7
FILL = 0xA5
GRAPH = (_lib.GraphParams, "bella_graph_params", (1000, 1000, 800, 1000))
CLEAN = (_lib.GraphCleanParams, "bella_graph_clean_params", (4, 3))
BUBBLE = (_lib.GraphBubbleParams, "bella_graph_bubble_params", (64, 50000, 3))
POLISH = (_lib.PolishParams, "bella_polish_params", (3,))
CONS = (_lib.ConsensusParams, "bella_consensus_params", (3,))


def _exact(kind):
    cls, _, values = kind
    return cls(C.sizeof(cls), *values)


def _longer(kind):
    """the struct followed by 8 zero bytes, struct_size saying so: what a caller built against a later header passes"""
    cls, _, values = kind
    raw = (C.c_uint8 * (C.sizeof(cls) + 8))()
    C.memmove(raw, C.byref(cls(C.sizeof(cls) + 8, *values)), C.sizeof(cls))
    return raw


def _short(kind):
    cls, _, values = kind
    return cls(C.sizeof(cls) - 4, *values)


def _ptr(kind, obj):
    return None if obj is None else C.cast(C.byref(obj), C.POINTER(kind[0]))


def _err(e):
    return e.lib.bella_hip_last_error(e.h).decode()


def _fields(st):
    """a statistics struct without its timers"""
    out = {}
    for k, _ in st._fields_:
        if not k.endswith("_ms"):
            v = getattr(st, k)
            out[k] = list(v) if isinstance(v, C.Array) else v
    return out


def _stats(e, fn, cls):
    st = cls()
    assert fn(e.h, C.byref(st), C.sizeof(st)) == 0
    return _fields(st)


def _graph_state(e):
    off, edges, cont = e.graph()
    return off.tobytes(), edges.tobytes(), cont.tobytes(), e.graph_removed().tobytes()


def _build(e, p):
    assert e.lib.bella_hip_graph_build(e.h, _ptr(GRAPH, p)) == 0, _err(e)
    return _graph_state(e), _stats(e, e.lib.bella_hip_graph_get_stats, _lib.GraphStats)


def _clean(e, p):
    _build(e, _exact(GRAPH))
    assert e.lib.bella_hip_graph_clean(e.h, _ptr(CLEAN, p)) == 0, _err(e)
    return _graph_state(e), _stats(e, e.lib.bella_hip_graph_get_unitig_stats, _lib.UnitigStats)


def _pop(e, p):
    _clean(e, _exact(CLEAN))
    assert e.lib.bella_hip_graph_pop_bubbles(e.h, _ptr(BUBBLE, p)) == 0, _err(e)
    return _graph_state(e), _stats(e, e.lib.bella_hip_graph_get_bubble_stats, _lib.BubbleStats)


def _polish(e, p):
    assert e.lib.bella_hip_graph_polish_unitigs(e.h, _ptr(POLISH, p), None) == 0, _err(e)
    st = _stats(e, e.lib.bella_hip_graph_get_polish_stats, _lib.PolishStats)
    out = [np.zeros(st["unitigs"] + 1, np.uint64), np.zeros(st["bases_after"], np.uint8), np.zeros(st["vertices"], np.uint64), np.zeros(st["vertices"], np.uint32),
           np.zeros(st["unitigs"], _lib.POLISH_DT)]
    assert e.lib.bella_hip_graph_get_polished(e.h, *(a.ctypes.data for a in out)) == 0
    return [a.tobytes() for a in out], st


def _consensus(e, p):
    tot = C.c_uint64(0)
    assert e.lib.bella_hip_consensus(e.h, _ptr(CONS, p), C.byref(tot)) == 0, _err(e)
    out = [np.zeros(e.nreads + 1, np.uint64), np.zeros(tot.value, np.uint8), np.zeros(e.nreads, _lib.CONS_DT)]
    assert e.lib.bella_hip_get_consensus(e.h, *(a.ctypes.data for a in out)) == 0
    return [a.tobytes() for a in out]


@pytest.fixture(scope="module")
def run():
    """every stage once with its explicit defaults, with a longer struct and (graph, clean, bubbles) with NULL; the engine is left after
    graph -> clean -> pop bubbles -> unitigs -> pileup -> polish"""
    lens, recs = U.two_round_input()
    seqs = [U.random_genome(int(n), 40 + i) for i, n in enumerate(lens)]
    e = Engine(0)
    e.set_reads(synth.ReadSet.from_strings(seqs))
    e.graph_add_overlaps(recs)
    got = {}
    for name, stage, kind in (("graph", _build, GRAPH), ("clean", _clean, CLEAN), ("bubble", _pop, BUBBLE)):
        got[name] = dict(longer=stage(e, _longer(kind)), null=stage(e, None), exact=stage(e, _exact(kind)))
    assert got["clean"]["exact"][1]["reads_removed"] == 3               # (the input's two rounds of tips: the stages had work to do)
    e.graph_unitigs()
    e.pileup_reset()
    e.add_pileup(0, e.nreads, U.random_table([len(s) for s in seqs], 0))
    got["consensus"] = dict(longer=_consensus(e, _longer(CONS)), exact=_consensus(e, _exact(CONS)))
    got["polish"] = dict(longer=_polish(e, _longer(POLISH)), exact=_polish(e, _exact(POLISH)))
    yield e, got
    e.close()


GETTERS = [("bella_hip_graph_get_stats", _lib.GraphStats), ("bella_hip_graph_get_unitig_stats", _lib.UnitigStats),
           ("bella_hip_graph_get_bubble_stats", _lib.BubbleStats), ("bella_hip_graph_get_polish_stats", _lib.PolishStats),
           ("bella_hip_get_trace_stats", _lib.TraceStats), ("bella_hip_get_memory_sized", _lib.Memory)]


@pytest.mark.parametrize("name,cls", GETTERS, ids=[g[0] for g in GETTERS])
def test_a_getter_writes_at_most_struct_size_bytes(run, name, cls):
    e, _ = run
    fn, size = getattr(e.lib, name), C.sizeof(cls)
    for n in (8, size - 4, size, size + 16):
        full = (C.c_uint8 * size)()
        assert fn(e.h, full, size) == 0
        buf = (C.c_uint8 * (size + 16))(*([FILL] * (size + 16)))
        assert fn(e.h, buf, n) == 0
        k = min(n, size)
        assert bytes(buf[:k]) == bytes(full[:k]), (name, n)
        assert bytes(buf[k:]) == bytes([FILL]) * (size + 16 - k), (name, n)


def test_get_memory_sized_refuses_less_than_one_field(run):
    e, _ = run
    buf = (C.c_uint8 * 8)()
    assert e.lib.bella_hip_get_memory_sized(e.h, buf, 4) == BAD


@pytest.mark.parametrize("entry,kind", [("bella_hip_graph_build", GRAPH), ("bella_hip_graph_clean", CLEAN), ("bella_hip_graph_pop_bubbles", BUBBLE),
                                        ("bella_hip_graph_polish_unitigs", POLISH), ("bella_hip_consensus", CONS)], ids=["graph", "clean", "bubble", "polish", "consensus"])
def test_a_shorter_parameter_struct_is_refused_by_name(run, entry, kind):
    e, _ = run
    short = _short(kind)                                               # (a name: the pointer below does not keep it alive)
    args = (e.h, _ptr(kind, short)) + ((None,) if kind in (POLISH, CONS) else ())
    assert getattr(e.lib, entry)(*args) == BAD
    assert kind[1] in _err(e) and "too small" in _err(e), _err(e)
    # (refused before anything changed: the results of the module's run still stand)
    assert e.lib.bella_hip_graph_get_polish_stats(e.h, (C.c_uint8 * 8)(), 8) == 0


@pytest.mark.parametrize("stage", ["graph", "clean", "bubble", "consensus", "polish"])
def test_a_longer_parameter_struct_gives_the_same_result(run, stage):
    _, got = run
    assert got[stage]["longer"] == got[stage]["exact"]


@pytest.mark.parametrize("stage", ["graph", "clean", "bubble"])
def test_null_means_the_documented_defaults(run, stage):
    """offsets, edges, contained and removed marks byte-equal, the statistics equal apart from the timers"""
    _, got = run
    assert got[stage]["null"] == got[stage]["exact"]


def test_null_is_refused_where_there_are_no_defaults(run):
    e, _ = run
    assert e.lib.bella_hip_graph_polish_unitigs(e.h, None, None) == BAD
    assert e.lib.bella_hip_consensus(e.h, None, None) == BAD and _err(e) == "null argument"


def test_the_graph_getters_want_their_stage_first():
    """on a fresh context; every one of these returns before any launch"""
    e = Engine(0)
    try:
        buf = (C.c_uint8 * 1024)()
        for name, msg in (("bella_hip_graph_get_stats", "bella_hip_graph_build first"), ("bella_hip_graph_get_unitig_stats", "bella_hip_graph_build first"),
                          ("bella_hip_graph_get_bubble_stats", "bella_hip_graph_build first"), ("bella_hip_graph_get_polish_stats", "bella_hip_graph_polish_unitigs first")):
            assert getattr(e.lib, name)(e.h, buf, 1024) == STATE, name
            assert _err(e) == msg, (name, _err(e))
    finally:
        e.close()
