"""ctypes mirror of the C-ABI (include/minivite_hip.h).

Graph construction runs on the host and works anywhere; Engine needs an
MI355X (mv_engine_create fails loudly without one — no CPU fallback).
"""
import ctypes
import os

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
_LIB = None

COMM_ID_BYTES = 128


class MvStats(ctypes.Structure):
    _fields_ = [
        ("total_ms", ctypes.c_double),
        ("sweep_ms", ctypes.c_double),
        ("sweep_launches", ctypes.c_int64),
        ("halo_ms", ctypes.c_double),
        ("setup_ms", ctypes.c_double),
        ("edges_local", ctypes.c_int64),
        ("iters", ctypes.c_int),
    ]


SWEEP_SLOTS = (4, 8, 12, 16, 24, 32, 48)  # general_slots index -> SLOTS


class MvSweepInfo(ctypes.Structure):
    _fields_ = [
        ("general", ctypes.c_int64),
        ("general_slots", ctypes.c_int64 * len(SWEEP_SLOTS)),
        ("iter1_label_order", ctypes.c_int64),
        ("iter1_internal_order", ctypes.c_int64),
        ("hi", ctypes.c_int64),
        ("lh", ctypes.c_int64),
        ("nhi", ctypes.c_int64),
        ("nlh", ctypes.c_int64),
        ("nghost", ctypes.c_int64),
        ("ssz", ctypes.c_int64),
        ("nexp", ctypes.c_int64),
        ("skewed", ctypes.c_int),
        ("overlap", ctypes.c_int),
        ("rows_sorted", ctypes.c_int),
        ("sell_sorted", ctypes.c_int),
        ("unit_weights", ctypes.c_int),
        ("deg_window", ctypes.c_int64),
        ("deg_quant", ctypes.c_int64),
        ("row_group", ctypes.c_int64),
        ("sell_entries", ctypes.c_int64),
        ("sched_unit", ctypes.c_int64),
        ("sched_grid", ctypes.c_int64),
        ("sched_tickets", ctypes.c_int64),
        ("sched_tickets_expected", ctypes.c_int64),
        ("perm_identity", ctypes.c_int64),
        ("slot_bytes", ctypes.c_int64),
    ]


class MvHaloInfo(ctypes.Structure):
    _fields_ = [(name, ctypes.c_int64) for name in (
        "exchanges",
        "send_full", "send_compact", "send_silent",
        "recv_full", "recv_compact", "recv_silent",
        "send_compact_entries", "recv_compact_entries",
        "prep_calls", "nrc_sum", "nrc_max", "nrc_zero", "nreq_sum")]


class MvPhaseInfo(ctypes.Structure):
    _fields_ = [
        ("iters", ctypes.c_int),
        ("run_mod", ctypes.c_double),
        ("nv_in", ctypes.c_int64),
        ("ne_in", ctypes.c_int64),
        ("run_ms", ctypes.c_double),
        ("coarsen_ms", ctypes.c_double),
        ("kept", ctypes.c_int),
    ]


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_DIR, "libminivite.so")
        if not os.path.exists(path):
            raise RuntimeError(
                "libminivite.so not built — run `make -C minivite_amd/csrc` "
                "or __graft_entry__.build()")
        L = ctypes.CDLL(path)
        i64, f64, vp = ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
        pi64 = ctypes.POINTER(i64)
        pf64 = ctypes.POINTER(f64)
        L.mv_graph_rgg.restype = vp
        L.mv_graph_rgg.argtypes = [i64, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, f64, ctypes.c_uint64]
        L.mv_graph_read_binary.restype = vp
        L.mv_graph_read_binary.argtypes = [ctypes.c_char_p, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int]
        L.mv_graph_from_csr.restype = vp
        L.mv_graph_from_csr.argtypes = [i64, ctypes.c_int, ctypes.c_int, pi64,
                                        i64, i64, pi64, pi64, pf64]
        L.mv_graph_write_binary.restype = ctypes.c_int
        L.mv_graph_write_binary.argtypes = [vp, ctypes.c_char_p]
        L.mv_graph_free.restype = None
        L.mv_graph_free.argtypes = [vp]
        for name in ("mv_graph_nv", "mv_graph_lnv", "mv_graph_lne"):
            getattr(L, name).restype = i64
            getattr(L, name).argtypes = [vp]
        for name in ("mv_graph_parts", "mv_graph_xadj", "mv_graph_tails"):
            getattr(L, name).restype = pi64
            getattr(L, name).argtypes = [vp]
        for name in ("mv_graph_rank", "mv_graph_nranks"):
            getattr(L, name).restype = ctypes.c_int
            getattr(L, name).argtypes = [vp]
        L.mv_graph_weights.restype = pf64
        L.mv_graph_weights.argtypes = [vp]
        pi32 = ctypes.POINTER(ctypes.c_int32)
        L.mv_graph_locality_hint.restype = pi32
        L.mv_graph_locality_hint.argtypes = [vp]
        L.mv_degree_window_order.restype = ctypes.c_int
        L.mv_degree_window_order.argtypes = [pi32, pi64, i64, i64, i64, i64,
                                             pi32]
        L.mv_sweep_schedule.restype = ctypes.c_int
        L.mv_sweep_schedule.argtypes = [i64, ctypes.c_int, i64, i64,
                                        ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_int), pi64,
                                        pi64]
        L.mv_comm_id.restype = ctypes.c_int
        L.mv_comm_id.argtypes = [ctypes.c_void_p]
        L.mv_lb_create.restype = vp
        L.mv_lb_create.argtypes = [ctypes.c_int]
        L.mv_lb_destroy.restype = None
        L.mv_lb_destroy.argtypes = [vp]
        L.mv_engine_create_lb.restype = vp
        L.mv_engine_create_lb.argtypes = [ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, vp]
        L.mv_engine_create.restype = vp
        L.mv_engine_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p]
        L.mv_engine_destroy.restype = None
        L.mv_engine_destroy.argtypes = [vp]
        L.mv_engine_load_graph.restype = ctypes.c_int
        L.mv_engine_load_graph.argtypes = [vp, vp]
        L.mv_engine_run.restype = f64
        L.mv_engine_run.argtypes = [vp, f64, f64, ctypes.POINTER(ctypes.c_int)]
        L.mv_engine_set_trace.restype = None
        L.mv_engine_set_trace.argtypes = [vp, pi64, pf64, ctypes.c_int]
        L.mv_engine_get_stats.restype = None
        L.mv_engine_get_stats.argtypes = [vp, ctypes.POINTER(MvStats)]
        L.mv_engine_get_sweep_info.restype = None
        L.mv_engine_get_sweep_info.argtypes = [vp,
                                               ctypes.POINTER(MvSweepInfo)]
        L.mv_engine_get_halo_info.restype = None
        L.mv_engine_get_halo_info.argtypes = [vp, ctypes.POINTER(MvHaloInfo)]
        L.mv_engine_get_communities.restype = ctypes.c_int
        L.mv_engine_get_communities.argtypes = [vp, pi64]
        L.mv_coarsen_csr.restype = vp
        L.mv_coarsen_csr.argtypes = [ctypes.c_int, vp, pi64, pi64]
        L.mv_engine_run_multiphase.restype = vp
        L.mv_engine_run_multiphase.argtypes = [vp, vp, f64, f64, ctypes.c_int]
        L.mv_engine_coarsen_dist.restype = vp
        L.mv_engine_coarsen_dist.argtypes = [vp, vp, pi64, pi64]
        L.mv_engine_run_multiphase_dist.restype = vp
        L.mv_engine_run_multiphase_dist.argtypes = [vp, vp, f64, f64,
                                                    ctypes.c_int]
        for name in ("mv_hierarchy_phases", "mv_hierarchy_levels"):
            getattr(L, name).restype = ctypes.c_int
            getattr(L, name).argtypes = [vp]
        L.mv_hierarchy_graph.restype = vp
        L.mv_hierarchy_graph.argtypes = [vp, ctypes.c_int]
        L.mv_hierarchy_map.restype = pi64
        L.mv_hierarchy_map.argtypes = [vp, ctypes.c_int]
        L.mv_hierarchy_modularity.restype = f64
        L.mv_hierarchy_modularity.argtypes = [vp, ctypes.c_int]
        L.mv_hierarchy_phase_info.restype = ctypes.c_int
        L.mv_hierarchy_phase_info.argtypes = [vp, ctypes.c_int,
                                              ctypes.POINTER(MvPhaseInfo)]
        L.mv_hierarchy_phase_proposal.restype = ctypes.c_int
        L.mv_hierarchy_phase_proposal.argtypes = [vp, ctypes.c_int, pi64, pf64]
        L.mv_hierarchy_communities.restype = pi64
        L.mv_hierarchy_communities.argtypes = [vp]
        L.mv_hierarchy_free.restype = None
        L.mv_hierarchy_free.argtypes = [vp]
        _LIB = L
    return _LIB


def _i64p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _f64p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def comm_id():
    """RCCL unique id bytes (call on rank 0, broadcast out of band)."""
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    if lib().mv_comm_id(buf) != 0:
        raise RuntimeError("mv_comm_id failed")
    return bytes(buf.raw)


class Graph:
    """This rank's slice of the 1-D partitioned CSR (host memory)."""

    def __init__(self, handle, owns=True):
        if not handle:
            raise RuntimeError("graph construction failed")
        self.h = handle
        self._owns = owns

    @classmethod
    def rgg(cls, nv, rank=0, nranks=1, unit_weight=True,
            random_edge_percent=0.0, random_edge_seed=7177):
        return cls(lib().mv_graph_rgg(nv, rank, nranks,
                                      1 if unit_weight else 0,
                                      random_edge_percent, random_edge_seed))

    @classmethod
    def read_binary(cls, path, rank=0, nranks=1, balanced=False):
        return cls(lib().mv_graph_read_binary(path.encode(), rank, nranks,
                                              1 if balanced else 0))

    @classmethod
    def from_csr(cls, nv, rank, nranks, parts, xadj, tails, weights=None):
        parts = np.ascontiguousarray(parts, dtype=np.int64)
        xadj = np.ascontiguousarray(xadj, dtype=np.int64)
        tails = np.ascontiguousarray(tails, dtype=np.int64)
        wp = None
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float64)
            wp = _f64p(weights)
        return cls(lib().mv_graph_from_csr(nv, rank, nranks, _i64p(parts),
                                           len(xadj) - 1, len(tails),
                                           _i64p(xadj), _i64p(tails), wp))

    @property
    def nv(self):
        return lib().mv_graph_nv(self.h)

    @property
    def lnv(self):
        return lib().mv_graph_lnv(self.h)

    @property
    def lne(self):
        return lib().mv_graph_lne(self.h)

    @property
    def parts(self):
        """Ownership bounds of the 1-D partition (read-only copy): rank r
        owns the global ids [parts[r], parts[r+1]). Its length is the rank
        count the graph was built for, plus one."""
        n = lib().mv_graph_nranks(self.h)
        a = np.ctypeslib.as_array(lib().mv_graph_parts(self.h),
                                  (n + 1,)).copy()
        a.flags.writeable = False
        return a

    def arrays(self):
        lnv, lne = self.lnv, self.lne
        xadj = np.ctypeslib.as_array(lib().mv_graph_xadj(self.h), (lnv + 1,)).copy()
        if lne == 0:  # an empty vector's data pointer may be NULL
            return xadj, np.zeros(0, dtype=np.int64), np.zeros(0)
        tails = np.ctypeslib.as_array(lib().mv_graph_tails(self.h), (lne,)).copy()
        w = np.ctypeslib.as_array(lib().mv_graph_weights(self.h), (lne,)).copy()
        return xadj, tails, w

    def locality_hint(self):
        """The builder's internal-layout hint (copy), or None."""
        p = lib().mv_graph_locality_hint(self.h)
        if not p:
            return None
        return np.ctypeslib.as_array(p, (self.lnv,)).copy()

    def write_binary(self, path):
        if lib().mv_graph_write_binary(self.h, path.encode()) != 0:
            raise RuntimeError("mv_graph_write_binary failed")

    def free(self):
        if getattr(self, "h", None) and self._owns:
            lib().mv_graph_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def degree_window_order(hint, xadj, window, quant=1, group=1):
    """mv_degree_window_order on the host: the windowed degree order of
    `hint` (None: the identity) for the CSR row bounds `xadj`."""
    xadj = np.ascontiguousarray(xadj, dtype=np.int64)
    lnv = len(xadj) - 1
    hp = None
    if hint is not None:
        hint = np.ascontiguousarray(hint, dtype=np.int32)
        if hint.shape != (lnv,):
            raise ValueError("hint must hold one vertex per position")
        hp = hint.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    out = np.empty(lnv, dtype=np.int32)
    if lib().mv_degree_window_order(
            hp, _i64p(xadj), lnv, window, quant, group,
            out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) != 0:
        raise ValueError("window must be a power of two >= 128, quant >= 1, "
                         "group a power of two <= window/64")
    return out


def sweep_schedule(lnv, sweep_grid, window=2048, positions=0, unit=1,
                   launch_grid=1):
    """mv_sweep_schedule on the host. Returns (default unit U, default
    row_group, per-head ticket additions of one queued launch)."""
    u = ctypes.c_int()
    s = ctypes.c_int64()
    tickets = np.zeros(8, dtype=np.int64)
    heads = lib().mv_sweep_schedule(lnv, sweep_grid, window, positions, unit,
                                    launch_grid, ctypes.byref(u),
                                    ctypes.byref(s), _i64p(tickets))
    if heads < 0:
        raise ValueError("sizes must be >= 0, grids and unit >= 1")
    return u.value, s.value, [int(t) for t in tickets[:heads]]


def coarsen_csr(graph, comm, device=0):
    """Aggregate the single-rank `graph` by the labels `comm` (values in
    [0, nv)) on the GPU. Returns (coarse Graph, fine->coarse map)."""
    comm = np.ascontiguousarray(comm, dtype=np.int64)
    if comm.shape != (graph.lnv,):
        raise ValueError("comm must hold one label per vertex")
    cmap = np.empty(graph.lnv, dtype=np.int64)
    h = lib().mv_coarsen_csr(device, graph.h, _i64p(comm), _i64p(cmap))
    if not h:
        raise RuntimeError("mv_coarsen_csr failed (label out of range, "
                           "multi-rank graph, or no GPU)")
    return Graph(h), cmap


class Hierarchy:
    """Result of Engine.run_multiphase: levels 1..levels of coarse graphs,
    the maps between them, q per level and per-phase records."""

    def __init__(self, handle, nv0):
        self.h = handle
        self._nv0 = nv0  # vertices of g this rank owns (all of them at p=1)

    @property
    def phases(self):
        return lib().mv_hierarchy_phases(self.h)

    @property
    def levels(self):
        return lib().mv_hierarchy_levels(self.h)

    def graph(self, level):
        """Level 1..levels as a Graph view (owned by the hierarchy)."""
        g = lib().mv_hierarchy_graph(self.h, level)
        if not g:
            raise IndexError(f"level {level} not in 1..{self.levels}")
        return Graph(g, owns=False)

    def map(self, level):
        """Dense map from level-1 vertices to level vertices."""
        if not 1 <= level <= self.levels:
            raise IndexError(f"level {level} not in 1..{self.levels}")
        n = self._nv0 if level == 1 else self.graph(level - 1).lnv
        if n == 0:  # this rank owns nothing there: the pointer may be NULL
            return np.zeros(0, dtype=np.int64)
        p = lib().mv_hierarchy_map(self.h, level)
        return np.ctypeslib.as_array(p, (n,)).copy()

    def modularity(self, level):
        if not 0 <= level <= self.levels:
            raise IndexError(f"level {level} not in 0..{self.levels}")
        return lib().mv_hierarchy_modularity(self.h, level)

    def phase_info(self, phase):
        """Phase 1..phases: the mv_phase_info fields plus what the phase
        proposed (nv_out, q_out)."""
        s = MvPhaseInfo()
        nv_out, q_out = ctypes.c_int64(0), ctypes.c_double(0.0)
        if lib().mv_hierarchy_phase_info(self.h, phase, ctypes.byref(s)) != 0:
            raise IndexError(f"phase {phase} not in 1..{self.phases}")
        lib().mv_hierarchy_phase_proposal(self.h, phase,
                                          ctypes.byref(nv_out),
                                          ctypes.byref(q_out))
        d = {f: getattr(s, f) for f, _ in s._fields_}
        d["kept"] = bool(d["kept"])
        d["nv_out"], d["q_out"] = nv_out.value, q_out.value
        return d

    @property
    def communities(self):
        if self._nv0 == 0:  # a rank without vertices
            return np.zeros(0, dtype=np.int64)
        p = lib().mv_hierarchy_communities(self.h)
        return np.ctypeslib.as_array(p, (self._nv0,)).copy()

    def free(self):
        if getattr(self, "h", None):
            lib().mv_hierarchy_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class LoopbackSession:
    """Hardware-validation harness: nranks engines in ONE process on ONE
    device (see minivite_hip.h). Test-only; product multi-GPU is RCCL."""

    def __init__(self, nranks):
        self.nranks = nranks
        self.h = lib().mv_lb_create(nranks)
        if not self.h:
            raise RuntimeError("mv_lb_create failed")

    def destroy(self):
        if getattr(self, "h", None):
            lib().mv_lb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Engine:
    """The GPU Louvain engine (one per process, one GPU)."""

    def __init__(self, device=0, rank=0, nranks=1, comm_id_bytes=None):
        cid = None
        if comm_id_bytes is not None:
            cid = ctypes.create_string_buffer(comm_id_bytes, COMM_ID_BYTES)
        self.h = lib().mv_engine_create(device, rank, nranks, cid)
        if not self.h:
            raise RuntimeError(
                "mv_engine_create failed — an MI355X GPU is required; "
                "there is no CPU fallback")
        self.rank = rank
        self._trace_buf = None

    @classmethod
    def loopback(cls, session, rank, device=0):
        """Rank `rank` of a LoopbackSession (all ranks share `device`)."""
        obj = cls.__new__(cls)
        obj.h = lib().mv_engine_create_lb(device, rank, session.nranks,
                                          session.h)
        if not obj.h:
            raise RuntimeError("mv_engine_create_lb failed")
        obj.rank = rank
        obj._trace_buf = None
        return obj

    def load_graph(self, g):
        if lib().mv_engine_load_graph(self.h, g.h) != 0:
            raise RuntimeError("mv_engine_load_graph failed")
        self._lnv = g.lnv

    def set_trace(self, cap=256):
        self._trace_buf = np.zeros(cap * self._lnv, dtype=np.int64)
        self._trace_mod = np.zeros(cap, dtype=np.float64)
        self._trace_cap = cap
        lib().mv_engine_set_trace(self.h, _i64p(self._trace_buf),
                                  _f64p(self._trace_mod), cap)

    def run(self, lower=-1.0, thresh=1e-6):
        it = ctypes.c_int(0)
        mod = lib().mv_engine_run(self.h, lower, thresh, ctypes.byref(it))
        return mod, it.value

    def trace(self, iters):
        n = min(iters, self._trace_cap)
        return (self._trace_buf.reshape(self._trace_cap, self._lnv)[:n],
                self._trace_mod[:n])

    def communities(self):
        """This rank's community labels (global vertex ids) of the last
        run(): the phase assignment (see mv_engine_get_communities)."""
        out = np.empty(self._lnv, dtype=np.int64)
        if lib().mv_engine_get_communities(self.h, _i64p(out)) != 0:
            raise RuntimeError("mv_engine_get_communities: no run yet")
        return out

    def run_multiphase(self, graph, lower=-1.0, thresh=1e-6, max_phases=0):
        """Multi-phase Louvain on `graph` (single rank). The engine is left
        holding the last level it loaded: load_graph() again before a
        plain run()."""
        h = lib().mv_engine_run_multiphase(self.h, graph.h, lower, thresh,
                                           max_phases)
        if not h:
            raise RuntimeError("mv_engine_run_multiphase failed")
        hier = Hierarchy(h, graph.nv)
        self._lnv = hier.phase_info(hier.phases)["nv_in"]  # last load
        self._trace_buf = None  # the loads dropped any armed trace
        return hier

    def run_multiphase_dist(self, graph, lower=-1.0, thresh=1e-6,
                            max_phases=0):
        """Multi-phase Louvain on the partitioned graph whose slice of
        this rank is `graph`. Collective: every rank calls it together. The
        Hierarchy is this rank's view (slices, local maps, local
        communities; see mv_engine_run_multiphase_dist). The engine is left
        holding the last level it loaded."""
        h = lib().mv_engine_run_multiphase_dist(self.h, graph.h, lower,
                                                thresh, max_phases)
        if not h:
            raise RuntimeError("mv_engine_run_multiphase_dist failed")
        hier = Hierarchy(h, graph.lnv)
        # phase P ran on level P-1, the last graph the driver loaded
        last = hier.phases - 1
        self._lnv = graph.lnv if last == 0 else hier.graph(last).lnv
        self._trace_buf = None  # the loads dropped any armed trace
        return hier

    def coarsen_dist(self, graph, comm):
        """Aggregate the partitioned graph (this rank's slice `graph`) by
        the global labels `comm` (one per local vertex, values in [0, nv)).
        Collective. Returns (this rank's slice of the coarse Graph, global
        coarse id of each local vertex); raises on every rank when any rank
        saw an error."""
        comm = np.ascontiguousarray(comm, dtype=np.int64)
        if comm.shape != (graph.lnv,):
            raise ValueError("comm must hold one label per local vertex")
        cmap = np.empty(graph.lnv, dtype=np.int64)
        h = lib().mv_engine_coarsen_dist(self.h, graph.h, _i64p(comm),
                                         _i64p(cmap))
        if not h:
            raise RuntimeError("mv_engine_coarsen_dist failed on some rank "
                               "(label out of range, not this rank's slice, "
                               "or a size limit)")
        return Graph(h), cmap

    def stats(self):
        s = MvStats()
        lib().mv_engine_get_stats(self.h, ctypes.byref(s))
        return {f: getattr(s, f) for f, _ in s._fields_}

    def sweep_info(self):
        """Kernel shapes launched by the last run() and the routing state
        behind them (mv_sweep_info); general_slots becomes {SLOTS: count}.
        With the row queue on (sched_unit > 0) the call waits for the
        engine's stream and copies the eight ticket words from the device;
        otherwise it touches only host state."""
        s = MvSweepInfo()
        lib().mv_engine_get_sweep_info(self.h, ctypes.byref(s))
        d = {f: getattr(s, f) for f, _ in s._fields_}
        d["general_slots"] = dict(zip(SWEEP_SLOTS, s.general_slots))
        return d

    def halo_info(self):
        """What the halo plans of the last run() carried on this rank
        (mv_halo_info): exchanges, segments per arm, candidate counts."""
        s = MvHaloInfo()
        lib().mv_engine_get_halo_info(self.h, ctypes.byref(s))
        return {f: getattr(s, f) for f, _ in s._fields_}

    def destroy(self):
        if getattr(self, "h", None):
            lib().mv_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
