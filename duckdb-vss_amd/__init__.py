"""duckdb-vss_amd — Python driver over libvssgpu.so (the MI355X-native engine behind the C ABI in include/vssgpu.h).

This module is plumbing for tests/ and bench.py: it loads the in-tree shared library with ctypes and exposes one
class, `GpuIndex`, whose methods map 1:1 onto the C entry points (which in turn map onto the calls the reference's
HNSWIndex makes on its usearch member — see include/vssgpu.h for the file:line of each).  There is NO fallback:
if the library is missing or no HIP device is present, construction raises.

The directory name carries a hyphen (it is the repo's package directory, not an importable dotted name); use
`__graft_entry__.load_package()` or importlib to import it.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.environ.get("VSS_LIBRARY") or os.path.join(HERE, "libvssgpu.so")  # VSS_LIBRARY: debug builds only
CSRC = os.path.join(HERE, "csrc")

METRICS = {"l2sq": 0, "cosine": 1, "ip": 2}
FUNCTIONS = {"array_distance": 0, "array_cosine_distance": 1, "array_negative_inner_product": 2}
FREE_KEY = np.iinfo(np.int64).max

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-int-to-pointer-cast"]


TRANSLATION_UNITS = ["vss_engine.hip", "vss_exchange.hip", "kernels_l2sq.hip", "kernels_cosine.hip", "kernels_ip.hip",
                     "kernels_boxes_l2sq.hip", "kernels_boxes_cosine.hip", "kernels_boxes_ip.hip",
                     "kernels_setboxes_l2sq.hip", "kernels_setboxes_cosine.hip", "kernels_setboxes_ip.hip"]


def build_library(force=False, extra_flags=(), out=None):
    """hipcc cross-compiles the engine for gfx950 (works without a GPU): eleven translation units in parallel, then a
    shared link.  Objects live in build/ (git-ignored)."""
    out = out or os.path.join(HERE, "libvssgpu.so")
    srcs = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))]
    srcs.append(os.path.join(ROOT, "include", "vssgpu.h"))
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in srcs):
        return out
    objdir = os.path.join(HERE, "build", os.path.basename(out))
    os.makedirs(objdir, exist_ok=True)
    flags = [f for f in HIPCC_FLAGS if f != "-shared"] + list(extra_flags) + ["-I", os.path.join(ROOT, "include")]
    procs, objs = [], []
    for tu in TRANSLATION_UNITS:
        obj = os.path.join(objdir, tu.replace(".hip", ".o"))
        objs.append(obj)
        procs.append(subprocess.Popen(["hipcc"] + flags + ["-c", os.path.join(CSRC, tu), "-o", obj]))
    for p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", out])
    return out


_u64, _i64, _vp, _int, _u32 = C.c_uint64, C.c_int64, C.c_void_p, C.c_int, C.c_uint32
WRITE_CB = C.CFUNCTYPE(_int, _vp, _vp, _u64)
READ_CB = C.CFUNCTYPE(_int, _vp, _vp, _u64)

# every symbol include/vssgpu.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "vss_version": (C.c_char_p, []),
    "vss_create": (_int, [_u64, _int, _u64, _u64, _u64, _u64, _int, C.POINTER(_vp)]),
    "vss_destroy": (None, [_vp]),
    "vss_last_error": (C.c_char_p, [_vp]),
    "vss_set_stream": (_int, [_vp, _vp]),
    "vss_synchronize": (_int, [_vp]),
    "vss_reserve": (_int, [_vp, _u64, _u64]),
    "vss_stage_batch": (_int, [_vp, _vp, _vp, _vp, _u64]),
    "vss_stage_batch_device": (_int, [_vp, _vp, _vp, _u64]),
    "vss_build_finalize": (_int, [_vp]),
    "vss_add_batch": (_int, [_vp, _vp, _vp, _vp, _u64]),
    "vss_set_build_params": (_int, [_vp, _u64, _u64]),
    "vss_set_build_reorder": (_int, [_vp, _int]),
    "vss_set_option": (_int, [_vp, C.c_char_p, _i64]),
    "vss_search": (_int, [_vp, _vp, _u64, _u64, _vp, _vp]),
    "vss_search_batch": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp]),
    "vss_search_batch_device": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp]),
    "vss_search_batch_filtered": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _vp]),
    "vss_search_batch_filtered_device": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _vp]),
    "vss_search_batch_filtered_groups": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    "vss_search_batch_filtered_groups_device": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    "vss_search_batch_device_begin": (_int, [_vp, _int, _vp, _u64, _u64, _u64, _vp, _vp, _vp]),
    "vss_search_multi_device_begin": (_int, [_vp, _int, _u64, _vp, _u64, _u64, _u64, _vp, _vp, _vp]),
    "vss_search_batch_filtered_device_begin": (_int, [_vp, _int, _vp, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _vp]),
    "vss_search_batch_filtered_groups_device_begin": (_int, [_vp, _int, _vp, _u64, _u64, _u64, _vp, _u64, _u64, _vp, _vp, _vp,
                                                             _vp]),
    "vss_search_multi_filtered_device_begin": (_int, [_vp, _int, _u64, _vp, _u64, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp,
                                                      _vp]),
    "vss_search_by_label_device_begin": (_int, [_vp, _int, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp]),
    "vss_search_multi_by_label_device_begin": (_int, [_vp, _int, _u64, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp]),
    "vss_search_batch_end": (_int, [_vp, _int]),
    "vss_search_exact_batch": (_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp]),
    "vss_search_exact_batch_device": (_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp]),
    "vss_search_exact_batch_filtered_groups": (_int, [_vp, _vp, _u64, _u64, _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    "vss_search_exact_batch_filtered_groups_device": (_int, [_vp, _vp, _u64, _u64, _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    "vss_last_exact_filtered": (_int, [_vp, _vp]),
    "vss_search_batch_filtered_groups_auto": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _u64, _u64, _vp, _u64, _vp, _vp, _vp,
                                                     _vp]),
    "vss_search_batch_filtered_groups_auto_device": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _u64, _u64, _vp, _u64, _vp, _vp,
                                                            _vp, _vp]),
    "vss_last_filter_route": (_int, [_vp, _vp]),
    "vss_set_labels": (_int, [_vp, _u64, _vp, _u64]),
    "vss_set_labels_device": (_int, [_vp, _u64, _vp, _u64]),
    "vss_clear_labels": (_int, [_vp]),
    "vss_labelled_rows": (_u64, [_vp]),
    "vss_search_batch_by_label": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _int, _u64, _vp, _vp, _vp, _vp]),
    "vss_search_batch_by_label_device": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _int, _u64, _vp, _vp, _vp, _vp]),
    "vss_search_batch_by_label_range": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _int, _u64, _vp, _vp, _vp, _vp]),
    "vss_search_batch_by_label_range_device": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _int, _u64, _vp, _vp, _vp, _vp]),
    "vss_search_batch_by_label_set": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _u64, _int, _u64, _vp, _vp, _vp, _vp]),
    "vss_search_batch_by_label_set_device": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _u64, _int, _u64, _vp, _vp, _vp, _vp]),
    "vss_set_label_column": (_int, [_vp, _u32, _u64, _vp, _u64]),
    "vss_set_label_column_device": (_int, [_vp, _u32, _u64, _vp, _u64]),
    "vss_clear_label_column": (_int, [_vp, _u32]),
    "vss_label_column_rows": (_u64, [_vp, _u32]),
    "vss_search_batch_by_label_box": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _int, _u64, _vp, _vp, _vp, _vp]),
    "vss_search_batch_by_label_box_device": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _int, _u64, _vp, _vp, _vp,
                                                    _vp]),
    "vss_set_label_column64": (_int, [_vp, _u32, _u64, _vp, _u64]),
    "vss_set_label_column64_device": (_int, [_vp, _u32, _u64, _vp, _u64]),
    "vss_label_column_width": (_u32, [_vp, _u32]),
    "vss_search_batch_by_label_box64": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _int, _u64, _vp, _vp, _vp, _vp]),
    "vss_search_batch_by_label_box64_device": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _int, _u64, _vp, _vp, _vp,
                                                      _vp]),
    "vss_search_batch_by_label_set_box": (_int, [_vp, _vp, _u64, _u64, _u64, _u32, _vp, _u32, _vp, _u64, _vp, _vp, _int, _u64, _vp, _vp,
                                                 _vp, _vp]),
    "vss_search_batch_by_label_set_box_device": (_int, [_vp, _vp, _u64, _u64, _u64, _u32, _vp, _u32, _vp, _u64, _vp, _vp, _int, _u64,
                                                        _vp, _vp, _vp, _vp]),
    "vss_last_exact_fallbacks": (_u64, [_vp]),
    "vss_last_search_stats": (_int, [_vp, _vp]),
    "vss_last_search_shape": (_int, [_vp, _vp]),
    "vss_last_search_prescore": (_int, [_vp, _vp]),
    "vss_last_search_prescore_descent": (_int, [_vp, _vp]),
    "vss_last_search_query_stats": (_int, [_vp, _vp, _u64]),
    "vss_timing": (_int, [_vp, _vp, _int]),
    "vss_build_work": (_int, [_vp, _vp]),
    "vss_remove_batch": (_int, [_vp, _vp, _u64, _vp]),
    "vss_compact": (_int, [_vp]),
    "vss_compact_ex": (_int, [_vp, _int, _vp]),
    "vss_size": (_u64, [_vp]),
    "vss_nodes": (_u64, [_vp]),
    "vss_build_progress": (_int, [_vp, _vp, _vp]),
    "vss_capacity": (_u64, [_vp]),
    "vss_max_level": (_u64, [_vp]),
    "vss_memory_usage": (_u64, [_vp]),
    "vss_dimensions": (_u64, [_vp]),
    "vss_metric": (_int, [_vp]),
    "vss_level_stats": (_int, [_vp, _u64, _vp]),
    "vss_serialized_length": (_u64, [_vp]),
    "vss_save": (_int, [_vp, WRITE_CB, _vp]),
    "vss_load": (_int, [_vp, READ_CB, _vp]),
    "vss_distance_batch": (_int, [_int, _vp, _vp, _int, _u64, _u64, _vp, _int]),
    "vss_distance_batch_device": (_int, [_int, _vp, _vp, _int, _u64, _u64, _vp, _vp]),
    "vss_merge_topk_device": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp]),
    "vss_packed_block_bytes": (_u64, [_u64, _u64]),
    "vss_merge_topk_packed_device": (_int, [_vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp]),
    "vss_exchange_available": (_int, []),
    "vss_exchange_last_error": (C.c_char_p, []),
    "vss_exchange_unique_id": (_int, [_vp]),
    "vss_exchange_init_rank": (_int, [C.POINTER(_vp), _int, _vp, _int, _int]),
    "vss_exchange_init_all": (_int, [C.POINTER(_vp), _int, C.POINTER(_int)]),
    "vss_exchange_adopt": (_int, [C.POINTER(_vp), _vp, _int, _int]),
    "vss_exchange_ranks": (_int, [_vp]),
    "vss_exchange_allgather": (_int, [_vp, _vp, _vp, _u64, _vp]),
    "vss_exchange_group_begin": (_int, []),
    "vss_exchange_group_end": (_int, []),
    "vss_exchange_destroy": (_int, [_vp]),
}

_lib = None


def load_library():
    """Load the in-tree libvssgpu.so (building it first if sources are newer). Raises if it cannot be loaded."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build_library()
        try:
            # torch ships its own libamdhip64.so.7; whichever HIP runtime is loaded first serves the whole process, and
            # torch cannot initialise on top of the system one.  Import it first so both share torch's runtime.
            import torch  # noqa: F401
        except Exception:
            pass
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if hasattr(lib, "vss_debug_phase_ticks"):
            lib.vss_debug_phase_ticks.restype = _int
            lib.vss_debug_phase_ticks.argtypes = [_vp, _vp, _u64]
        _lib = lib
    return _lib


def _p(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a  # raw device pointer (int)


class VssError(RuntimeError):
    pass


class LabelPredicateStruct(C.Structure):
    """vss_label_predicate of include/vssgpu.h"""
    _fields_ = [("kind", _int), ("set_column", _u32), ("set_width", _u32), ("n_columns", _u32), ("columns", _u32 * 4),
                ("d_want", _vp), ("d_sets", _vp), ("d_lo", _vp), ("d_hi", _vp)]


class LabelPredicate:
    """One batch's label predicate for search_by_label_begin / search_multi_by_label_begin: the kind and what the kind's blocking
    _device call takes.  The per-query words are device tensors (anything with data_ptr()) or raw device addresses; the object
    keeps the tensors alive, and `c` is the ctypes struct."""
    KINDS = {"eq": 0, "range": 1, "set": 2, "box": 3, "box64": 4, "set_box": 5}

    def __init__(self, kind, want=None, lo=None, hi=None, sets=None, set_width=0, columns=(), set_column=0):
        self.kind = kind
        self.keep = (want, lo, hi, sets)
        columns = [int(c) for c in columns]
        if len(columns) > 4:
            raise ValueError("at most 4 label columns, got %d" % len(columns))
        self.c = LabelPredicateStruct(self.KINDS.get(kind, kind), set_column, set_width, len(columns),
                                      (_u32 * 4)(*columns), *[self._address(t) for t in (want, sets, lo, hi)])

    @staticmethod
    def _address(t):
        if t is None:
            return None
        return int(t.data_ptr()) if hasattr(t, "data_ptr") else (int(t) or None)

    @classmethod
    def eq(cls, want):
        return cls("eq", want=want)

    @classmethod
    def range(cls, lo, hi):
        return cls("range", lo=lo, hi=hi)

    @classmethod
    def set(cls, sets, width):
        return cls("set", sets=sets, set_width=width)

    @classmethod
    def box(cls, columns, lo, hi):
        return cls("box", columns=columns, lo=lo, hi=hi)

    @classmethod
    def box64(cls, columns, lo, hi):
        return cls("box64", columns=columns, lo=lo, hi=hi)

    @classmethod
    def set_box(cls, set_column, sets, width, columns=(), lo=None, hi=None):
        return cls("set_box", set_column=set_column, sets=sets, set_width=width, columns=columns, lo=lo, hi=hi)


class GpuIndex:
    """One HNSW index resident on one MI355X (same call shapes as the reference's HNSWIndex uses on usearch)."""

    def __init__(self, dim, metric="l2sq", M=16, M0=None, ef_construction=128, ef_search=64, device=0):
        self.lib = load_library()
        self.dim, self.metric = dim, metric
        self.M, self.M0 = M, (2 * M if M0 is None else M0)
        h = _vp()
        rc = self.lib.vss_create(dim, METRICS[metric], self.M, self.M0, ef_construction, ef_search, device, C.byref(h))
        if rc != 0 or not h.value:
            raise VssError("vss_create failed: no MI355X / HIP device %d available (the engine has no CPU fallback)" % device)
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.vss_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise VssError(self.lib.vss_last_error(self.h).decode())

    # ---- build
    def reserve(self, members, threads=1):
        self._check(self.lib.vss_reserve(self.h, members, threads))

    def set_build_params(self, max_batch, growth_div):
        self._check(self.lib.vss_set_build_params(self.h, max_batch, growth_div))

    def set_build_reorder(self, on=True):
        self._check(self.lib.vss_set_build_reorder(self.h, 1 if on else 0))

    def set_stream(self, stream_ptr):
        self._check(self.lib.vss_set_stream(self.h, stream_ptr))

    def stage(self, rowids, vecs, validity=None):
        rowids = np.ascontiguousarray(rowids, dtype=np.int64)
        vecs = np.ascontiguousarray(vecs, dtype=np.float32)
        if validity is not None:
            validity = np.ascontiguousarray(validity, dtype=np.uint64)
        self._check(self.lib.vss_stage_batch(self.h, _p(rowids), _p(vecs), _p(validity), len(rowids)))

    def stage_device(self, d_rowids, d_vecs, count):
        self._check(self.lib.vss_stage_batch_device(self.h, d_rowids, d_vecs, count))

    def build_finalize(self):
        self._check(self.lib.vss_build_finalize(self.h))

    def add(self, rowids, vecs, validity=None):
        rowids = np.ascontiguousarray(rowids, dtype=np.int64)
        vecs = np.ascontiguousarray(vecs, dtype=np.float32)
        if validity is not None:
            validity = np.ascontiguousarray(validity, dtype=np.uint64)
        self._check(self.lib.vss_add_batch(self.h, _p(rowids), _p(vecs), _p(validity), len(rowids)))

    # ---- search
    # ---- tuning (vss_set_option: results never depend on any of these; tests and A/B measurements only)
    def set_option(self, name, value):
        self._check(self.lib.vss_set_option(self.h, name.encode(), int(value)))

    def set_search_params(self, waves=16, walkers=0):
        self.set_option("search.walkers", 0)  # (so that any waves / walkers pair can be reached in two steps)
        self.set_option("search.waves", waves)
        self.set_option("search.walkers", walkers)

    def set_search_solo(self, mode=1, max_queries=0):
        self.set_option("search.solo", mode)
        if max_queries:
            self.set_option("search.solo_max_queries", max_queries)

    def set_search_team(self, on=True):
        self.set_option("search.team", int(bool(on)))

    def set_search_crew(self, on=True):
        self.set_option("search.crew", int(on))

    def set_search_pipelined(self, on=True):
        self.set_option("search.pipelined", int(bool(on)))

    def set_search_wide_lists(self, on=True):
        self.set_option("search.wide_lists", int(bool(on)))

    def set_search_visited_set(self, compact=True, lds_table_log2_max=0, cells_per_limit=0, retry_in_place=True):
        self.set_option("search.visited_compact", int(bool(compact)))
        self.set_option("search.visited_lds_log2_max", lds_table_log2_max)
        self.set_option("search.visited_cells_per_limit", cells_per_limit)
        self.set_option("search.retry_in_place", int(bool(retry_in_place)))

    def set_search_probe_wait(self, flag_wait=True):
        self.set_option("search.probe_flag_wait", int(bool(flag_wait)))

    def set_search_lookahead(self, max_active_walkers=2):
        self.set_option("search.lookahead", max_active_walkers)

    def search(self, q, k, ef=0):
        """vss_search: ONE query (HNSW_INDEX_SCAN).  Kept lean: this wrapper's own microseconds count against the call."""
        if not (type(q) is np.ndarray and q.dtype == np.float32 and q.flags.c_contiguous):
            q = np.ascontiguousarray(q, dtype=np.float32)
        out = np.empty(k, dtype=np.int64)  # the engine writes every cell (unused ones = -1)
        n = _u64(0)
        rc = self.lib.vss_search(self.h, q.ctypes.data, k, ef, out.ctypes.data, C.byref(n))
        if rc != 0:
            self._check(rc)
        return out[:n.value]

    def search_batch(self, Q, k, ef=0, exact=False):
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        nq = len(Q)
        keys = np.full((nq, k), -1, dtype=np.int64)
        d = np.full((nq, k), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        if exact:
            self._check(self.lib.vss_search_exact_batch(self.h, _p(Q), nq, k, _p(keys), _p(d), _p(cnt)))
        else:
            self._check(self.lib.vss_search_batch(self.h, _p(Q), nq, k, ef, _p(keys), _p(d), _p(cnt)))
        return keys, d, cnt

    def search_batch_filtered(self, Q, k, ef, allowed_bitmap, n_bits):
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        allowed_bitmap = np.ascontiguousarray(allowed_bitmap, dtype=np.uint64)
        nq = len(Q)
        keys = np.full((nq, k), -1, dtype=np.int64)
        d = np.full((nq, k), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        self._check(self.lib.vss_search_batch_filtered(self.h, _p(Q), nq, k, ef, _p(allowed_bitmap), n_bits, _p(keys), _p(d),
                                                       _p(cnt)))
        return keys, d, cnt

    def search_batch_filtered_groups(self, Q, k, ef, bitmaps, n_bits, group_of):
        """vss_search_batch_filtered_groups: query q is filtered by row `group_of[q]` of `bitmaps`, an
        n_groups x ((n_bits + 63) // 64) uint64 array of row-id bitmaps — one launch for a chunk of per-query predicates."""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        bitmaps = np.ascontiguousarray(bitmaps, dtype=np.uint64)
        words = (n_bits + 63) // 64
        if bitmaps.ndim != 2 or bitmaps.shape[1] != words:
            raise ValueError("bitmaps must be n_groups x %d uint64 words for %d bits, got shape %r"
                             % (words, n_bits, bitmaps.shape))
        group_of = np.ascontiguousarray(group_of, dtype=np.uint32)
        nq = len(Q)
        if group_of.shape != (nq,):
            raise ValueError("group_of must name one group per query: %d queries, shape %r" % (nq, group_of.shape))
        keys = np.full((nq, k), -1, dtype=np.int64)
        d = np.full((nq, k), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        self._check(self.lib.vss_search_batch_filtered_groups(self.h, _p(Q), nq, k, ef, _p(bitmaps), len(bitmaps), n_bits,
                                                              _p(group_of), _p(keys), _p(d), _p(cnt)))
        return keys, d, cnt

    def search_batch_filtered_groups_device(self, d_Q, nq, k, ef, d_bitmaps, n_groups, n_bits, d_group_of, d_keys, d_dist,
                                            d_counts):
        """The same over raw device pointers (the caller keeps the tensors alive); blocking."""
        self._check(self.lib.vss_search_batch_filtered_groups_device(self.h, d_Q, nq, k, ef, d_bitmaps, n_groups, n_bits,
                                                                     d_group_of, d_keys, d_dist, d_counts))

    def search_exact_batch_filtered_groups(self, Q, k, bitmaps, n_bits, group_of=None):
        """vss_search_exact_batch_filtered_groups: the exact top-k of query q among the live rows that row `group_of[q]` of
        `bitmaps` admits (group_of=None: every query takes row 0), scoring the admitted rows only."""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        bitmaps = np.ascontiguousarray(bitmaps, dtype=np.uint64)
        words = (n_bits + 63) // 64
        if bitmaps.ndim != 2 or bitmaps.shape[1] != words:
            raise ValueError("bitmaps must be n_groups x %d uint64 words for %d bits, got shape %r"
                             % (words, n_bits, bitmaps.shape))
        nq = len(Q)
        if group_of is not None:
            group_of = np.ascontiguousarray(group_of, dtype=np.uint32)
            if group_of.shape != (nq,):
                raise ValueError("group_of must name one group per query: %d queries, shape %r" % (nq, group_of.shape))
        keys = np.full((nq, k), -1, dtype=np.int64)
        d = np.full((nq, k), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        self._check(self.lib.vss_search_exact_batch_filtered_groups(self.h, _p(Q), nq, k, _p(bitmaps), len(bitmaps), n_bits,
                                                                    _p(group_of), _p(keys), _p(d), _p(cnt)))
        return keys, d, cnt

    def search_exact_batch_filtered_groups_device(self, d_Q, nq, k, d_bitmaps, n_groups, n_bits, d_group_of, d_keys, d_dist,
                                                  d_counts):
        """The same over raw device pointers (d_group_of may be None); blocking."""
        self._check(self.lib.vss_search_exact_batch_filtered_groups_device(self.h, d_Q, nq, k, d_bitmaps, n_groups, n_bits,
                                                                           d_group_of, d_keys, d_dist, d_counts))

    def last_exact_filtered(self):
        """[admitted rows listed over the groups that had queries, (query, row) distances computed, passes, bytes of list
        scratch held] of the last search_exact_batch_filtered_groups call."""
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.vss_last_exact_filtered(self.h, _p(out)))
        return out

    def search_batch_filtered_groups_auto(self, Q, k, ef, bitmaps, n_bits, group_of=None, route_c=0):
        """vss_search_batch_filtered_groups_auto: every group answered by the cheaper of search_batch_filtered_groups and
        search_exact_batch_filtered_groups, decided from its count of live admitted rows (route_c=0: the default constant).
        Returns (ids, distances, counts, route); route[q] is 0 (graph) or 1 (exact)."""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        bitmaps = np.ascontiguousarray(bitmaps, dtype=np.uint64)
        words = (n_bits + 63) // 64
        if bitmaps.ndim != 2 or bitmaps.shape[1] != words:
            raise ValueError("bitmaps must be n_groups x %d uint64 words for %d bits, got shape %r"
                             % (words, n_bits, bitmaps.shape))
        nq = len(Q)
        if group_of is not None:
            group_of = np.ascontiguousarray(group_of, dtype=np.uint32)
            if group_of.shape != (nq,):
                raise ValueError("group_of must name one group per query: %d queries, shape %r" % (nq, group_of.shape))
        keys = np.full((nq, k), -1, dtype=np.int64)
        d = np.full((nq, k), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        route = np.zeros(nq, dtype=np.uint8)
        self._check(self.lib.vss_search_batch_filtered_groups_auto(self.h, _p(Q), nq, k, ef, _p(bitmaps), len(bitmaps), n_bits,
                                                                   _p(group_of), route_c, _p(keys), _p(d), _p(cnt), _p(route)))
        return keys, d, cnt, route

    def search_batch_filtered_groups_auto_device(self, d_Q, nq, k, ef, d_bitmaps, n_groups, n_bits, d_group_of, d_keys, d_dist,
                                                 d_counts, d_route=None, route_c=0):
        """The same over raw device pointers (d_group_of, d_dist and d_route may be None); blocking."""
        self._check(self.lib.vss_search_batch_filtered_groups_auto_device(self.h, d_Q, nq, k, ef, d_bitmaps, n_groups, n_bits,
                                                                          d_group_of, route_c, d_keys, d_dist, d_counts, d_route))

    def last_filter_route(self):
        """[queries routed graph, queries routed exact, groups in use routed graph, groups in use routed exact, L, C, limit, 0]
        of the last search_batch_filtered_groups_auto call."""
        out = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.vss_last_filter_route(self.h, _p(out)))
        return out

    # ---- the label column (include/vssgpu.h, "Equality predicates on a resident label column")
    NO_LABEL = 0xFFFFFFFF
    BY_LABEL_MODES = {"graph": 0, "exact": 1, "auto": 2}

    def set_labels(self, first_rowid, labels):
        """vss_set_labels: cells first_rowid .. first_rowid + len(labels) - 1 of the per-row-id label column."""
        labels = np.ascontiguousarray(labels, dtype=np.uint32)
        if labels.ndim != 1:
            raise ValueError("labels must be one uint32 per row id, got shape %r" % (labels.shape,))
        self._check(self.lib.vss_set_labels(self.h, first_rowid, _p(labels), len(labels)))

    def set_labels_device(self, first_rowid, d_labels, n):
        """The same from a raw device pointer."""
        self._check(self.lib.vss_set_labels_device(self.h, first_rowid, d_labels, n))

    def clear_labels(self):
        self._check(self.lib.vss_clear_labels(self.h))

    def labelled_rows(self):
        return int(self.lib.vss_labelled_rows(self.h))

    def search_batch_by_label(self, Q, k, ef, want, mode="auto", route_c=0):
        """vss_search_batch_by_label: query q admits the live rows whose label is want[q] (NO_LABEL wants nothing).  mode:
        "graph", "exact" or "auto" (or 0 / 1 / 2).  Returns (ids, distances, counts, route)."""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        want = np.ascontiguousarray(want, dtype=np.uint32)
        nq = len(Q)
        if want.shape != (nq,):
            raise ValueError("want must name one label per query: %d queries, shape %r" % (nq, want.shape))
        keys = np.full((nq, k), -1, dtype=np.int64)
        d = np.full((nq, k), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        route = np.zeros(nq, dtype=np.uint8)
        self._check(self.lib.vss_search_batch_by_label(self.h, _p(Q), nq, k, ef, _p(want), self.BY_LABEL_MODES.get(mode, mode),
                                                       route_c, _p(keys), _p(d), _p(cnt), _p(route)))
        return keys, d, cnt, route

    def search_batch_by_label_device(self, d_Q, nq, k, ef, d_want, d_keys, d_dist, d_counts, d_route=None, mode="auto", route_c=0):
        """The same over raw device pointers (d_dist and d_route may be None); blocking."""
        self._check(self.lib.vss_search_batch_by_label_device(self.h, d_Q, nq, k, ef, d_want, self.BY_LABEL_MODES.get(mode, mode),
                                                              route_c, d_keys, d_dist, d_counts, d_route))

    def search_batch_by_label_range(self, Q, k, ef, lo, hi, mode="auto", route_c=0):
        """vss_search_batch_by_label_range: query q admits the live rows whose label lies in [lo[q], hi[q]], both ends inclusive,
        unsigned (lo > hi admits nothing, hi = NO_LABEL is no upper bound, a NO_LABEL cell is in no range).  mode as for
        search_batch_by_label.  Returns (ids, distances, counts, route)."""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        lo = np.ascontiguousarray(lo, dtype=np.uint32)
        hi = np.ascontiguousarray(hi, dtype=np.uint32)
        nq = len(Q)
        if lo.shape != (nq,) or hi.shape != (nq,):
            raise ValueError("lo and hi must name one range per query: %d queries, shapes %r and %r" % (nq, lo.shape, hi.shape))
        keys = np.full((nq, k), -1, dtype=np.int64)
        d = np.full((nq, k), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        route = np.zeros(nq, dtype=np.uint8)
        self._check(self.lib.vss_search_batch_by_label_range(self.h, _p(Q), nq, k, ef, _p(lo), _p(hi),
                                                             self.BY_LABEL_MODES.get(mode, mode), route_c, _p(keys), _p(d), _p(cnt),
                                                             _p(route)))
        return keys, d, cnt, route

    def search_batch_by_label_range_device(self, d_Q, nq, k, ef, d_lo, d_hi, d_keys, d_dist, d_counts, d_route=None, mode="auto",
                                           route_c=0):
        """The same over raw device pointers (d_dist and d_route may be None); blocking."""
        self._check(self.lib.vss_search_batch_by_label_range_device(self.h, d_Q, nq, k, ef, d_lo, d_hi,
                                                                    self.BY_LABEL_MODES.get(mode, mode), route_c, d_keys, d_dist,
                                                                    d_counts, d_route))

    LABEL_COLUMNS_MAX = 4  # VSS_LABEL_COLUMNS_MAX

    def set_label_column(self, column, first_rowid, labels):
        """vss_set_label_column: cells first_rowid .. first_rowid + len(labels) - 1 of label column `column` (0 .. 3; column 0 is
        the column of set_labels)."""
        labels = np.ascontiguousarray(labels, dtype=np.uint32)
        if labels.ndim != 1:
            raise ValueError("labels must be one uint32 per row id, got shape %r" % (labels.shape,))
        self._check(self.lib.vss_set_label_column(self.h, column, first_rowid, _p(labels), len(labels)))

    def set_label_column_device(self, column, first_rowid, d_labels, n):
        """The same from a raw device pointer."""
        self._check(self.lib.vss_set_label_column_device(self.h, column, first_rowid, d_labels, n))

    def clear_label_column(self, column):
        self._check(self.lib.vss_clear_label_column(self.h, column))

    def label_column_rows(self, column):
        return int(self.lib.vss_label_column_rows(self.h, column))

    def search_batch_by_label_box(self, Q, k, ef, columns, lo, hi, mode="auto", route_c=0):
        """vss_search_batch_by_label_box: `columns` names 1 .. LABEL_COLUMNS_MAX distinct label columns for the whole call, and
        query q admits the live rows whose cell in columns[j] lies in [lo[q, j], hi[q, j]] for EVERY j (both ends inclusive,
        unsigned; any lo > hi empties the box, hi = NO_LABEL is no upper bound, a NO_LABEL cell or a row beyond a named column
        is in no box).  lo and hi are nq x len(columns) matrices.  mode as for search_batch_by_label.  Returns (ids, distances,
        counts, route)."""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        columns = np.ascontiguousarray(columns, dtype=np.uint32)
        lo = np.ascontiguousarray(lo, dtype=np.uint32)
        hi = np.ascontiguousarray(hi, dtype=np.uint32)
        nq = len(Q)
        if columns.ndim != 1:
            raise ValueError("columns must be a list of column numbers, got shape %r" % (columns.shape,))
        if lo.shape != (nq, len(columns)) or hi.shape != (nq, len(columns)):
            raise ValueError("lo and hi must hold one range per query and named column: %d queries x %d columns, shapes %r and %r"
                             % (nq, len(columns), lo.shape, hi.shape))
        keys = np.full((nq, k), -1, dtype=np.int64)
        d = np.full((nq, k), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        route = np.zeros(nq, dtype=np.uint8)
        self._check(self.lib.vss_search_batch_by_label_box(self.h, _p(Q), nq, k, ef, _p(columns), len(columns), _p(lo), _p(hi),
                                                           self.BY_LABEL_MODES.get(mode, mode), route_c, _p(keys), _p(d), _p(cnt),
                                                           _p(route)))
        return keys, d, cnt, route

    def search_batch_by_label_box_device(self, d_Q, nq, k, ef, columns, d_lo, d_hi, d_keys, d_dist, d_counts, d_route=None,
                                         mode="auto", route_c=0):
        """The same over raw device pointers (`columns` stays a host sequence; d_lo and d_hi: nq x len(columns) words, row-major;
        d_dist and d_route may be None); blocking."""
        columns = np.ascontiguousarray(columns, dtype=np.uint32)
        self._check(self.lib.vss_search_batch_by_label_box_device(self.h, d_Q, nq, k, ef, _p(columns), len(columns), d_lo, d_hi,
                                                                  self.BY_LABEL_MODES.get(mode, mode), route_c, d_keys, d_dist,
                                                                  d_counts, d_route))

    NO_LABEL64 = 0xFFFFFFFFFFFFFFFF  # VSS_NO_LABEL64

    def set_label_column64(self, column, first_rowid, labels):
        """vss_set_label_column64: the same with 64-bit cells (NO_LABEL64 is the NULL cell).  The column must be empty or 64 bits
        wide already; clear_label_column forgets a column's width."""
        labels = np.ascontiguousarray(labels, dtype=np.uint64)
        if labels.ndim != 1:
            raise ValueError("labels must be one uint64 per row id, got shape %r" % (labels.shape,))
        self._check(self.lib.vss_set_label_column64(self.h, column, first_rowid, _p(labels), len(labels)))

    def set_label_column64_device(self, column, first_rowid, d_labels, n):
        """The same from a raw device pointer."""
        self._check(self.lib.vss_set_label_column64_device(self.h, column, first_rowid, d_labels, n))

    def label_column_width(self, column):
        """0 (no cells), 32 or 64."""
        return int(self.lib.vss_label_column_width(self.h, column))

    def search_batch_by_label_box64(self, Q, k, ef, columns, lo, hi, mode="auto", route_c=0):
        """vss_search_batch_by_label_box64: search_batch_by_label_box with 64-bit ends; the named columns may be 32 or 64 bits
        wide, mixed (a 32-bit cell is read zero-extended, NO_LABEL as NO_LABEL64).  hi = NO_LABEL64 is no upper bound.  lo and
        hi are nq x len(columns) matrices of uint64.  Returns (ids, distances, counts, route)."""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        columns = np.ascontiguousarray(columns, dtype=np.uint32)
        lo = np.ascontiguousarray(lo, dtype=np.uint64)
        hi = np.ascontiguousarray(hi, dtype=np.uint64)
        nq = len(Q)
        if columns.ndim != 1:
            raise ValueError("columns must be a list of column numbers, got shape %r" % (columns.shape,))
        if lo.shape != (nq, len(columns)) or hi.shape != (nq, len(columns)):
            raise ValueError("lo and hi must hold one range per query and named column: %d queries x %d columns, shapes %r and %r"
                             % (nq, len(columns), lo.shape, hi.shape))
        keys = np.full((nq, k), -1, dtype=np.int64)
        d = np.full((nq, k), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        route = np.zeros(nq, dtype=np.uint8)
        self._check(self.lib.vss_search_batch_by_label_box64(self.h, _p(Q), nq, k, ef, _p(columns), len(columns), _p(lo), _p(hi),
                                                             self.BY_LABEL_MODES.get(mode, mode), route_c, _p(keys), _p(d),
                                                             _p(cnt), _p(route)))
        return keys, d, cnt, route

    def search_batch_by_label_box64_device(self, d_Q, nq, k, ef, columns, d_lo, d_hi, d_keys, d_dist, d_counts, d_route=None,
                                           mode="auto", route_c=0):
        """The same over raw device pointers (`columns` stays a host sequence; d_lo and d_hi: nq x len(columns) uint64,
        row-major; d_dist and d_route may be None); blocking."""
        columns = np.ascontiguousarray(columns, dtype=np.uint32)
        self._check(self.lib.vss_search_batch_by_label_box64_device(self.h, d_Q, nq, k, ef, _p(columns), len(columns), d_lo, d_hi,
                                                                    self.BY_LABEL_MODES.get(mode, mode), route_c, d_keys, d_dist,
                                                                    d_counts, d_route))

    def search_batch_by_label_set_box(self, Q, k, ef, set_column, sets, columns=(), lo=None, hi=None, mode="auto", route_c=0):
        """vss_search_batch_by_label_set_box: query q admits the rows whose cell in `set_column` is one of the uint64 words of
        sets[q] (NO_LABEL64 pads a shorter list) and whose cells in the range `columns` (0 to 3 of them) lie within lo[q] .. hi[q];
        columns of either width, mixed.  sets: nq x width; lo and hi: nq x len(columns) matrices of uint64 (not needed without
        range columns).  Returns (ids, distances, counts, route)."""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        nq = len(Q)
        sets = np.ascontiguousarray(sets, dtype=np.uint64)
        columns = np.ascontiguousarray(columns, dtype=np.uint32)
        if sets.ndim != 2 or sets.shape[0] != nq:
            raise ValueError("sets must hold one row of uint64 words per query: %d queries, shape %r" % (nq, sets.shape))
        if columns.ndim != 1:
            raise ValueError("columns must be a list of column numbers, got shape %r" % (columns.shape,))
        m = len(columns)
        if m:
            lo = np.ascontiguousarray(lo, dtype=np.uint64)
            hi = np.ascontiguousarray(hi, dtype=np.uint64)
            if lo.shape != (nq, m) or hi.shape != (nq, m):
                raise ValueError("lo and hi must hold one range per query and range column: %d queries x %d columns, shapes %r and "
                                 "%r" % (nq, m, lo.shape, hi.shape))
        keys = np.full((nq, k), -1, dtype=np.int64)
        d = np.full((nq, k), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        route = np.zeros(nq, dtype=np.uint8)
        self._check(self.lib.vss_search_batch_by_label_set_box(self.h, _p(Q), nq, k, ef, set_column, _p(sets), sets.shape[1],
                                                               _p(columns) if m else None, m, _p(lo) if m else None,
                                                               _p(hi) if m else None, self.BY_LABEL_MODES.get(mode, mode), route_c,
                                                               _p(keys), _p(d), _p(cnt), _p(route)))
        return keys, d, cnt, route

    def search_batch_by_label_set_box_device(self, d_Q, nq, k, ef, set_column, d_sets, width, columns, d_lo, d_hi, d_keys, d_dist,
                                             d_counts, d_route=None, mode="auto", route_c=0):
        """The same over raw device pointers (`columns` stays a host sequence; d_sets: nq x width uint64, d_lo and d_hi: nq x
        len(columns) uint64, row-major, None without range columns; d_dist and d_route may be None); blocking."""
        columns = np.ascontiguousarray(columns, dtype=np.uint32)
        m = len(columns)
        self._check(self.lib.vss_search_batch_by_label_set_box_device(self.h, d_Q, nq, k, ef, set_column, d_sets, width,
                                                                      _p(columns) if m else None, m, d_lo, d_hi,
                                                                      self.BY_LABEL_MODES.get(mode, mode), route_c, d_keys, d_dist,
                                                                      d_counts, d_route))

    LABEL_SET_MAX = 32  # VSS_LABEL_SET_MAX

    @staticmethod
    def label_set_matrix(sets, nq):
        """The nq x width uint32 matrix of a call by label set: `sets` as it is where it is one already, or a list of per-query
        sequences padded with NO_LABEL to the longest (to width 1 where every one is empty)."""
        if not isinstance(sets, np.ndarray):
            rows = [np.asarray(r, dtype=np.uint32).reshape(-1) for r in sets]
            width = max([len(r) for r in rows] + [1])
            sets = np.full((len(rows), width), GpuIndex.NO_LABEL, dtype=np.uint32)
            for q, r in enumerate(rows):
                sets[q, :len(r)] = r
        sets = np.ascontiguousarray(sets, dtype=np.uint32)
        if sets.ndim != 2 or sets.shape[0] != nq:
            raise ValueError("sets must be one row of labels per query: %d queries, shape %r" % (nq, sets.shape))
        return sets

    def search_batch_by_label_set(self, Q, k, ef, sets, mode="auto", route_c=0):
        """vss_search_batch_by_label_set: query q admits the live rows whose label is one of sets[q] (an nq x width uint32 matrix,
        width 1 .. LABEL_SET_MAX, NO_LABEL pads a shorter list and equals nothing; or a list of per-query sequences, padded
        here).  mode as for search_batch_by_label.  Returns (ids, distances, counts, route)."""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        nq = len(Q)
        sets = self.label_set_matrix(sets, nq)
        keys = np.full((nq, k), -1, dtype=np.int64)
        d = np.full((nq, k), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        route = np.zeros(nq, dtype=np.uint8)
        self._check(self.lib.vss_search_batch_by_label_set(self.h, _p(Q), nq, k, ef, _p(sets), sets.shape[1],
                                                           self.BY_LABEL_MODES.get(mode, mode), route_c, _p(keys), _p(d), _p(cnt),
                                                           _p(route)))
        return keys, d, cnt, route

    def search_batch_by_label_set_device(self, d_Q, nq, k, ef, d_sets, width, d_keys, d_dist, d_counts, d_route=None, mode="auto",
                                         route_c=0):
        """The same over raw device pointers (d_sets: nq x width words, row-major; d_dist and d_route may be None); blocking."""
        self._check(self.lib.vss_search_batch_by_label_set_device(self.h, d_Q, nq, k, ef, d_sets, width,
                                                                  self.BY_LABEL_MODES.get(mode, mode), route_c, d_keys, d_dist,
                                                                  d_counts, d_route))

    def search_batch_device(self, d_Q, nq, k, ef, d_keys, d_dist, d_counts, exact=False):
        if exact:
            self._check(self.lib.vss_search_exact_batch_device(self.h, d_Q, nq, k, d_keys, d_dist, d_counts))
        else:
            self._check(self.lib.vss_search_batch_device(self.h, d_Q, nq, k, ef, d_keys, d_dist, d_counts))

    def search_begin(self, context, d_Q, nq, k, ef, d_keys, d_dist, d_counts):
        self._check(self.lib.vss_search_batch_device_begin(self.h, context, d_Q, nq, k, ef, d_keys, d_dist, d_counts))

    def search_multi_begin(self, context, d_Qs, per_batch, k, ef, d_keys, d_dists, d_counts):
        """Several batches (lists of device pointers, one entry per batch) answered by one launch; search_end completes."""
        n = len(d_Qs)
        tables = [(C.c_void_p * n)(*[int(p) if p else None for p in t]) for t in (d_Qs, d_keys, d_dists, d_counts)]
        self._check(self.lib.vss_search_multi_device_begin(self.h, context, n, tables[0], per_batch, k, ef, tables[1], tables[2],
                                                           tables[3]))

    def search_filtered_begin(self, context, d_Q, nq, k, ef, d_bitmap, n_bits, d_keys, d_dist, d_counts):
        """search_begin under one row-id bitmap (a device address); the bitmap stays untouched until search_end returns."""
        self._check(self.lib.vss_search_batch_filtered_device_begin(self.h, context, d_Q, nq, k, ef, d_bitmap, n_bits, d_keys,
                                                                    d_dist, d_counts))

    def search_filtered_groups_begin(self, context, d_Q, nq, k, ef, d_bitmaps, n_groups, n_bits, d_group_of, d_keys, d_dist,
                                     d_counts):
        """search_begin with one predicate per query: query q takes bitmap d_group_of[q] of the table d_bitmaps."""
        self._check(self.lib.vss_search_batch_filtered_groups_device_begin(self.h, context, d_Q, nq, k, ef, d_bitmaps, n_groups,
                                                                           n_bits, d_group_of, d_keys, d_dist, d_counts))

    def search_multi_filtered_begin(self, context, d_Qs, per_batch, k, ef, d_bitmaps, n_groups, n_bits, d_group_ofs, d_keys,
                                    d_dists, d_counts):
        """search_multi_begin where batch b has its own table d_bitmaps[b] of n_groups[b] bitmaps and its own group numbers
        d_group_ofs[b] (None: every query of the batch takes bitmap 0).  Lists of device addresses, one entry per batch."""
        n = len(d_Qs)
        tables = [(C.c_void_p * n)(*[int(p) if p else None for p in t]) if t is not None else None
                  for t in (d_Qs, d_bitmaps, d_group_ofs, d_keys, d_dists, d_counts)]
        groups = (C.c_uint64 * n)(*[int(g) for g in n_groups]) if n_groups is not None else None
        self._check(self.lib.vss_search_multi_filtered_device_begin(self.h, context, n, tables[0], per_batch, k, ef, tables[1],
                                                                    groups, n_bits, tables[2], tables[3], tables[4], tables[5]))

    def search_by_label_begin(self, context, d_Q, nq, k, ef, predicate, d_keys, d_dist, d_counts):
        """search_begin under one label predicate per query (a LabelPredicate over device tensors or addresses): the walk of the
        form's blocking _device call in mode graph, on the caller's context; search_end completes.  The predicate's device
        memory stays untouched until then."""
        self._check(self.lib.vss_search_by_label_device_begin(self.h, context, d_Q, nq, k, ef, C.byref(predicate.c), d_keys, d_dist,
                                                              d_counts))

    def search_multi_by_label_begin(self, context, d_Qs, per_batch, k, ef, predicates, d_keys, d_dists, d_counts):
        """search_multi_begin where batch b brings predicates[b] (LabelPredicate): all of one kind, over the same columns, of the
        same set width.  Lists with one entry per batch; d_dists[b] may be None."""
        n = len(d_Qs)
        for name, t in (("predicates", predicates), ("d_keys", d_keys), ("d_dists", d_dists), ("d_counts", d_counts)):
            if t is not None and len(t) != n:
                raise ValueError("%s has %d entries for %d batches" % (name, len(t), n))
        tables = [(C.c_void_p * n)(*[int(p) if p else None for p in t]) if t is not None else None
                  for t in (d_Qs, d_keys, d_dists, d_counts)]
        preds =(LabelPredicateStruct * len(predicates))(*[p.c for p in predicates]) if predicates is not None else None
        self._check(self.lib.vss_search_multi_by_label_device_begin(self.h, context, n, tables[0], per_batch, k, ef, preds, tables[1],
                                                                    tables[2], tables[3]))

    def set_search_gating(self, on):
        self.set_option("search.gating", 1 if on else 0)

    def search_end(self, context):
        self._check(self.lib.vss_search_batch_end(self.h, context))

    def last_search_stats(self):
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.vss_last_search_stats(self.h, _p(out)))
        return out

    def last_search_shape(self):
        """[threads, walkers, workgroups, LDS bytes, list placement (0 registers, 1 LDS, 2 HBM), visited-set placement
        (0 LDS, 1 LDS compact, 2 HBM), solo, 0] of the last search call's launch."""
        out = np.zeros(8, dtype=np.uint32)
        self._check(self.lib.vss_last_search_shape(self.h, _p(out)))
        return out

    def last_search_prescore(self):
        """[filter active in the last search call's first launch, rows pre-scored on their codes, rows rejected there, bytes of
        row codes held] (search.prescore)."""
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.vss_last_search_prescore(self.h, _p(out)))
        return out

    def last_search_prescore_descent(self):
        """[rows the greedy descent handed over with a finite bound, rows among them rejected on their codes] of the last
        search call (search.prescore_descent)."""
        out = np.zeros(2, dtype=np.uint64)
        self._check(self.lib.vss_last_search_prescore_descent(self.h, _p(out)))
        return out

    def last_exact_fallbacks(self):
        """Queries of the last exact search that were answered again by brute force in the metric (their selection by ranking
        score could not be certified, csrc/exact_certificate.h)."""
        return int(self.lib.vss_last_exact_fallbacks(self.h))

    def timing(self, reset=False):
        out = np.zeros(6, dtype=np.float64)
        self._check(self.lib.vss_timing(self.h, _p(out), int(reset)))
        return dict(search_kernel_ms=out[0], build_phase_a_ms=out[1], build_phase_b_ms=out[2], build_wall_ms=out[3],
                    build_batches=int(out[4]), build_retries=int(out[5]))

    def build_work(self):
        out = np.zeros(3, dtype=np.uint64)
        self._check(self.lib.vss_build_work(self.h, _p(out)))
        return dict(insert_distances=int(out[0]), insert_expansions=int(out[1]), link_distances=int(out[2]))

    def last_query_stats(self, nq):
        out = np.zeros((nq, 2), dtype=np.uint32)
        self._check(self.lib.vss_last_search_query_stats(self.h, _p(out), nq))
        return out

    # ---- maintenance
    def remove(self, rowids):
        rowids = np.ascontiguousarray(rowids, dtype=np.int64)
        n = _u64(0)
        self._check(self.lib.vss_remove_batch(self.h, _p(rowids), len(rowids), C.byref(n)))
        return n.value

    def compact(self, reorder=True):
        """vss_compact: drop tombstones + the reference's (level, cluster) reordering; reorder=False only prunes.
        Returns True if the rows were reordered."""
        done = C.c_int(0)
        self._check(self.lib.vss_compact_ex(self.h, 1 if reorder else 0, C.byref(done)))
        return bool(done.value)

    def size(self):
        return self.lib.vss_size(self.h)

    def nodes(self):
        return self.lib.vss_nodes(self.h)

    def capacity(self):
        return self.lib.vss_capacity(self.h)

    def max_level(self):
        return self.lib.vss_max_level(self.h)

    def build_progress(self):
        """(rows linked so far, rows of that build) — callable from another thread while build_finalize / add runs."""
        a, b = _u64(0), _u64(0)
        self.lib.vss_build_progress(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def memory_usage(self):
        return self.lib.vss_memory_usage(self.h)

    def level_stats(self, level):
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.vss_level_stats(self.h, level, _p(out)))
        return out

    # ---- persistence
    def save(self):
        chunks = []

        def write(ctx, data, size):
            chunks.append(C.string_at(data, size))
            return 1
        cb = WRITE_CB(write)
        self._check(self.lib.vss_save(self.h, cb, None))
        return b"".join(chunks)

    def serialized_length(self):
        return self.lib.vss_serialized_length(self.h)

    def save_into(self, buf):
        """Serialise into a preallocated uint8 numpy buffer (no intermediate copies; for multi-GB indexes)."""
        state = {"off": 0}
        base = buf.ctypes.data

        def write(ctx, data, size):
            if state["off"] + size > buf.nbytes:
                return 0
            C.memmove(base + state["off"], data, size)
            state["off"] += size
            return 1
        cb = WRITE_CB(write)
        self._check(self.lib.vss_save(self.h, cb, None))
        return state["off"]

    def load(self, blob):
        state = {"off": 0}

        def read(ctx, data, size):
            if state["off"] + size > len(blob):
                return 0
            C.memmove(data, blob[state["off"]:state["off"] + size], size)
            state["off"] += size
            return 1
        cb = READ_CB(read)
        self._check(self.lib.vss_load(self.h, cb, None))
        self.dim = self.lib.vss_dimensions(self.h)


def distance_batch(fn, a, b, device=0):
    """array_distance / array_cosine_distance / array_negative_inner_product over host arrays."""
    lib = load_library()
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    rows, dim = a.shape
    b_const = int(b.ndim == 1)
    out = np.zeros(rows, dtype=np.float32)
    rc = lib.vss_distance_batch(FUNCTIONS[fn], _p(a), _p(b), b_const, rows, dim, _p(out), device)
    if rc != 0:
        raise VssError("vss_distance_batch failed (no HIP device? the engine has no CPU fallback)")
    return out
