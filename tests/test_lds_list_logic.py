"""CPU tests of the candidate list kept in LDS (search limits of 513-4096): the placement rule of
duckdb-vss_amd/csrc/host_logic.h, the list's index arithmetic (duckdb-vss_amd/csrc/lds_list_index.h) as a lane-by-lane model
against std::vector, and the resources of the k_search instantiations that carry the list."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
LDS_PER_CU = 160 * 1024
LDS_LIST_E = 64  # the value of k_search's template parameter E that selects LdsList (hnsw_kernels.h)


@pytest.fixture(scope="module")
def ll():
    src = os.path.join(HERE, "lds_list_probe.cpp")
    hdrs = [os.path.join(ROOT, "duckdb-vss_amd", "csrc", h) for h in ("host_logic.h", "engine_layout.h", "visited_compact.h", "lds_list_index.h")]
    out = os.path.join(HERE, "lds_list_probe.so")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", src, "-o", out])
    lib = C.CDLL(out)
    lib.ll_model_check.restype = C.c_uint64
    for f in (lib.ll_placement, lib.ll_engine_walkers_that_fit, lib.ll_header_bytes, lib.ll_list_bytes):
        f.restype = C.c_uint32
    return lib


def align16(x):
    return (x + 15) & ~15


def slot_bytes(dim, visited_in_lds, M0=32):
    """engine_slot_bytes (engine_layout.h) without a list: [visited set of 2^13 cells][staged query][2 x (ids, distances)]"""
    V = (dim + 3) // 4
    return (4 << 13 if visited_in_lds else 0) + align16(16 * V) + 4 * align16(4 * M0)


def list_bytes(cells):
    """two arrays of `cells` words and the 64 tile tops"""
    return 2 * align16(4 * cells) + 256


def test_list_bytes_and_header(ll):
    assert ll.ll_header_bytes() == 48 + 16 * 32 + 64 * 8  # = ENGINE_HEADER_BYTES (engine_layout.h: the kernels' own)
    assert ll.ll_list_bytes(0) == 0
    for cells in (513, 514, 1536, 4095, 4096):
        assert ll.ll_list_bytes(cells) == list_bytes(cells)
    assert ll.ll_list_bytes(1536) <= 12 * 1024 + 256 and ll.ll_list_bytes(4096) == 32 * 1024 + 256


@pytest.mark.parametrize("dim", [128, 768, 1536])
@pytest.mark.parametrize("visited_in_lds", [True, False])
def test_placement_rule(ll, dim, visited_in_lds):
    header = ll.ll_header_bytes()
    slot = slot_bytes(dim, visited_in_lds)
    cap = 4  # the engine's default ceiling of walkers per workgroup
    n_lds = 0
    for wanted in (1, 2, 4):  # walkers the launch asks for (ceil(queries / compute units))
        today = max(1, min(wanted, cap, (LDS_PER_CU - header) // slot))
        assert ll.ll_engine_walkers_that_fit(slot, cap) == min(cap, (LDS_PER_CU - header) // slot)
        for cells in (512, 513, 1536, 4096, 4097):
            for solo in (0, 1):
                for mode in (0, 1, 2):
                    w = C.c_uint32(99)
                    got = ll.ll_placement(mode, cells, solo, slot, today, cap, C.byref(w))
                    fit = min(cap, (LDS_PER_CU - header) // (slot + list_bytes(cells)))
                    eligible = not solo and 513 <= cells <= 4096
                    if mode == 0 or not eligible:
                        want = 2
                    elif mode == 1:
                        want = 1 if fit >= today else 2
                    else:
                        want = 1 if fit >= 1 else 2
                    assert got == want, (dim, visited_in_lds, wanted, cells, solo, mode, got, want)
                    if got == 1:
                        n_lds += 1
                        assert 1 <= w.value <= cap and w.value == fit
                        assert w.value * (slot + list_bytes(cells)) + header <= LDS_PER_CU
                        if mode == 1:
                            assert w.value >= today  # no launch loses occupancy under the automatic rule
                    else:
                        assert w.value == 0
    assert n_lds > 0
    assert ll.ll_placement(1, 0, 0, slot, 4, cap, None) == 0  # no list in memory at all: registers


def test_placement_rule_keeps_todays_walkers_in_the_production_shape(ll):
    """768 dimensions, visited set in HBM (every limit above 512 on a large index): the largest list leaves four walkers."""
    w = C.c_uint32(0)
    assert ll.ll_placement(1, 4096, 0, slot_bytes(768, False), 4, 4, C.byref(w)) == 1 and w.value == 4
    assert ll.ll_placement(1, 1536, 0, slot_bytes(1536, False), 4, 4, C.byref(w)) == 1 and w.value == 4
    # a 32-KiB visited set next to it: four walkers no longer fit — HBM under the automatic rule, LDS when forced or when the
    # launch runs one walker per workgroup anyway
    assert ll.ll_placement(1, 4096, 0, slot_bytes(128, True), 4, 4, C.byref(w)) == 2
    assert ll.ll_placement(2, 4096, 0, slot_bytes(128, True), 4, 4, C.byref(w)) == 1 and w.value == 2
    assert ll.ll_placement(1, 4096, 0, slot_bytes(128, True), 1, 4, C.byref(w)) == 1 and w.value == 2
    # a slot that leaves no room at all
    assert ll.ll_placement(2, 4096, 0, LDS_PER_CU - 4096, 1, 4, C.byref(w)) == 2


@pytest.mark.parametrize("cells,limit", [(513, 513), (576, 576), (577, 577), (640, 600), (1536, 1536), (4096, 4096), (4096, 4095)])
def test_list_model_equals_sorted_vector(ll, cells, limit):
    """The list's arithmetic — tile tops, two-read lower_bound, tile-wise shift — against a std::vector kept by
    sorted_buffer_gt's rule.  Distances from a handful of values (ties in bulk: "new before equal"), ascending and
    descending runs (every insert at the end / at the front), and more inserts than the limit (the last entry drops)."""
    rng = np.random.default_rng(cells * 7 + limit)
    n = 2 * limit + 300
    parts = [rng.integers(0, 40, n // 2).astype(np.float32), rng.random(n // 4, dtype=np.float32),
             np.arange(n // 8, dtype=np.float32)[::-1] / 8, np.arange(n - n // 2 - n // 4 - n // 8, dtype=np.float32) / 3]
    for order in (0, 1):
        d = np.ascontiguousarray(np.concatenate(parts if order == 0 else parts[::-1]))
        s = np.arange(len(d), dtype=np.uint32)
        bad = ll.ll_model_check(d.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), C.c_uint64(len(d)), cells, limit)
        assert bad == 0, "first difference after insert %d" % (bad - 1)


def test_lds_list_kernels_exist_and_spill_nothing():
    """Every metric and row width has a k_search instantiation with the list in LDS; none uses scratch memory, and all fit the
    128 registers per lane of a 1024-thread workgroup."""
    from __graft_entry__ import load_package
    pkg = load_package()
    pkg.build_library()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    seen = set()
    for name, vgpr, agpr, sgpr, scratch, lds in kernel_resources.resources(pkg.LIB_PATH):
        m = re.match(r"void vss::k_search<(\d+), (\d+), (\d+), (\d+), (\d+)>", name)
        if not m or int(m.group(4)) != LDS_LIST_E:
            continue
        assert int(m.group(5)) == 1024, name
        assert scratch == 0, (name, vgpr, sgpr, scratch)
        assert vgpr <= 128, (name, vgpr, agpr)
        seen.add((int(m.group(1)), int(m.group(2))))
    assert seen == {(mt, nch) for mt in (0, 1, 2) for nch in (0, 1, 2, 3, 4, 6)}, seen
