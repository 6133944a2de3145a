"""The host side of vss_search_batch_by_label without a GPU: duckdb-vss_amd/csrc/label_filter.h — the distinct values and
group numbers of a `want` array, the lookup the label listing kernels run, the admission rule, the range check and the gap
filling of vss_set_labels — checked by host/label_filter_check.cpp as a stand-alone program under the address and
undefined-behaviour sanitizers, every line it prints restated in NumPy, and the harness of the host classes through the
compiler's host pass."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")
NO_LABEL = 0xFFFFFFFF
NONE = 0xFFFFFFFF  # NO_LABEL_GROUP
TWO32 = 1 << 32


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    """its own binary, nothing preloaded, nothing loaded into Python"""
    exe = str(tmp_path_factory.mktemp("label_filter") / "label_filter_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HOST, "label_filter_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout.strip().splitlines()


def ints(line):
    return [int(x) for x in line.split()[1:]]


def test_label_filter_check_runs_clean_under_sanitizers(check_output):
    assert check_output[-1] == "label filter check ok"
    assert not [line for line in check_output if line.startswith("FAILED")]


def test_groups_are_numpy_unique(check_output):
    """values = the ascending distinct wanted values (NO_LABEL last), group_of = each query's index among them"""
    at = [i for i, line in enumerate(check_output) if line.split()[:1] == ["want"]]
    assert len(at) >= 7
    shapes = set()
    for i in at:
        want = np.array(ints(check_output[i]), dtype=np.uint32)
        assert check_output[i + 1].split()[0] == "values" and check_output[i + 2].split()[0] == "group_of"
        values, group_of = ints(check_output[i + 1]), ints(check_output[i + 2])
        u, inv = np.unique(want, return_inverse=True)
        assert values == u.tolist() and group_of == inv.tolist(), want
        if len(want):
            shapes.add("equal" if len(u) == 1 and len(want) > 1 else "distinct" if len(u) == len(want) else "mixed")
        if NO_LABEL in want.tolist():
            assert values[-1] == NO_LABEL
            shapes.add("null")
        if 0 in want.tolist() and TWO32 - 2 in want.tolist():
            shapes.add("ends")
    assert shapes == {"equal", "distinct", "mixed", "null", "ends"}


def test_lookup_is_searchsorted(check_output):
    sets, seen_u, outcomes = {}, set(), set()
    current = None
    n = 0
    for line in check_output:
        if line.startswith("lookupset "):
            f = ints(line)
            current = np.array(f[1:], dtype=np.uint64)
            assert len(current) == f[0] and np.all(current[1:] > current[:-1])
            sets[f[0]] = current
        elif line.startswith("lookup "):
            u, label, got = ints(line)
            assert len(current) == u
            at = int(np.searchsorted(current, label))
            want = at if label != NO_LABEL and at < u and int(current[at]) == label else NONE
            assert got == want, (u, label, got, want)
            seen_u.add(u)
            outcomes.add((got != NONE, label == NO_LABEL, NO_LABEL in current.tolist()))
            n += 1
    assert seen_u == {1, 2, 63, 64, 65, 1024} and n > 3000
    # found and not found; NO_LABEL probed against sets with and without it, never found
    assert {(True, False, False), (False, False, False), (False, True, True), (False, True, False)} <= outcomes
    assert not [o for o in outcomes if o[0] and o[1]]


def test_want_cell_and_admission(check_output):
    cells = dict(tuple(ints(line)) for line in check_output if line.startswith("cell "))
    assert cells == {0: 0, 1: 1, TWO32 - 2: TWO32 - 2, NO_LABEL: TWO32}
    labels = [ints(line) for line in check_output if line.startswith("labels ")]
    assert len(labels) == 1
    labels = labels[0]
    rows = [ints(line) for line in check_output if line.startswith("admit ")]
    assert len(rows) >= 100
    seen = set()
    for labelled, key, want, got in rows:
        expect = 0 <= key < labelled and want != NO_LABEL and labels[key] == want
        assert bool(got) == expect, (labelled, key, want, got)
        # every clause of the rule decides somewhere: (has a cell, wants a label, cell equals want)
        seen.add((0 <= key < labelled, want != NO_LABEL, 0 <= key < len(labels) and labels[key] == want, got))
    assert {s[3] for s in seen} == {0, 1}
    assert (False, True, True, 0) in seen      # the value matches but the row id has no cell (column shorter than the array)
    assert (True, False, True, 0) in seen      # the cell holds NO_LABEL and so does want: not admitted
    assert (True, True, False, 0) in seen and (True, True, True, 1) in seen


def test_label_range_ends_at_two_to_the_32(check_output):
    rows = [ints(line) for line in check_output if line.startswith("range ")]
    faults = set()
    for has_ptr, first, n, fault in rows:
        expect = 0 if n == 0 else 1 if not has_ptr else 2 if first + n > TWO32 else 0
        assert fault == expect, (has_ptr, first, n, fault)
        faults.add(fault)
    assert faults == {0, 1, 2}
    by_range = {(first, n): fault for has_ptr, first, n, fault in rows if has_ptr}
    assert by_range[(TWO32 - 1, 1)] == 0 and by_range[(TWO32 - 1, 2)] == 2  # first + n at 2^32 and one past it
    assert by_range[(0, TWO32)] == 0 and by_range[(0, TWO32 + 1)] == 2


def test_label_search_harness_compiles():
    """hipcc, host pass only: the harness names the new entry points and the new methods of both host classes"""
    subprocess.check_call(["hipcc", "-std=c++17", "-fsyntax-only", "-Wall", "--offload-arch=gfx950",
                           os.path.join(HOST, "label_search_harness.cpp")])


def test_gap_filling(check_output):
    rows = [ints(line) for line in check_output if line.startswith("write ")]
    assert len(rows) >= 8
    kinds = set()
    for labelled, first, n, rows_after, gap_begin, gap_end in rows:
        assert rows_after == max(labelled, first + n)
        assert (gap_begin, gap_end) == (labelled, max(labelled, first))
        kinds.add(("gap" if first > labelled else "touch" if first == labelled else "inside",
                   "grows" if first + n > labelled else "fits"))
    assert kinds == {("gap", "grows"), ("touch", "grows"), ("inside", "grows"), ("inside", "fits")}
