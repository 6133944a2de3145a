"""The host side of vss_search_batch_by_label_range without a GPU: the range half of duckdb-vss_amd/csrc/label_filter.h — the
admission rule of a label range, the walker's two-cell one-comparison form of it, the listing kernels' form, the distinct pairs
and group numbers of a call — checked by host/label_range_check.cpp as a stand-alone program under the address and
undefined-behaviour sanitizers, every line it prints restated in NumPy, and the harness of the host classes through the
compiler's host pass."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")
NO_LABEL = 0xFFFFFFFF
TWO32 = 1 << 32
EDGE = [0, 1, 2, 7, 8, 9, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF]
LABELLED = 11
FREE_KEY = (1 << 63) - 1


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    """its own binary, nothing preloaded, nothing loaded into Python"""
    exe = str(tmp_path_factory.mktemp("label_range") / "label_range_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HOST, "label_range_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout.strip().splitlines()


def ints(line):
    return [int(x) for x in line.split()[1:]]


def test_label_range_check_runs_clean_under_sanitizers(check_output):
    """the program itself compares the rule with the walker's and the listing kernels' forms on every combination"""
    assert check_output[-1] == "label range check ok"
    assert not [line for line in check_output if line.startswith("FAILED")]


def test_rule_is_the_numpy_restatement(check_output):
    """admit lo hi label key result: every combination of the edge values, at keys -1, 0, last cell, one past it, the free key"""
    rows = np.array([ints(line) for line in check_output if line.startswith("admit ")], dtype=object)
    keys = [-1, 0, LABELLED - 1, LABELLED, FREE_KEY]
    assert len(rows) == len(EDGE) ** 3 * len(keys)
    lo, hi, label, key = (np.array(rows[:, c].tolist(), dtype=np.int64 if c == 3 else np.uint64) for c in range(4))
    got = np.array(rows[:, 4].tolist(), dtype=bool)
    assert set(lo.tolist()) == set(EDGE) and set(hi.tolist()) == set(EDGE) and set(label.tolist()) == set(EDGE)
    assert set(key.tolist()) == set(keys)
    expect = (key >= 0) & (key < LABELLED) & (label != NO_LABEL) & (lo <= label) & (label <= hi)
    assert np.array_equal(got, expect)
    # every clause decides somewhere
    has_cell = (key >= 0) & (key < LABELLED)
    assert got.any() and (~got & has_cell).any()
    assert (~got & ~has_cell & (lo <= label) & (label <= hi) & (label != NO_LABEL)).any()   # in range, but no cell
    assert (~got & has_cell & (label == NO_LABEL) & (hi == NO_LABEL)).any()                  # "no upper bound" meets a NO_LABEL cell
    assert (got & (hi == NO_LABEL) & (label == NO_LABEL - 1)).any()                          # ... and the largest label
    assert (~got & has_cell & (lo > hi)).any() and (got & (lo == hi)).any()


def test_walker_cells_are_the_documented_encoding(check_output):
    """cells lo hi cell_lo cell_width: {lo, min(hi, 2^32 - 2) - lo}, an empty range {2^32, 0}; and the one comparison
    (label - cell_lo) mod 2^64 <= cell_width is the rule for every 32-bit label, the NO_LABEL cell included"""
    rows = [ints(line) for line in check_output if line.startswith("cells ")]
    assert len(rows) == len(EDGE) ** 2
    labels = np.array(EDGE, dtype=np.uint64)
    empties = 0
    for lo, hi, cell_lo, cell_width in rows:
        top = min(hi, NO_LABEL - 1)
        assert (cell_lo, cell_width) == ((TWO32, 0) if lo > top else (lo, top - lo)), (lo, hi)
        empties += lo > top
        with np.errstate(over="ignore"):
            one_comparison = (labels - np.uint64(cell_lo)) <= np.uint64(cell_width)  # uint64 arithmetic wraps, as the kernel's
        rule = (labels != NO_LABEL) & (labels >= lo) & (labels <= hi)
        assert np.array_equal(one_comparison, rule), (lo, hi)
    assert 0 < empties < len(rows)


def test_groups_are_the_sorted_distinct_raw_pairs(check_output):
    at = [i for i, line in enumerate(check_output) if line.split()[:1] == ["lo"]]
    assert len(at) >= 7
    seen = set()
    for i in at:
        assert [check_output[i + j].split()[0] for j in range(4)] == ["lo", "hi", "pairs", "group_of"]
        lo, hi, flat, group_of = (ints(check_output[i + j]) for j in range(4))
        want = sorted(set(zip(lo, hi)))  # tuples of Python ints: lexicographic, unsigned
        assert list(zip(flat[0::2], flat[1::2])) == want
        assert group_of == [want.index(p) for p in zip(lo, hi)]
        if len(want) < len(lo):
            seen.add("duplicates")
        if len([p for p in want if p[0] > p[1]]) >= 2:
            seen.add("two empty pairs")
        if len({p[0] for p in want}) < len(want):
            seen.add("same lo")
        if any(p[0] >= 0x80000000 for p in want) and any(p[0] < 0x80000000 for p in want):
            seen.add("sign bit")
        if not lo:
            seen.add("none")
    assert seen == {"duplicates", "two empty pairs", "same lo", "sign bit", "none"}


def test_label_range_harness_compiles():
    """hipcc, host pass only: the harness names the new entry points and the new methods of both host classes"""
    subprocess.check_call(["hipcc", "-std=c++17", "-fsyntax-only", "-Wall", "--offload-arch=gfx950",
                           os.path.join(HOST, "label_range_harness.cpp")])
