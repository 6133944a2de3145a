"""The host side of vss_search_batch_by_label_box without a GPU: the box part of duckdb-vss_amd/csrc/label_filter.h — the admission
rule of a conjunction of ranges over several label columns, the walker's AND of two-cell forms, the listing kernels' register
form, the layout of the walker's table, the distinct rows and group numbers of a call — checked by host/label_box_check.cpp as
a stand-alone program under the address and undefined-behaviour sanitizers, every line it prints restated in NumPy, and the
harness of the host classes through the compiler's host pass."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")
NO_LABEL = 0xFFFFFFFF
TWO32 = 1 << 32
EDGE = [0, 1, 2, 7, 8, 9, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF]
COLUMN_ROWS = {0: 11, 1: 7, 2: 9, 3: 5}
FREE_KEY = (1 << 63) - 1


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    """its own binary, nothing preloaded, nothing loaded into Python"""
    exe = str(tmp_path_factory.mktemp("label_box") / "label_box_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HOST, "label_box_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout.strip().splitlines()


def ints(line):
    return [int(x) for x in line.split()[1:]]


def test_label_box_check_runs_clean_under_sanitizers(check_output):
    """the program itself compares the rule with the walker's and the listing kernels' forms on every case"""
    assert check_output[-1] == "label box check ok"
    assert not [line for line in check_output if line.startswith("FAILED")]


@pytest.fixture(scope="module")
def admit_rows(check_output):
    """{m: uint64 matrix}: m, key (as uint64: -1 and the free key are recognised by value), result, then per named column its
    number, its cells, the label every cell holds, lo, hi"""
    by_m = {1: [], 2: [], 4: []}
    for line in check_output:
        if line.startswith("admit "):
            by_m[int(line[6])].append(line)
    out = {}
    for m, lines in by_m.items():
        out[m] = np.array([ints(line) for line in lines], dtype=object)
        assert out[m].shape[1] == 3 + 5 * m
    return out


@pytest.mark.parametrize("m", [1, 2, 4])
def test_rule_is_the_numpy_restatement(admit_rows, m):
    """admit m key result (column rows label lo hi) x m: every combination of the eleven edge values in the first named column and
    a reduced set in the others, at keys -1, 0, the last cell of the shortest named column, one past it, the last cell of the
    longest, the free key"""
    rows = admit_rows[m]
    cases = len(EDGE) ** 3 * 3 ** (m - 1) + (len(EDGE) if m == 2 else 0)
    assert len(rows) == cases * 6
    key = np.array(rows[:, 1].tolist(), dtype=np.int64)
    got = np.array(rows[:, 2].tolist(), dtype=bool)
    expect = np.ones(len(rows), dtype=bool)
    clause, has_cell, named_rows = [], [], []
    for j in range(m):
        column, cells, label, lo, hi = (np.array(rows[:, 3 + 5 * j + c].tolist(), dtype=np.uint64) for c in range(5))
        assert all(COLUMN_ROWS[int(c)] == int(r) for c, r in set(zip(column.tolist(), cells.tolist())))
        has_cell.append((key >= 0) & (key < cells.astype(np.int64)))
        clause.append((label != NO_LABEL) & (lo <= label) & (label <= hi))
        named_rows.append(cells.astype(np.int64))
        expect &= has_cell[j] & clause[j]
    assert np.array_equal(got, expect)
    # the keys: -1, 0, shortest - 1, shortest, longest - 1, the free key
    shortest, longest = np.min(named_rows, axis=0), np.max(named_rows, axis=0)
    assert np.all(np.isin(key, [-1, 0, FREE_KEY]) | (key == shortest - 1) | (key == shortest) | (key == longest - 1))
    for special in (-1, 0, FREE_KEY):
        assert (key == special).sum() == cases
    # the first named column sees every combination of the edge values
    first = set(zip(*(rows[:, 3 + 2 + c].tolist() for c in range(3))))
    assert first >= {(a, b, c) for a in EDGE for b in EDGE for c in EDGE}
    # every clause decides somewhere
    assert got.any()  # all clauses true
    everywhere = np.all(has_cell, axis=0)
    for j in range(m):
        others = np.all([clause[i] & has_cell[i] for i in range(m) if i != j] + [np.ones(len(rows), dtype=bool)], axis=0)
        assert (~got & others & has_cell[j] & ~clause[j]).any(), j   # this column's range alone rejects
        label, lo, hi = (np.array(rows[:, 3 + 5 * j + c].tolist(), dtype=np.uint64) for c in (2, 3, 4))
        assert (~got & others & has_cell[j] & (label == NO_LABEL) & (lo == 0) & (hi == NO_LABEL)).any(), j  # NO_LABEL in this column only
        assert (~got & others & everywhere & (lo > hi)).any(), j                                             # one empty range empties the box
    if m > 1:
        # a row that has a cell in one named column and not in the shorter one: every range holds, the row is not admitted
        assert (~got & np.all(clause, axis=0) & np.any(has_cell, axis=0) & ~everywhere).any()
        assert (key == shortest).sum() and (got[key == shortest - 1]).any() and not got[key == shortest].any()


def test_table_cells_are_the_documented_encoding(check_output):
    """table m n_queries cells, then cell q j index lo hi cell_lo cell_width: cell 0 holds m, cells 1 .. m the columns, query q's
    pair for named column j sits at 1 + m + 2 m q + 2 j, and the pair is the range call's {lo, min(hi, 2^32 - 2) - lo} / {2^32, 0}"""
    at = [i for i, line in enumerate(check_output) if line.startswith("table ")]
    assert [ints(check_output[i])[0] for i in at] == [1, 2, 4]
    empties = pairs = 0
    for i in at:
        m, nq, cells = ints(check_output[i])
        assert cells == 1 + m + 2 * m * nq
        seen = []
        for line in check_output[i + 1:i + 1 + nq * m]:
            assert line.startswith("cell ")
            q, j, index, lo, hi, cell_lo, cell_width = ints(line)
            assert index == 1 + m + 2 * m * q + 2 * j and index + 1 < cells
            top = min(hi, NO_LABEL - 1)
            assert (cell_lo, cell_width) == ((TWO32, 0) if lo > top else (lo, top - lo)), (lo, hi)
            empties += lo > top
            pairs += 1
            seen += [index, index + 1]
        assert seen == list(range(1 + m, cells))  # the pairs tile the table behind its header, in query order
    assert 0 < empties < pairs


def test_groups_are_the_sorted_distinct_raw_rows(check_output):
    at = [i for i, line in enumerate(check_output) if line.startswith("boxes ")]
    assert len(at) >= 9
    seen = set()
    for i in at:
        assert [check_output[i + j].split()[0] for j in range(5)] == ["boxes", "lo", "hi", "rows", "group_of"]
        (m,), lo, hi, flat, group_of = (ints(check_output[i + j]) for j in range(5))
        n = len(lo) // m
        mine = [tuple(v for j in range(m) for v in (lo[q * m + j], hi[q * m + j])) for q in range(n)]
        want = sorted(set(mine))  # tuples of Python ints: lexicographic, unsigned
        assert [tuple(flat[g * 2 * m:(g + 1) * 2 * m]) for g in range(len(flat) // (2 * m))] == want
        assert group_of == [want.index(row) for row in mine]
        if len(want) < n:
            seen.add("duplicates")
        if len([row for row in want if any(row[2 * j] > row[2 * j + 1] for j in range(m))]) >= 2:
            seen.add("two empty rows")
        if m > 1 and any(a[:-2] == b[:-2] and a != b for a, b in zip(want, want[1:])):
            seen.add("last column only")
        if any(row[0] >= 0x80000000 for row in want) and any(row[0] < 0x80000000 for row in want):
            seen.add("sign bit")
        if not lo:
            seen.add("none")
        seen.add("m %d" % m)
    assert seen == {"duplicates", "two empty rows", "last column only", "sign bit", "none", "m 1", "m 2", "m 3", "m 4"}


def test_label_box_harness_compiles():
    """hipcc, host pass only: the harness names the new entry points and the new methods of both host classes"""
    subprocess.check_call(["hipcc", "-std=c++17", "-fsyntax-only", "-Wall", "--offload-arch=gfx950",
                           os.path.join(HOST, "label_box_harness.cpp")])
