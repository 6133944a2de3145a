"""The host side of vss_search_batch_by_label_box64 without a GPU: the 64-bit part of duckdb-vss_amd/csrc/label_filter.h — the
admission rule of a conjunction of ranges with 64-bit ends over label columns of either width, the walker's (cell - lo) < count
form, the listing kernels' register form, the layout of the walker's table, the word pairs a box travels as, the distinct rows
and group numbers of a call — checked by host/label_box64_check.cpp as a stand-alone program under the address and
undefined-behaviour sanitizers, every line it prints restated in NumPy, and the harness of the host classes through the
compiler's host pass."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")
NO_LABEL = 0xFFFFFFFF
NO_LABEL64 = (1 << 64) - 1
T31, T32, T63 = 1 << 31, 1 << 32, 1 << 63
EDGE = [0, 1, T31, T32 - 2, T32 - 1, T32, T63 - 1, T63, NO_LABEL64 - 1, NO_LABEL64]
COLUMN_ROWS = {0: 11, 1: 7, 2: 9, 3: 5}
FREE_KEY = (1 << 63) - 1


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    """its own binary, nothing preloaded, nothing loaded into Python"""
    exe = str(tmp_path_factory.mktemp("label_box64") / "label_box64_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HOST, "label_box64_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout.strip().splitlines()


def ints(line):
    return [int(x) for x in line.split()[1:]]


def test_label_box64_check_runs_clean_under_sanitizers(check_output):
    """the program itself compares the rule with the walker's and the listing kernels' forms on every case"""
    assert check_output[-1] == "label box64 check ok"
    assert not [line for line in check_output if line.startswith("FAILED")]


@pytest.fixture(scope="module")
def admit_rows(check_output):
    """{m: object matrix}: m, key, result, then per named column its number, its cells, its width, the cell every row holds AS
    STORED, lo, hi"""
    by_m = {1: [], 2: [], 4: []}
    for line in check_output:
        if line.startswith("admit "):
            by_m[int(line[6])].append(line)
    out = {}
    for m, lines in by_m.items():
        out[m] = np.array([ints(line) for line in lines], dtype=object)
        assert out[m].shape[1] == 3 + 6 * m
    return out


def column_of(rows, j, c):
    return np.array(rows[:, 3 + 6 * j + c].tolist(), dtype=np.uint64)


@pytest.mark.parametrize("m", [1, 2, 4])
def test_rule_is_the_numpy_restatement(admit_rows, m):
    """admit m key result (column rows width cell lo hi) x m: every combination of the ten edge values for the cell, lo and hi
    of the first named column, for both widths of that column (m = 4: the wide one, the others 32, 64, 32), a reduced set in the
    others, at keys -1, 0, the last cell of the shortest named column, one past it, the free key"""
    rows = admit_rows[m]
    cases = {1: 2 * len(EDGE) ** 3, 2: 2 * len(EDGE) ** 3 * 3 + len(EDGE) + 3, 4: len(EDGE) ** 3 * 27}[m]
    assert len(rows) == cases * 5
    key = np.array(rows[:, 1].tolist(), dtype=np.int64)
    got = np.array(rows[:, 2].tolist(), dtype=bool)
    expect = np.ones(len(rows), dtype=bool)
    clause, has_cell, named_rows, widths = [], [], [], []
    for j in range(m):
        column, cells, width, stored, lo, hi = (column_of(rows, j, c) for c in range(6))
        assert all(COLUMN_ROWS[int(c)] == int(r) for c, r in set(zip(column.tolist(), cells.tolist())))
        assert set(width.tolist()) <= {32, 64}
        assert np.all(stored[width == 32] <= NO_LABEL)  # what a 32-bit column can hold
        # the widening: zero-extension, and the 32-bit NULL becomes the 64-bit NULL
        cell = np.where((width == 32) & (stored == NO_LABEL), np.uint64(NO_LABEL64), stored)
        has_cell.append((key >= 0) & (key < cells.astype(np.int64)))
        clause.append((cell != NO_LABEL64) & (lo <= cell) & (cell <= hi))
        named_rows.append(cells.astype(np.int64))
        widths.append(width)
        expect &= has_cell[j] & clause[j]
    assert np.array_equal(got, expect)
    shortest = np.min(named_rows, axis=0)
    assert np.all(np.isin(key, [-1, 0, FREE_KEY]) | (key == shortest - 1) | (key == shortest))
    for special in (-1, 0, FREE_KEY):
        assert (key == special).sum() == cases
    assert (key == shortest - 1).sum() == cases and (key == shortest).sum() == cases
    # the first named column sees every combination of the edge values — at both widths where the program runs both
    for width in ((32, 64) if m < 4 else (64,)):
        at = widths[0] == width
        first = set(zip(*(rows[at][:, 3 + 3 + c].tolist() for c in range(3))))
        low = (lambda v: v & NO_LABEL) if width == 32 else (lambda v: v)
        assert first >= {(low(a), b, c) for a in EDGE for b in EDGE for c in EDGE}
    if m > 1:  # mixed widths inside one case
        assert np.any(np.any([w == 32 for w in widths], axis=0) & np.any([w == 64 for w in widths], axis=0))
    if m == 4:
        assert all(set(widths[j].tolist()) == {(64, 32, 64, 32)[j]} for j in range(4))
    # every clause decides somewhere
    assert got.any()
    everywhere = np.all(has_cell, axis=0)
    for j in range(m):
        others = np.all([clause[i] & has_cell[i] for i in range(m) if i != j] + [np.ones(len(rows), dtype=bool)], axis=0)
        assert (~got & others & has_cell[j] & ~clause[j]).any(), j   # this column's range alone rejects
        width, stored, lo, hi = (column_of(rows, j, c) for c in (2, 3, 4, 5))
        null = np.where(width == 32, np.uint64(NO_LABEL), np.uint64(NO_LABEL64))
        assert (~got & others & has_cell[j] & (stored == null) & (lo == 0) & (hi == NO_LABEL64)).any(), j  # a NULL in this column only
        assert (~got & others & everywhere & (lo > hi)).any(), j                                            # one empty range empties the box
    # a comparison that the high word alone decides, either way
    stored, lo, hi = (column_of(rows, 0, c) for c in (3, 4, 5))
    same_low = ((stored & np.uint64(NO_LABEL)) >= (lo & np.uint64(NO_LABEL))) & ((stored & np.uint64(NO_LABEL)) <= (hi & np.uint64(NO_LABEL)))
    assert (~got & everywhere & same_low & (stored < lo)).any() or m == 4
    if m > 1:
        # a row that has a cell in one named column and not in the shorter one: every range holds, the row is not admitted
        assert (~got & np.all(clause, axis=0) & np.any(has_cell, axis=0) & ~everywhere).any()
        assert (got[key == shortest - 1]).any() and not got[key == shortest].any()


def test_high_word_pair(admit_rows):
    """ends (2^32 + 5, 2^32 + 9): the cell 2^32 + 7 is inside, the cell 7 is not, and a 32-bit column's 7 is not either"""
    rows = admit_rows[2]
    mine = [r for r in rows.tolist() if r[1] == 0 and r[3 + 6 + 4] == T32 + 5 and r[3 + 6 + 5] == T32 + 9]
    assert [(r[3 + 3], r[3 + 4], r[3 + 6 + 3], r[2]) for r in mine] == [(7, 7, T32 + 7, 1), (7, 7, 7, 0), (7, T32 + 5, T32 + 7, 0)]


def test_table_cells_are_the_documented_encoding(check_output):
    """table m n_queries cells wide_mask head, then cell q j index lo hi cell_lo cell_count: cell 0 holds m and the widths, cells
    1 .. m the columns, query q's pair for named column j sits at 1 + m + 2 m q + 2 j, and the pair is {lo, count} with top =
    min(hi, 2^64 - 2), count = 0 if lo > top else top - lo + 1"""
    at = [i for i, line in enumerate(check_output) if line.startswith("table ")]
    assert [ints(check_output[i])[0] for i in at] == [1, 2, 4]
    empties = pairs = unbounded = 0
    for i in at:
        m, nq, cells, wide_mask, head = ints(check_output[i])
        assert cells == 1 + m + 2 * m * nq
        assert head == m | wide_mask << 8 and wide_mask < 1 << m
        seen = []
        for line in check_output[i + 1:i + 1 + nq * m]:
            assert line.startswith("cell ")
            q, j, index, lo, hi, cell_lo, cell_count = ints(line)
            assert index == 1 + m + 2 * m * q + 2 * j and index + 1 < cells
            top = min(hi, NO_LABEL64 - 1)
            assert (cell_lo, cell_count) == (lo, 0 if lo > top else top - lo + 1), (lo, hi)
            assert cell_count < 1 << 64
            # the walker's test on the edge values IS the rule
            for cell in EDGE:
                assert ((cell - cell_lo) % (1 << 64) < cell_count) == (cell != NO_LABEL64 and lo <= cell <= hi), (cell, lo, hi)
            empties += lo > top
            unbounded += hi == NO_LABEL64 and lo <= top
            pairs += 1
            seen += [index, index + 1]
        assert seen == list(range(1 + m, cells))  # the pairs tile the table behind its header, in query order
    assert 0 < empties < pairs and unbounded


def test_groups_are_the_sorted_distinct_raw_rows(check_output):
    at = [i for i, line in enumerate(check_output) if line.startswith("boxes ")]
    assert len(at) >= 10
    seen = set()
    for i in at:
        assert [check_output[i + j].split()[0] for j in range(5)] == ["boxes", "lo", "hi", "rows", "group_of"]
        (m,), lo, hi, flat, group_of = (ints(check_output[i + j]) for j in range(5))
        n = len(lo) // m
        mine = [tuple(v for j in range(m) for v in (lo[q * m + j], hi[q * m + j])) for q in range(n)]
        want = sorted(set(mine))  # tuples of Python ints: lexicographic, unsigned, as 64-bit words
        assert [tuple(flat[g * 2 * m:(g + 1) * 2 * m]) for g in range(len(flat) // (2 * m))] == want
        assert group_of == [want.index(row) for row in mine]
        if len(want) < n:
            seen.add("duplicates")
        if len([row for row in want if any(row[2 * j] > row[2 * j + 1] for j in range(m))]) >= 2:
            seen.add("two empty rows")
        if m > 1 and any(a[:-2] == b[:-2] and a != b for a, b in zip(want, want[1:])):
            seen.add("last column only")
        if any(row[0] >= T63 for row in want) and any(row[0] < T63 for row in want):
            seen.add("sign bit")
        # an order that sorting by LOW words first, or as signed words, would get wrong
        if any(a[0] >> 32 < b[0] >> 32 and a[0] & NO_LABEL > b[0] & NO_LABEL for a, b in zip(want, want[1:])):
            seen.add("high word first")
        if not lo:
            seen.add("none")
        seen.add("m %d" % m)
    assert seen == {"duplicates", "two empty rows", "last column only", "sign bit", "high word first", "none", "m 1", "m 2", "m 3",
                    "m 4"}


def test_label_box64_harness_compiles():
    """hipcc, host pass only: the harness names the new entry points and the new methods of both host classes"""
    subprocess.check_call(["hipcc", "-std=c++17", "-fsyntax-only", "-Wall", "--offload-arch=gfx950",
                           os.path.join(HOST, "label_box64_harness.cpp")])
