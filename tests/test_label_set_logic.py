"""The host side of vss_search_batch_by_label_set without a GPU: the set half of duckdb-vss_amd/csrc/label_filter.h — the
admission rule of a label set, the register form the kernels apply to a cell, the padded rows of the walker's table, the distinct
raw rows and group numbers of a call — checked by host/label_set_check.cpp as a stand-alone program under the address and
undefined-behaviour sanitizers, every line it prints restated in NumPy; the harness of the host classes through the compiler's
host pass; and the registers and scratch of the new kernels, read from the built library's code object."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")
NO_LABEL = 0xFFFFFFFF
SET_MAX = 32
EDGE = [0, 1, 2, 7, 8, 9, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF]
LABELLED = 11
FREE_KEY = (1 << 63) - 1


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    """its own binary, nothing preloaded, nothing loaded into Python"""
    exe = str(tmp_path_factory.mktemp("label_set") / "label_set_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HOST, "label_set_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout.strip().splitlines()


def ints(line):
    return [int(x) for x in line.split()[1:]]


def test_label_set_check_runs_clean_under_sanitizers(check_output):
    """the program itself compares the rule with the register form and with the walker's padded rows on every combination"""
    assert check_output[-1] == "label set check ok"
    assert not [line for line in check_output if line.startswith("FAILED")]


def test_rule_is_the_numpy_restatement(check_output):
    """admit label key result width word ...: the edge values as label and as members, widths 1, 2, 3 and 32, at keys -1, 0,
    the last cell, one past it and the free key"""
    rows = [ints(line) for line in check_output if line.startswith("admit ")]
    keys = [-1, 0, LABELLED - 1, LABELLED, FREE_KEY]
    n_sets = len(EDGE) + len(EDGE) ** 2 + len(EDGE) ** 3 + 3 * len(EDGE) + 2
    assert len(rows) == n_sets * len(EDGE) * len(keys)
    seen = set()
    widths = {}
    for label, key, got, width, *words in rows:
        assert len(words) == width
        has_cell = 0 <= key < LABELLED
        expect = has_cell and label != NO_LABEL and label in words
        assert got == int(expect), (label, key, words)
        widths[width] = widths.get(width, 0) + 1
        members = [w for w in words if w != NO_LABEL]
        if has_cell and label == NO_LABEL and NO_LABEL in words and not got:
            seen.add("NO_LABEL cell meets NO_LABEL padding: not admitted")
        if got and width == SET_MAX and words[-1] == label and label not in words[:-1]:
            seen.add("the only hit is the last of 32 words")
        if got and width == SET_MAX and words[0] == label and label not in words[1:]:
            seen.add("the only hit is the first of 32 words")
        if not got and not has_cell and label != NO_LABEL and label in words:
            seen.add("a member, but no cell")
        if not members and not got and has_cell:
            seen.add("all padding admits nothing")
        if got and words.count(label) > 1:
            seen.add("a repeat")
        if got and label >= 0x80000000:
            seen.add("sign bit")
        if not got and has_cell and label != NO_LABEL and members:
            seen.add("no member")
    assert set(widths) == {1, 2, 3, SET_MAX}
    assert {w for _, _, _, _, *ws in rows for w in ws} >= set(EDGE)
    assert {label for label, *_ in rows} == set(EDGE) and {key for _, key, *_ in rows} == set(keys)
    assert seen == {"NO_LABEL cell meets NO_LABEL padding: not admitted", "the only hit is the last of 32 words",
                    "the only hit is the first of 32 words", "a member, but no cell", "all padding admits nothing", "a repeat",
                    "sign bit", "no member"}
    # order and repeats inside a row do not change what it admits: the answers depend on the SET of members only
    by_members = {}
    for label, key, got, width, *words in rows:
        by_members.setdefault((label, key, frozenset(w for w in words if w != NO_LABEL)), set()).add(got)
    assert all(len(v) == 1 for v in by_members.values())


def test_groups_are_the_sorted_distinct_raw_rows(check_output):
    at = [i for i, line in enumerate(check_output) if line.split()[:1] == ["sets"]]
    assert len(at) >= 10
    seen = set()
    padding_widths = set()
    for i in at:
        assert [check_output[i + j].split()[0] for j in range(3)] == ["sets", "rows", "group_of"]
        (width, *flat), rows, group_of = (ints(check_output[i + j]) for j in range(3))
        sets = [tuple(flat[q * width:(q + 1) * width]) for q in range(len(flat) // width)]
        want = sorted(set(sets))  # tuples of Python ints: lexicographic, unsigned
        assert [tuple(rows[g * width:(g + 1) * width]) for g in range(len(rows) // width)] == want
        assert group_of == [want.index(s) for s in sets]
        # NumPy says the same (and the GPU test derives its table so)
        if sets:
            u, inverse = np.unique(np.array(sets, dtype=np.uint32), axis=0, return_inverse=True)
            assert [tuple(r) for r in u.tolist()] == want and np.asarray(inverse).reshape(-1).tolist() == group_of
        if len(want) < len(sets):
            seen.add("duplicates")
        if (NO_LABEL,) * width in want:
            padding_widths.add(width)
        if len({frozenset(s) for s in want}) < len(want):
            seen.add("same members, two orders")
        if any(s[0] >= 0x80000000 for s in want) and any(s[0] < 0x80000000 for s in want):
            seen.add("sign bit")
        if not sets:
            seen.add("none")
        if width == SET_MAX and any(a[:-1] == b[:-1] and a != b for a in want for b in want):
            seen.add("32 words, the last decides")
    assert len(padding_widths) >= 2  # all-padding rows at different widths, across calls
    assert seen == {"duplicates", "same members, two orders", "sign bit", "none", "32 words, the last decides"}


def test_wrapper_pads_lists_and_refuses_shapes():
    """GpuIndex.label_set_matrix: the matrix as it is, per-query sequences padded with NO_LABEL to the longest, a wrong shape
    refused"""
    sys.path.insert(0, ROOT)
    import __graft_entry__
    G = __graft_entry__.load_package().GpuIndex
    m = G.label_set_matrix([[3, 1], [], (7,), np.array([4, 5, 6])], 4)
    assert m.dtype == np.uint32 and m.tolist() == [[3, 1, NO_LABEL], [NO_LABEL] * 3, [7, NO_LABEL, NO_LABEL], [4, 5, 6]]
    assert G.label_set_matrix([[], []], 2).tolist() == [[NO_LABEL], [NO_LABEL]]
    a = np.arange(6, dtype=np.uint32).reshape(3, 2)
    assert G.label_set_matrix(a, 3).tolist() == a.tolist()
    for bad, nq in ((a, 2), (a.reshape(-1), 6), ([[1], [2]], 3)):
        with pytest.raises(ValueError):
            G.label_set_matrix(bad, nq)
    assert G.LABEL_SET_MAX == SET_MAX


def test_label_set_harness_compiles():
    """hipcc, host pass only: the harness names the new entry points and the new methods of both host classes"""
    subprocess.check_call(["hipcc", "-std=c++17", "-fsyntax-only", "-Wall", "--offload-arch=gfx950",
                           os.path.join(HOST, "label_set_harness.cpp")])


# ------------------------------------------------------------------------------------------------- kernel resources
@pytest.fixture(scope="module")
def resources():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__
    import kernel_resources
    pkg = __graft_entry__.load_package()
    assert os.path.exists(pkg.LIB_PATH), "the library is built by __graft_entry__.build()"
    return {name: (vgpr, sgpr, scratch) for name, vgpr, agpr, sgpr, scratch, lds in kernel_resources.resources(pkg.LIB_PATH)}


def test_set_walkers_spill_no_more_than_their_range_twins(resources):
    """every k_search_sets / k_search_solo_sets instantiation beside the *_ranges kernel of the same template arguments: at most
    its scratch bytes, none where it has none; and within the 128 VGPRs a 1024-thread workgroup may use"""
    seen = 0
    for name, (vgpr, sgpr, scratch) in resources.items():
        m = re.match(r"void vss::(k_search_sets|k_search_solo_sets)<(.*)>\(", name)
        if not m:
            continue
        twin = name.replace("_sets<", "_ranges<")
        assert twin in resources, name
        assert scratch <= resources[twin][2], (name, scratch, resources[twin])
        args = [int(x) for x in m.group(2).split(", ")]
        if m.group(1) == "k_search_sets" and args[4] == 1024:
            assert vgpr <= 128, (name, vgpr)
        seen += 1
    twins = [n for n in resources if re.match(r"void vss::k_search(_solo)?_ranges<", n)]
    assert seen == len(twins) >= 200, (seen, len(twins))  # the same template arguments, every one of them


def test_set_listing_kernels_use_no_scratch(resources):
    found = {n: r for n, r in resources.items() if re.match(r"vss::k_set_list_(count|scatter)\(", n)}
    assert len(found) == 2, sorted(found)
    for name, (vgpr, sgpr, scratch) in found.items():
        assert scratch == 0, (name, vgpr, sgpr, scratch)


def test_resource_listing_shows_no_existing_kernel_touched():
    """profiles/r20_label_set_kernel_resources.diff: the listing of the parent commit's library against this tree's.  Every
    line of the diff is an added one"""
    body = [line for line in open(os.path.join(ROOT, "profiles", "r20_label_set_kernel_resources.diff")).read().splitlines()
            if line and not line.startswith("#")]
    assert len(body) > 200
    assert not [line for line in body if line.startswith("<") or line.startswith("-") or line.startswith("!")]
    assert sum(line.startswith(">") for line in body) >= 214
