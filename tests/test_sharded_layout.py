"""CPU: where a row of the sharded index lives, and how a persisted sharded index is framed
(duckdb-vss_amd/host/shard_layout.hpp): the routing rule — the row-range owner inside the build's range, block-cyclic in
2048-id blocks past it — and the container header, checked by shard_layout_check as a stand-alone program under
AddressSanitizer / UBSan; the same rule in duckdb-vss_amd/sharded.py (route_row) against the C++ table, line by line."""
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")

SHARDS = (1, 2, 3, 8)
TOTALS = (0, 1, 7, 6001)
BLOCK = 2048
INSERTED = 3 * BLOCK + 1


@pytest.fixture(scope="module")
def layout_check(tmp_path_factory):
    """shard_layout_check built under the sanitizers: its own binary, nothing preloaded, nothing loaded into Python."""
    exe = str(tmp_path_factory.mktemp("shard_layout") / "shard_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(HOST, "shard_layout_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def sharded():
    spec = importlib.util.spec_from_file_location("vss_sharded", os.path.join(ROOT, "duckdb-vss_amd", "sharded.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_layout_header_includes_nothing_of_the_engine():
    src = open(os.path.join(HOST, "shard_layout.hpp")).read()
    assert "#include <hip" not in src and "#include \"" not in src
    check = open(os.path.join(HOST, "shard_layout_check.cpp")).read()
    assert [l for l in check.splitlines() if l.startswith("#include \"")] == ['#include "shard_layout.hpp"']


def test_shard_layout_check_runs_clean_under_sanitizers(layout_check):
    p = subprocess.run([layout_check], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == "shard layout ok"
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_route_row_reproduces_the_cpp_table(layout_check, sharded):
    p = subprocess.run([layout_check, "--table"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    seen = set()
    lines = 0
    for line in p.stdout.splitlines():
        rowid, world, n_total, owner = map(int, line.split())
        assert sharded.route_row(rowid, world, n_total) == owner, line
        seen.add((world, n_total))
        lines += 1
    assert seen == {(g, n) for g in SHARDS for n in TOTALS}
    assert lines == sum(n + INSERTED for n in TOTALS) * len(SHARDS)  # every row of the grid, once


def test_route_row_is_owner_of_inside_the_build_range(sharded):
    for world in SHARDS:
        for n_total in TOTALS:
            for rowid in range(n_total):
                assert sharded.route_row(rowid, world, n_total) == sharded.owner_of(rowid, world, n_total)
            # past the range: block-cyclic, both sides of every block edge
            for b in range(1, 4):
                assert sharded.route_row(n_total + b * BLOCK - 1, world, n_total) == (b - 1) % world
                assert sharded.route_row(n_total + b * BLOCK, world, n_total) == b % world
    assert sharded.route_row(10, 4, 0, block=5) == 2
    with pytest.raises(ValueError):
        sharded.route_row(-1, 3, 6001)


def test_lifecycle_harness_compiles():
    """The host class and its lifecycle harness talk to the HIP runtime API: hipcc, host pass only (as
    test_host_harness.py does for sharded_harness.cpp)."""
    subprocess.check_call(["hipcc", "-std=c++17", "-fsyntax-only", "--offload-arch=gfx950",
                           os.path.join(HOST, "sharded_lifecycle_harness.cpp")])
