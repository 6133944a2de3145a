"""The host side of vss_search_batch_filtered_groups_auto without a GPU: the routing rule and the partition plan
(duckdb-vss_amd/csrc/filter_route.h — the code vss_engine.hip carries out) checked by host/filter_route_check.cpp as a
stand-alone program under the address and undefined-behaviour sanitizers, the rule held against its restatement in Python
integers, and the harness of the host classes through the compiler's host pass."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")


def rule_exact(length, live, limit, c):
    """group goes exact iff len^2 * 64 <= C * limit * L; nothing admitted, or nothing linked, is exact"""
    if length == 0 or live == 0:
        return True
    return length * length * 64 <= c * limit * live


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    """its own binary, nothing preloaded, nothing loaded into Python"""
    exe = str(tmp_path_factory.mktemp("filter_route") / "filter_route_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HOST, "filter_route_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout.strip().splitlines()


def test_filter_route_check_runs_clean_under_sanitizers(check_output):
    assert check_output[-1] == "filter route check ok"


def test_rule_matches_python_integers(check_output):
    rows = [tuple(int(x) for x in line.split()[1:]) for line in check_output if line.startswith("rule ")]
    assert len(rows) >= 300
    seen = set()
    for length, live, limit, c, exact in rows:
        assert bool(exact) == rule_exact(length, live, limit, c), (length, live, limit, c, exact)
        seen.add(exact)
    assert seen == {0, 1}  # both answers occur: the comparison is not vacuous
    # the record the default constant comes from: exact at a quarter of 10^6 rows, graph at a half
    assert rule_exact(250_000, 1_000_000, 64, 62_500) and not rule_exact(250_001, 1_000_000, 64, 62_500)


def test_filter_route_harness_compiles():
    """hipcc, host pass only: the harness names the new entry points and the new methods of both host classes"""
    subprocess.check_call(["hipcc", "-std=c++17", "-fsyntax-only", "-Wall", "--offload-arch=gfx950",
                           os.path.join(HOST, "filter_route_harness.cpp")])
