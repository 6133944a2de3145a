"""Per-query predicates through the host classes (duckdb-vss_amd/host): HNSWIndex::ExecuteMultiScanBatchGrouped and
ShardedHNSWIndex::SearchBatchFilteredGroups, checked by host/filter_groups_harness.cpp cell by cell against one filtered
call per group — on one index, on one shard and on two shards co-resident on a device (-m gpu).  Without a GPU: the
harness compiles, and the group-table arithmetic, validation and packing (csrc/filter_groups.h,
host/filter_group_tables.hpp) run as a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")


@pytest.mark.gpu
def test_filter_groups_harness_runs_clean():
    subprocess.check_call(["make", "-s", "-C", HOST])
    p = subprocess.run([os.path.join(HOST, "filter_groups_harness")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "filter groups ok", p.stdout
    assert any(l.startswith("one index:") for l in lines)
    assert any(l.startswith("1 shard(s)") for l in lines) and any(l.startswith("2 shard(s), exchange peer") for l in lines)


def test_filter_groups_check_runs_clean_under_sanitizers(tmp_path):
    """its own binary, nothing preloaded, nothing loaded into Python"""
    exe = str(tmp_path / "filter_groups_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HOST, "filter_groups_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == "filter groups check ok"


def test_filter_groups_harness_compiles():
    """The harness talks to the HIP runtime API through the sharded host class: hipcc, host pass only; its host-only part
    (the group tables) also under the sanitizers' instrumentation."""
    subprocess.check_call(["hipcc", "-std=c++17", "-fsyntax-only", "-Wall", "--offload-arch=gfx950",
                           os.path.join(HOST, "filter_groups_harness.cpp")])
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-fsanitize=address,undefined", "-x", "c++",
                           os.path.join(HOST, "filter_group_tables.hpp")])

