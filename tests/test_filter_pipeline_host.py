"""Filtered probes through the pipelined (_begin / _end) and multi-batch calls, from the host side (duckdb-vss_amd/host):
host/filter_probe_harness.cpp holds ShardedHNSWIndex::SearchBatchFiltered / SearchBatchFilteredGroups — which now start every
shard before they wait for the first — against the merge of per-shard blocking calls, and the three C entry points against
their blocking counterparts (-m gpu).  Without a GPU: the harness compiles, and the resolve arithmetic of a launch that carries
several tables (csrc/filter_groups.h, the code k_resolve_filter_group_batches runs) is checked by host/filter_probe_check.cpp
as a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")


@pytest.mark.gpu
def test_filter_probe_harness_runs_clean():
    subprocess.check_call(["make", "-s", "-C", HOST])
    p = subprocess.run([os.path.join(HOST, "filter_probe_harness")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "filter probes ok", p.stdout
    assert any(l.startswith("one index:") for l in lines)
    assert any(l.startswith("1 shard(s)") for l in lines) and any(l.startswith("2 shard(s), exchange peer") for l in lines)


def test_filter_probe_check_runs_clean_under_sanitizers(tmp_path):
    """its own binary, nothing preloaded, nothing loaded into Python"""
    exe = str(tmp_path / "filter_probe_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HOST, "filter_probe_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == "filter probe check ok"


def test_filter_probe_harness_compiles():
    """hipcc, host pass only: the harness names the three new entry points and ShardedHNSWIndex::ShardHandle"""
    subprocess.check_call(["hipcc", "-std=c++17", "-fsyntax-only", "-Wall", "--offload-arch=gfx950",
                           os.path.join(HOST, "filter_probe_harness.cpp")])
