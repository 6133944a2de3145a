"""-m gpu: routed per-query predicates through the host classes (duckdb-vss_amd/host/filter_route_harness.cpp):
vss_host::HNSWIndex against the two existing calls according to its route table, vss_host::ShardedHNSWIndex with 1, 2 and 3
co-resident shards against the CPU merge of per-shard answers assembled from the two existing per-shard calls according to each
shard's route table."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")


@pytest.mark.gpu
def test_filter_route_harness():
    subprocess.check_call(["make", "-s", "-C", HOST])
    p = subprocess.run([os.path.join(HOST, "filter_route_harness")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "filter route ok", p.stdout
    assert any(l.startswith("one index:") for l in lines)
    assert all(any(l.startswith("%d shard(s)" % g) for l in lines) for g in (1, 2, 3))
