"""-m gpu: exact top-k under per-query predicates through the host classes (duckdb-vss_amd/host/exact_filtered_harness.cpp):
vss_host::HNSWIndex against the harness's own brute force over the admitted live rows, vss_host::ShardedHNSWIndex with 1, 2 and
3 co-resident shards against the one index, cell by cell."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")


@pytest.mark.gpu
def test_exact_filtered_harness():
    subprocess.check_call(["make", "-s", "-C", HOST])
    p = subprocess.run([os.path.join(HOST, "exact_filtered_harness")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "exact filtered ok", p.stdout
    assert any(l.startswith("one index:") for l in lines)
    assert all(any(l.startswith("%d shard(s)" % g) for l in lines) for g in (1, 2, 3))
