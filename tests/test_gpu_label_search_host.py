"""-m gpu: the search by label through the host classes (duckdb-vss_amd/host/label_search_harness.cpp): vss_host::HNSWIndex
against the bitmap calls on the table the contract derives from the label column, in all three modes;
vss_host::ShardedHNSWIndex with 1 and 3 co-resident shards, each holding the whole column, against the single index's answers
(exact; every mode for one shard) and against the CPU merge of the per-shard calls."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")


@pytest.mark.gpu
def test_label_search_harness():
    subprocess.check_call(["make", "-s", "-C", HOST])
    p = subprocess.run([os.path.join(HOST, "label_search_harness")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "label search ok", p.stdout
    assert any(l.startswith("one index:") for l in lines)
    assert all(any(l.startswith("%d shard(s)" % g) for l in lines) for g in (1, 3))
