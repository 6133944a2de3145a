"""-m gpu: label predicates in the pipelined and multi-batch launches through the host classes
(duckdb-vss_amd/host/label_pipeline_harness.cpp): a vss_host::ShardedHNSWIndex of 2 co-resident shards whose six SearchBatchByLabel*
methods, in mode graph, start every shard through vss_search_by_label_device_begin before the first is ended — against the merge of
the blocking per-shard _device calls they made before, called directly; and vss_host::HNSWIndex::ExecuteMultiScanChunksByLabel —
three join chunks with a predicate each in one launch — against the per-chunk methods."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")

FORMS = ("eq", "range", "set", "box", "box64", "set box")


@pytest.mark.gpu
def test_label_pipeline_harness():
    subprocess.check_call(["make", "-s", "-C", HOST])
    p = subprocess.run([os.path.join(HOST, "label_pipeline_harness")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "label pipeline ok", p.stdout
    for form in FORMS:
        assert any(l.startswith("2 shards, %s:" % form) for l in lines), form
        assert any(l.startswith("one index, %s:" % form) for l in lines), form
