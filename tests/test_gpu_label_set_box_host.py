"""-m gpu: the search by label set box through the host classes (duckdb-vss_amd/host/label_set_box_harness.cpp):
vss_host::HNSWIndex and a vss_host::ShardedHNSWIndex of 2 co-resident shards, each holding the whole columns — a 32-bit group as
the set column and a 64-bit timestamp of different length as the range column — against their bitmap methods on the table the
contract derives from the columns and the call's lists and ranges, in all three modes; the shards' merged answers also equal the
single index's."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")


@pytest.mark.gpu
def test_label_set_box_harness():
    subprocess.check_call(["make", "-s", "-C", HOST])
    p = subprocess.run([os.path.join(HOST, "label_set_box_harness")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "label set box ok", p.stdout
    assert any(l.startswith("one index:") for l in lines)
    assert any(l.startswith("2 shards") for l in lines)
