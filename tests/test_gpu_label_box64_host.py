"""-m gpu: the search by label box64 through the host classes (duckdb-vss_amd/host/label_box64_harness.cpp):
vss_host::HNSWIndex and a vss_host::ShardedHNSWIndex of 3 co-resident shards, each holding the whole columns — a 32-bit tenant and
a 64-bit timestamp of different length — against their bitmap methods on the table the contract derives from the columns and the
call's boxes of 64-bit ends, in all three modes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")


@pytest.mark.gpu
def test_label_box64_harness():
    subprocess.check_call(["make", "-s", "-C", HOST])
    p = subprocess.run([os.path.join(HOST, "label_box64_harness")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "label box64 ok", p.stdout
    assert any(l.startswith("one index:") for l in lines)
    assert any(l.startswith("3 shards") for l in lines)
