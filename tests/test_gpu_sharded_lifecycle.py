"""-m gpu: the single-process sharded index (duckdb-vss_amd/host/sharded_index.hpp) through an index's life after
CREATE INDEX — bulk build and GetStats, exact probe against a host brute force, inserts after the build (block-cyclic
routing, NULL rows), deletes routed by the same rule, filtered probe, PersistToBlocks / LoadFromBlocks (bit-identical
answers after reload), Compact, and refused loads that leave the index as it was.  host/sharded_lifecycle_harness.cpp
holds the checks; it exits non-zero at the first one that fails."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")


def _run(*devices):
    subprocess.check_call(["make", "-s", "-C", HOST])
    p = subprocess.run([os.path.join(HOST, "sharded_lifecycle_harness"), *devices], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[-2] == "sharded lifecycle ok", p.stdout
    return lines


@pytest.mark.gpu
def test_sharded_lifecycle_three_shards_on_one_device():
    """Three shards on device 0: the per-shard answers travel by peer copies; 6001 rows do not divide by 3, the inserts
    are dealt to all three shards."""
    lines = _run()
    assert lines[-1] == "exchange: peer"
    assert sum(l.startswith("refused (") for l in lines) == 3


@pytest.mark.gpu
def test_sharded_lifecycle_one_shard_exchanges_through_rccl():
    """`sharded_lifecycle_harness 0`: one shard on a device of its own takes the RCCL path (one grouped all-gather of the
    packed blocks per probe, vss_merge_topk_packed_device) for every kind of probe."""
    lines = _run("0")
    assert lines[-1] == "exchange: rccl"
    assert sum(l.startswith("refused (") for l in lines) == 3
