"""The host side of the label predicates in the pipelined and multi-batch launches without a GPU: the "several batches" part of
duckdb-vss_amd/csrc/label_filter.h — the launch-wide query -> (batch, row) mapping, the table's offsets under several batches, its
head, and every cell of it as the resolve kernels write it from the batches' separate matrices — checked by
host/label_batches_check.cpp against the single-batch cell functions, as a stand-alone program under the address and
undefined-behaviour sanitizers; and the harness of the host classes through the compiler's host pass."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")

PER_BATCH = 4  # 1, 2, 13, 256
BATCHES = (1, 5, 32)
WIDTHS = 4  # 1, 4, 5, 32
# per (per_batch, n_batches): EQ, RANGE, SET x widths, BOX and BOX64 x 1..4 columns, SET_BOX x widths x 0..3 range columns
KINDS = 1 + 1 + WIDTHS + 2 * 4 + WIDTHS * 4


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    """its own binary, nothing preloaded, nothing loaded into Python"""
    exe = str(tmp_path_factory.mktemp("label_batches") / "label_batches_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HOST, "label_batches_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout.strip().splitlines()


def test_label_batches_check_runs_clean_under_sanitizers(check_output):
    """the program itself compares the launch's table with the single-batch tables, cell for cell, for every kind"""
    assert check_output[-1] == "label batches check ok"
    assert not [line for line in check_output if line.startswith("FAILED")]


def test_label_batches_check_counts_its_cases(check_output):
    """every combination the program is meant to run has run: the four batch sizes x 1 / 5 / 32 batches x every kind and shape;
    the mapping at three rows of every batch, the offsets at four queries of every table"""
    tables = PER_BATCH * len(BATCHES) * KINDS
    assert "table cases %d" % tables in check_output
    assert "map cases %d" % (PER_BATCH * sum(BATCHES) * 3 + tables * 4) in check_output


def test_label_pipeline_harness_compiles():
    """hipcc, host pass only: the harness names the new entry points and the new methods of both host classes"""
    subprocess.check_call(["hipcc", "-std=c++17", "-fsyntax-only", "-Wall", "--offload-arch=gfx950",
                           os.path.join(HOST, "label_pipeline_harness.cpp")])
