"""The host plan of vss_search_range_batch_by_label_box64 (duckdb-vss_amd/csrc/range_filtered_plan.h) without a GPU, checked by
tests/range_filtered_plan_probe.cpp, a stand-alone program under the address and undefined-behaviour sanitizers: every (known
query, list position) pair in exactly one launch, every launch within the pair bound, no tile across a query-block boundary."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_range_filtered_plan_runs_clean_under_sanitizers(tmp_path):
    """its own binary, nothing preloaded, nothing loaded into Python"""
    exe = str(tmp_path / "range_filtered_plan_probe")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, "range_filtered_plan_probe.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == "range filtered plan ok"
