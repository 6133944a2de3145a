"""The host side of vss_search_exact_batch_filtered_groups without a GPU: its plan and admission rule
(duckdb-vss_amd/csrc/exact_filtered_plan.h — the code the listing kernels and vss_engine.hip run) checked by
host/exact_filtered_check.cpp as a stand-alone program under the address and undefined-behaviour sanitizers, and the harness of
the host classes through the compiler's host pass."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "duckdb-vss_amd", "host")


def test_exact_filtered_check_runs_clean_under_sanitizers(tmp_path):
    """its own binary, nothing preloaded, nothing loaded into Python"""
    exe = str(tmp_path / "exact_filtered_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HOST, "exact_filtered_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == "exact filtered check ok"


def test_exact_filtered_harness_compiles():
    """hipcc, host pass only: the harness names the new entry points and the new methods of both host classes"""
    subprocess.check_call(["hipcc", "-std=c++17", "-fsyntax-only", "-Wall", "--offload-arch=gfx950",
                           os.path.join(HOST, "exact_filtered_harness.cpp")])
