"""CPU test of the int8 bound tiles' upper bound (csrc/exact_codes_bound.h) through tests/exact_codes_probe.cpp: U is never below
the float64 distance plus the engine's rounding term, what it gives away stays within the reported slack, and records without a
bound give +inf."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "duckdb-vss_amd", "csrc")


@pytest.fixture(scope="module")
def probe():
    src = os.path.join(HERE, "exact_codes_probe.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("exact_codes_bound.h", "exact_range_codes.h", "exact_range.h",
                                                    "exact_certificate.h", "row_codes.h", "prescore_bound.h")]
    out = os.path.join(HERE, "exact_codes_probe")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", src, "-o", out])
    return out


@pytest.mark.parametrize("dim", [32, 160, 768])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_the_upper_bound_is_above_every_distance(probe, metric, dim):
    text = subprocess.run([probe, str(metric), str(dim), str(9000 + 10 * dim + metric)], check=True, capture_output=True,
                          text=True).stdout
    lines = [line.split() for line in text.splitlines()]
    assert [line[0] for line in lines] == ["0.001", "1", "1000", "slack", "guards"]
    for scale, pairs, bad in lines[:3]:
        assert int(pairs) == 256 and int(bad) == 0, (metric, dim, scale)
    assert lines[3][1:] == ["256", "0"], lines[3]  # U - d within range_codes_slack on N(0, 1) rows
    assert lines[4][1:] == ["18", "0"], lines[4]
