"""CPU test of the int8 range tiles' pair test (csrc/exact_range_codes.h) through tests/range_codes_probe.cpp: against the true
float64 distance no pair within the radius is dropped, pairs far outside it are, records without a bound keep everything."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "duckdb-vss_amd", "csrc")


@pytest.fixture(scope="module")
def probe():
    src = os.path.join(HERE, "range_codes_probe.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("exact_range_codes.h", "exact_range.h", "exact_certificate.h", "row_codes.h",
                                                    "prescore_bound.h")]
    out = os.path.join(HERE, "range_codes_probe")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", src, "-o", out])
    return out


@pytest.mark.parametrize("dim", [32, 96, 768])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_no_pair_within_the_radius_is_dropped(probe, metric, dim):
    text = subprocess.run([probe, str(metric), str(dim), str(7000 + 10 * dim + metric)], check=True, capture_output=True,
                          text=True).stdout
    lines = [line.split() for line in text.splitlines()]
    assert [line[0] for line in lines] == ["random", "offset", "near", "halfstep", "limits", "guards"]
    for kind, pairs, bad, far_dropped in lines[:5]:
        print(kind, "dropped far outside the radius: %s of %s" % (far_dropped, pairs))
        assert int(pairs) == 256 and int(bad) == 0, (metric, dim, kind)
    assert int(lines[0][3]) > 128  # random pairs: the bound is no formality
    assert int(lines[5][1]) == 16 and int(lines[5][2]) == 0, lines[5]
