"""CPU tests of the split-bf16 score's arithmetic (duckdb-vss_amd/csrc/split_bf16.h, exact_cert_error_split in
exact_certificate.h) through the stand-alone program tests/exact_split_probe.cpp, all in float64: hi + lo reconstructs x within
2^-16 |x|; the three kept terms are within the header's split term of q.x; accumulated in f32 in a shuffled order they are within
the whole score-side bound; the split form's E is never below the f32 form's and refuses exactly where it does."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "duckdb-vss_amd", "csrc")


@pytest.fixture(scope="module")
def probe():
    src = os.path.join(HERE, "exact_split_probe.cpp")
    deps = [src, os.path.join(CSRC, "exact_certificate.h"), os.path.join(CSRC, "split_bf16.h")]
    out = os.path.join(HERE, "exact_split_probe")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", src, "-o", out])
    return out


@pytest.mark.parametrize("dim", [32, 96, 768])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_split_score_is_within_its_bound(probe, metric, dim):
    text = subprocess.run([probe, str(metric), str(dim), str(9000 + 10 * dim + metric)], check=True, capture_output=True,
                          text=True).stdout
    lines = [line.split() for line in text.splitlines()]
    assert [line[0] for line in lines] == ["random", "offset", "alternating", "guards"]
    for kind, pairs, recon_bad, split_bad, total_bad, cert_bad, worst_split, worst_total in lines[:3]:
        print(kind, "worst split / bound %s, worst total / bound %s" % (worst_split, worst_total))
        assert int(pairs) == 256
        assert (int(recon_bad), int(split_bad), int(total_bad), int(cert_bad)) == (0, 0, 0, 0), (metric, dim, kind)
        assert 0.0 < float(worst_split) <= 1.0 and 0.0 < float(worst_total) <= 1.0
    assert int(lines[3][1]) > 0 and int(lines[3][2]) == 0, lines[3]
