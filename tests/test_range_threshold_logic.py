"""CPU tests of the exact range search's score threshold (duckdb-vss_amd/csrc/exact_range.h) through the stand-alone program
tests/range_threshold_probe.cpp: no pair whose float64 distance is within the radius has an f32 ranking score above its
query's threshold — the dot product summed in one accumulator and in wave order — on random, unit-norm and offset-2048 data;
the threshold is +inf exactly where the certificate has no finite error bound (rows of norm 2^41 and more)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
METRICS = {"l2sq": 0, "cosine": 1, "ip": 2}


@pytest.fixture(scope="module")
def probe():
    src = os.path.join(HERE, "range_threshold_probe.cpp")
    hdrs = [os.path.join(ROOT, "duckdb-vss_amd", "csrc", h) for h in ("exact_range.h", "exact_certificate.h")]
    out = os.path.join(HERE, "range_threshold_probe")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + hdrs):
        flags = ["-std=c++17", "-O2", "-ffp-contract=off"]
        try:  # fmaf as one instruction where the processor has it (the library call is exact too, only slower)
            if " fma " in open("/proc/cpuinfo").read():
                flags.append("-mfma")
        except OSError:
            pass
        subprocess.check_call(["g++"] + flags + [src, "-o", out])

    def run(metric, dim, seed):
        text = subprocess.run([out, "run", str(METRICS[metric]), str(dim), str(seed)], check=True, capture_output=True, text=True).stdout
        rows = {}
        for line in text.splitlines():
            name, queries, matching, violations, inf_mismatches, without_e, kept = line.split()
            rows[name] = dict(queries=int(queries), matching=int(matching), violations=int(violations),
                              inf_mismatches=int(inf_mismatches), without_e=int(without_e), kept=float(kept))
        return rows
    return run


@pytest.mark.parametrize("dim", [64, 100, 768])
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_no_matching_pair_scores_above_the_threshold(probe, metric, dim):
    rows = probe(metric, dim, 7 * dim + METRICS[metric])
    assert set(rows) == {"random", "unit", "offset2048", "huge"}
    for name, r in rows.items():
        assert r["violations"] == 0 and r["inf_mismatches"] == 0, (metric, dim, name, r)
        assert r["matching"] > 0, (metric, dim, name, r)  # (not vacuous)
        assert r["without_e"] == (r["queries"] if name == "huge" else 0), (metric, dim, name, r)
    # the threshold does reject: on ordinary data it keeps little more than the matching pairs (about 0.31 of all triples here)
    assert rows["random"]["kept"] < 0.4 and rows["unit"]["kept"] < 0.4, (metric, dim, rows)
    assert rows["huge"]["kept"] == 1.0
