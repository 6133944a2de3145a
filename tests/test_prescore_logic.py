"""CPU tests of the pre-scoring bound (duckdb-vss_amd/csrc/prescore_bound.h), the row encoder's arithmetic and the staleness
bookkeeping (duckdb-vss_amd/csrc/row_codes.h) through the stand-alone program tests/prescore_probe.cpp: the bound never
exceeds the engine's f32 distance, whatever the summation order of either; degenerate inputs get no bound; the stored
residual norm is an upper bound of the real one."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
PAIRS = 1500  # per case: ten cases x three orders of the bound x three orders of the distance each
METRICS = {"l2sq": 0, "cosine": 1, "ip": 2}


@pytest.fixture(scope="module")
def probe():
    src = os.path.join(HERE, "prescore_probe.cpp")
    hdrs = [os.path.join(ROOT, "duckdb-vss_amd", "csrc", h) for h in ("prescore_bound.h", "row_codes.h")]
    out = os.path.join(HERE, "prescore_probe")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + hdrs):
        flags = ["-std=c++17", "-O2", "-ffp-contract=off"]
        try:  # fmaf as one instruction where the processor has it (the library call is exact too, only slower)
            if " fma " in open("/proc/cpuinfo").read():
                flags.append("-mfma")
        except OSError:
            pass
        subprocess.check_call(["g++"] + flags + [src, "-o", out])

    def run(*args):
        text = subprocess.run([out] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout
        return [line.split() for line in text.splitlines()]
    return run


@pytest.mark.parametrize("dim", [512, 768, 1536])
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_bound_never_exceeds_the_f32_distance(probe, metric, dim):
    rows = {r[0]: r[1:] for r in probe("bound", METRICS[metric], dim, PAIRS, 1000 * dim + METRICS[metric])}
    assert set(rows) == {"random", "near", "multiples", "tiny_rows", "huge_rows", "tiny_queries", "huge_both", "dominant",
                         "small_rows", "large_both"}
    for name, (pairs, violations, bounded, worst) in rows.items():
        assert int(pairs) == PAIRS
        assert int(violations) == 0, (metric, dim, name, violations, worst)
        if name in ("random", "near", "multiples", "dominant", "small_rows", "large_both"):  # (not vacuous: every such pair does get a bound)
            assert int(bounded) == PAIRS, (metric, dim, name, bounded)
            assert float(worst) >= 0.0


@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_degenerate_inputs_get_no_bound(probe, metric):
    rows = {r[0]: (int(r[1]), int(r[2])) for r in probe("degenerate", METRICS[metric], 768)}
    assert rows.pop("control") == (1, 0)
    query_cases = {"zero_query", "denormal_query"}
    for name, (bounded, violated) in rows.items():
        assert violated == 0, (metric, name)
        # l2sq never looks at |q|: a zero or denormal query is an ordinary point there (and the bound still holds)
        if not (metric == "l2sq" and name in query_cases):
            assert bounded == 0, (metric, name)
    assert len(rows) == 9


@pytest.mark.parametrize("dim", [512, 768, 1536])
def test_stored_residual_norm_is_an_upper_bound(probe, dim):
    (rows, violations), = probe("residual", dim, 3000, dim)
    assert int(rows) == 3000 and int(violations) == 0


def test_staleness_bookkeeping(probe):
    (rounds, violations), = probe("stale", 3000, 7)
    assert int(rounds) == 3000 and int(violations) == 0
