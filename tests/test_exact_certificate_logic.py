"""CPU tests of the exact search's certificate (duckdb-vss_amd/csrc/exact_certificate.h) through the stand-alone program
tests/exact_cert_probe.cpp: whenever the certificate vouches for a query, the top-K' by ranking score holds the top-k of the
engine's f32 metric — with the score's dot product summed in three orders; the error bound E it rests on holds for every
(query, row) pair; it says no on the data built against the selection (a large common offset under l2sq, near-duplicate groups
under l2sq and cosine) and yes on ordinary data."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
METRICS = {"l2sq": 0, "cosine": 1, "ip": 2}
CASES = {"random", "unit", "offset2048", "offset8192", "scaled", "dominant", "near_duplicates"}


@pytest.fixture(scope="module")
def probe():
    src = os.path.join(HERE, "exact_cert_probe.cpp")
    hdr = os.path.join(ROOT, "duckdb-vss_amd", "csrc", "exact_certificate.h")
    out = os.path.join(HERE, "exact_cert_probe")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        flags = ["-std=c++17", "-O2", "-ffp-contract=off"]
        try:  # fmaf as one instruction where the processor has it (the library call is exact too, only slower)
            if " fma " in open("/proc/cpuinfo").read():
                flags.append("-mfma")
        except OSError:
            pass
        subprocess.check_call(["g++"] + flags + [src, "-o", out])

    def run(metric, dim, k, seed):
        text = subprocess.run([out, "run", str(METRICS[metric]), str(dim), str(k), str(seed)], check=True, capture_output=True,
                              text=True).stdout
        rows = {}
        for line in text.splitlines():
            name, order, queries, certified, lost, wrong, violations, worst = line.split()
            rows[(name, int(order))] = dict(queries=int(queries), certified=int(certified), lost=int(lost), wrong=int(wrong),
                                            violations=int(violations), worst=float(worst))
        return rows
    return run


@pytest.mark.parametrize("dim,k", [(64, 10), (100, 10), (100, 40), (768, 10)])
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "ip"])
def test_a_certified_query_has_lost_nothing(probe, metric, dim, k):
    rows = probe(metric, dim, k, 100 * dim + k)
    assert {name for name, _ in rows} == CASES and len(rows) == 3 * len(CASES)
    for (name, order), r in rows.items():
        assert r["queries"] == 8
        assert r["wrong"] == 0, (metric, dim, name, order, r)
        assert r["violations"] == 0 and r["worst"] <= 1.0, (metric, dim, name, order, r)
        if name in ("random", "unit"):  # (not vacuous: ordinary data is certified, every query)
            assert r["certified"] == 8 and r["lost"] == 0, (metric, dim, name, order, r)
    # the constructions of tests/test_gpu_exact_contract.py: no certificate, and the selection by score does lose rows
    hard = [("offset8192", "l2sq"), ("near_duplicates", "l2sq"), ("near_duplicates", "cosine")]
    for name, m in hard:
        if m == metric:
            assert all(rows[(name, order)]["certified"] == 0 for order in range(3)), (metric, dim, name)
            # (order 0: one f32 accumulator, like the MFMA's; the pairwise and the wave order lose rows on most of these, not all)
            assert rows[(name, 0)]["lost"] > 0, (metric, dim, name)
