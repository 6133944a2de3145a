#!/bin/bash
# round 3, GPU session E: solo shape with the look-ahead in the load shadow and a roomier visited set.
cd ${GRAFT_REPO_ROOT:-/root/repo}
O=gpurun_out
export TMPDIR=/tmp
(time timeout 600 python -m pytest tests -m gpu -x -q -p no:cacheprovider -k "not config and not full_benchmark") > $O/r3e_pytest.txt 2>&1; echo "pytest rc $?"; tail -n 3 $O/r3e_pytest.txt
timeout 300 python tools/gpu_solo_probe.py 1000000 128 l2sq 16 128 64 > $O/r3e_solo_1m128.txt 2>&1; echo "solo probe rc $?"; grep -E "single|  32:|1024|build" $O/r3e_solo_1m128.txt
VSS_LIBRARY=duckdb-vss_amd/libvssgpu_prof.so timeout 300 python tools/gpu_solo_phase_probe.py 1000000 128 l2sq 16 128 64 > $O/r3e_solo_phase_1m128.txt 2>&1; echo "phase probe rc $?"; cat $O/r3e_solo_phase_1m128.txt
(timeout 300 python bench.py --full --config c2) > $O/r3e_bench_c2.json 2> $O/r3e_bench_c2.err; echo "bench c2 rc $?"; tail -c 300 $O/r3e_bench_c2.err
python - <<'PY'
import json
try:
    r = json.loads([l for l in open("gpurun_out/r3e_bench_c2.json") if l.startswith("{")][-1])
    print("c2:", round(r["value"]), "q/s", round(r["ms_per_step"] * 1e3, 1), "us/call kernel", round(r["roofline"]["avg_kernel_ms"] * 1e3, 1), "us",
          round(r["roofline"]["us_per_expansion"], 2), "us/expansion; cpu", round(r["cpu_baseline"]["value"]), "build", round(r["build_rows_per_s"]))
except Exception as e:
    print("unreadable", e)
PY
