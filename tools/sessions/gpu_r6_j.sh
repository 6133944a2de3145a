#!/bin/bash
# round 6, session J: the scoring waves' prologue — row chunk offsets as immediates (compile-time lane group for wide rows), the crew box in one
# LDS read — parity suite, crew probe, solo probe, phase ticks at limits of 257-512, c2, c5, the headline.
ulimit -c 0
cd ${GRAFT_REPO_ROOT:-/root/repo}
O=gpurun_out
export TMPDIR=/tmp
mkdir -p $O
(time timeout 1500 python -m pytest tests -m gpu -x -q -p no:cacheprovider --ignore tests/test_gpu_configs.py) > $O/r6j_pytest.txt 2>&1; echo "pytest rc $?"; tail -n 6 $O/r6j_pytest.txt | cut -c1-400
VSS_LIBRARY=$PWD/duckdb-vss_amd/libvssgpu_prof.so timeout 400 python tools/gpu_crew_probe.py 3000000 768 cosine 32 256 80 2>&1 | grep -v amdgpu > $O/r6j_crew_probe_3m768_prof.txt; echo "crew probe rc $?"
grep -A3 "^B=   1 \|^B= 204 " $O/r6j_crew_probe_3m768_prof.txt | grep "crews+pipe plain:\|^B=" | cut -c1-420
grep "per call" $O/r6j_crew_probe_3m768_prof.txt | grep "crews+pipe plain" | cut -c1-200
VSS_LIBRARY=$PWD/duckdb-vss_amd/libvssgpu_prof.so timeout 300 python tools/gpu_solo_phase_probe.py 1000000 128 l2sq 16 128 64 > $O/r6j_solo_phase_1m128_prof.txt 2>&1; echo "solo probe rc $?"
grep -v "amdgpu.ids" $O/r6j_solo_phase_1m128_prof.txt | cut -c1-330 | head -8
VSS_LIBRARY=$PWD/duckdb-vss_amd/libvssgpu_prof.so timeout 600 python tools/gpu_wide_list_probe.py 10000000 768 cosine 16 128 10 512,288 > $O/r6j_wide_lists_phase_ticks_10m768_prof.txt 2>&1; echo "wide probe rc $?"
grep -v "^built\|amdgpu.ids" $O/r6j_wide_lists_phase_ticks_10m768_prof.txt | grep -A1 "retry in place" | cut -c1-330
(time timeout 400 python bench.py --full --config c2 --steps 2000 --cpu-seconds 3 --sidecar $O/r6j_c2_sidecar.json) > $O/r6j_c2.jsonl 2> $O/r6j_c2.err; tail -n 1 $O/r6j_c2.jsonl | cut -c1-700
(time timeout 900 python bench.py --full --config c5 --steps 32 --warmup 16 --cpu-seconds 4 --sidecar $O/r6j_c5_sidecar.json) > $O/r6j_c5.jsonl 2> $O/r6j_c5.err; tail -n 1 $O/r6j_c5.jsonl | cut -c1-1200
(time timeout 900 python bench.py --full --gpus 1 --steps 20 --warmup 5 --extras none --cpu-seconds 4 --sidecar $O/r6j_c3_sidecar.json) > $O/r6j_c3.jsonl 2> $O/r6j_c3.err; grep '"detail": "regime"\|small_launches\|"detail": "repeat"' $O/r6j_c3.jsonl | cut -c1-400; tail -n 1 $O/r6j_c3.jsonl | cut -c1-1500
