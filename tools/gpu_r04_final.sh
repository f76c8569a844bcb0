# Round-4 measurement pass on the committed tree: the driver's three steps (pytest -m gpu, smoke, bench), the C consumer,
# the kernel trace + idle-gap analysis, the two PMC traffic passes, secondary configs and kernel micro-benchmarks.
# Everything lands in gpurun_out/r04_final/; copy what should be judged into profiles/.
R=$GRAFT_REPO_ROOT
O=$R/gpurun_out/r04_final
mkdir -p $O
cd $R
timeout 2400 python -m pytest tests -m gpu -q --tb=short --durations=8 -p no:cacheprovider 2>&1 \
  | grep -v '^RCCL version\|^HIP version\|^ROCm version\|^Hostname\|^Librccl path' > $O/r04_pytest_gpu.log
tail -14 $O/r04_pytest_gpu.log
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1 | tee -a $O/r04_pytest_gpu.log
./tools/bin/abi_c_check 1 2>&1 | tail -2 | tee -a $O/r04_pytest_gpu.log
# PMC traffic first: the bench lines below then quote it (same build, same workload)
TAG=r04 timeout 1500 bash $R/tools/pmc_traffic_bench.sh > $O/pmc.log 2>&1
cp $R/gpurun_out/r04_pmc_traffic.json $R/gpurun_out/r04_pmc_fetch_size.txt $R/gpurun_out/r04_pmc_write_size.txt $O/ 2>/dev/null
mkdir -p $R/profiles && cp $R/gpurun_out/r04_pmc_traffic.json $R/profiles/ 2>/dev/null
tail -3 $O/pmc.log | cut -c1-300
cd $R
( time timeout 1500 python bench.py --full --steps 20 --warmup 5 > $O/r04_bench_cfg5_driver_args.json 2> $O/bench_driver.err ) 2> $O/bench_driver.time
( time timeout 1500 python bench.py --full > $O/r04_bench_cfg5.json 2> $O/bench_cfg5.err ) 2> $O/bench_cfg5.time
python - <<'PY'
import json
for f in ("r04_bench_cfg5_driver_args", "r04_bench_cfg5"):
    d = json.loads(open(f"gpurun_out/r04_final/{f}.json").read().strip().splitlines()[-1])
    r, c = d["roofline"], d["config"]
    print(f, round(d["value"], 3), d["steps"], c["scf_wall_s"], c["converged"], round(r["frac"], 3), r["traffic"], c["complex_iteration"]["value"], d["cpu_baseline"]["kind"], d["cpu_baseline"]["value"], c["parity"]["pass"], d["amdahl"]["predicted_speedup"])
PY
cd /tmp && export TMPDIR=/tmp
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/kt -o p -- python $R/bench.py --full --no-cpu-baseline --no-complex-leg --no-parity > /tmp/bench_kt.json 2>/tmp/bench_kt.err
python $R/tools/kernel_stats_txt.py /tmp/kt/p_kernel_stats.csv 40 > $O/r04_kernel_trace_cfg5.txt
tail -1 /tmp/bench_kt.json >> $O/r04_kernel_trace_cfg5.txt
python $R/tools/trace_gaps.py /tmp/kt/p_kernel_trace.csv 24 0.5 > $O/r04_trace_gaps_cfg5.txt
head -12 $O/r04_kernel_trace_cfg5.txt; head -6 $O/r04_trace_gaps_cfg5.txt
rm -rf /tmp/kt
cd $R
timeout 600 python bench.py --full --supercell 4 --no-cpu-baseline --no-complex-leg > $O/r04_bench_cfg2.json 2> $O/bench_cfg2.err
timeout 900 python bench.py --full --mode kpoints --system al --no-cpu-baseline > $O/r04_bench_kpoints_al.json 2> $O/bench_kpoints_al.err
for S in si graphene; do
  timeout 600 python bench.py --full --mode kpoints --system $S --no-cpu-baseline --no-amdahl-probe > $O/r04_bench_kpoints_$S.json 2> $O/bench_kpoints_$S.err
done
python - <<'PY'
import json
for f in ("r04_bench_cfg2", "r04_bench_kpoints_al", "r04_bench_kpoints_si", "r04_bench_kpoints_graphene"):
    try:
        d = json.loads(open(f"gpurun_out/r04_final/{f}.json").read().strip().splitlines()[-1])
        print(f, round(d["value"], 2), d["steps"], d["config"]["scf_wall_s"], d["config"]["E_total"], (d.get("amdahl") or {}).get("predicted_speedup"), (d["config"].get("parity") or {}).get("pass"))
    except Exception as e:
        print(f, "failed", e)
PY
DFTK_MI_GEMM_SHAPES=1 timeout 300 python tools/late_step_profile.py 5 8 6 > $O/r04_late_step_cfg5.txt 2> $O/late.err
timeout 300 python tools/fft_bench.py 5 64 2>&1 | grep -v amdgpu > $O/r04_fft_bench_192.txt
timeout 300 python tools/heev_bench.py real 503 1006 1509 2>&1 | grep -v amdgpu > $O/r04_heev_bench.txt
timeout 300 python tools/gemm_real_bench.py 264859 503 struct 2>&1 | grep -v amdgpu > $O/r04_gemm_struct_bench.txt
timeout 300 python tools/kpoints_share_profile.py 8 > $O/r04_kpoints_share_step_N8.txt 2>/dev/null
cat $O/r04_late_step_cfg5.txt | head -16; cat $O/r04_heev_bench.txt
timeout 300 python tools/potrf_bench.py 2>&1 | grep -v amdgpu > $O/r04_potrf_bench.txt
timeout 300 python tools/ew_bench.py 2>&1 | grep -v amdgpu > $O/r04_ew_bench.txt
cat $O/r04_potrf_bench.txt $O/r04_ew_bench.txt
