# Round-6 measurement pass on the committed tree: the driver's three steps (pytest -m gpu, smoke, bench), the C consumer,
# PMC traffic, kernel trace + idle gaps, the k-point workloads with their launch / synchronisation counts, secondary configs.
# Everything lands in gpurun_out/r06_final/; what should be judged is copied into profiles/.
# rocprofv3's own tear-down hangs on this pool after the application has exited (the result database is complete by
# then): every profiler run is bounded by `timeout -s KILL` and read back through tools/rocpd_*.py from the database.
R=$GRAFT_REPO_ROOT
O=$R/gpurun_out/r06_final
mkdir -p $O
cd $R
if [ "${SKIP_TESTS:-0}" != "1" ]; then
timeout 2400 python -m pytest tests -m gpu -q --tb=short --durations=8 -p no:cacheprovider 2>&1 \
  | grep -v '^RCCL version\|^HIP version\|^ROCm version\|^Hostname\|^Librccl path' > $O/r06_pytest_gpu.log
tail -14 $O/r06_pytest_gpu.log
fi
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1 | tee -a $O/r06_pytest_gpu.log
./tools/bin/abi_c_check 1 2>&1 | tail -3 | tee -a $O/r06_pytest_gpu.log
if [ "${SKIP_PMC:-0}" != "1" ]; then
cd /tmp && export TMPDIR=/tmp
ARGS="--no-cpu-baseline --no-complex-leg --no-random-start-leg --no-parity --no-amdahl-probe --prof-all"
export DFTK_MI_HEEV_PARTIAL=0
export PMC_NOTE="; Rayleigh-Ritz by the full Jacobi in these passes (DFTK_MI_HEEV_PARTIAL=0) so that all k_zgemm dispatches are booked zgemm calls; read back from the rocpd database (tools/rocpd_export_csv.py)"
rm -rf /tmp/pf /tmp/pw
timeout -s KILL 420 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d /tmp/pf -o pf -- python $R/bench.py --full $ARGS > /tmp/bench_f.json 2>/dev/null
timeout -s KILL 420 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d /tmp/pw -o pw -- python $R/bench.py --full $ARGS > /tmp/bench_w.json 2>/dev/null
python $R/tools/rocpd_export_csv.py $(ls /tmp/pf/*results.db | head -1) counters /tmp/pf.csv
python $R/tools/rocpd_export_csv.py $(ls /tmp/pw/*results.db | head -1) counters /tmp/pw.csv
python $R/tools/pmc_to_traffic.py /tmp/pf.csv /tmp/pw.csv /tmp/bench_f.json $O/r06_pmc_traffic.json
python $R/tools/pmc_summary.py /tmp/pf.csv FETCH_SIZE 24 > $O/r06_pmc_fetch_size.txt
python $R/tools/pmc_summary.py /tmp/pw.csv WRITE_SIZE 24 > $O/r06_pmc_write_size.txt
mkdir -p $R/profiles && cp $O/r06_pmc_traffic.json $R/profiles/ 2>/dev/null
unset DFTK_MI_HEEV_PARTIAL PMC_NOTE
rm -rf /tmp/pf /tmp/pw /tmp/pf.csv /tmp/pw.csv
fi
cd $R
( time timeout 1500 python bench.py --full --steps 20 --warmup 5 > $O/r06_bench_cfg5_driver_args.json 2> $O/bench_driver.err ) 2> $O/bench_driver.time
( time timeout 1500 python bench.py --full --no-cpu-baseline > $O/r06_bench_cfg5.json 2> $O/bench_cfg5.err ) 2> $O/bench_cfg5.time
python - <<'PY'
import json
for f in ("r06_bench_cfg5_driver_args", "r06_bench_cfg5"):
    d = json.loads(open(f"gpurun_out/r06_final/{f}.json").read().strip().splitlines()[-1])
    r, c = d["roofline"], d["config"]
    print(f, round(d["value"], 3), d.get("complex_iteration_value"), d["steps"], c["scf_wall_s"], c["converged"], round(r["frac"], 3), r["traffic"], (d.get("cpu_baseline") or {}).get("value"), c.get("parity_pass"), c.get("late_step_ms"), c.get("step_roofline_frac"), (d.get("amdahl") or {}).get("measured_speedup"))
PY
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/kt
timeout -s KILL 420 rocprofv3 --kernel-trace -d /tmp/kt -o p -- python $R/bench.py --full --no-cpu-baseline --no-complex-leg --no-random-start-leg --no-parity --no-amdahl-probe > /tmp/bench_kt.json 2>/tmp/bench_kt.err
DB=$(ls /tmp/kt/*results.db | head -1)
python $R/tools/rocpd_stats.py $DB 44 > $O/r06_kernel_trace_cfg5.txt
tail -1 /tmp/bench_kt.json >> $O/r06_kernel_trace_cfg5.txt
python $R/tools/rocpd_export_csv.py $DB kernel_trace /tmp/kt.csv
python $R/tools/trace_gaps.py /tmp/kt.csv 24 0.5 > $O/r06_trace_gaps_cfg5.txt
head -14 $O/r06_kernel_trace_cfg5.txt; head -6 $O/r06_trace_gaps_cfg5.txt
rm -rf /tmp/kt /tmp/kt.csv
cd $R
timeout 600 python bench.py --full --supercell 4 --no-cpu-baseline --no-complex-leg > $O/r06_bench_cfg2.json 2> $O/bench_cfg2.err
timeout 900 python bench.py --full --mode kpoints --system al --no-cpu-baseline > $O/r06_bench_kpoints_al.json 2> $O/bench_kpoints_al.err
for S in si graphene; do
  timeout 600 python bench.py --full --mode kpoints --system $S --no-cpu-baseline --no-amdahl-probe > $O/r06_bench_kpoints_$S.json 2> $O/bench_kpoints_$S.err
done
python - <<'PY'
import json
for f in ("r06_bench_cfg2", "r06_bench_kpoints_al", "r06_bench_kpoints_si", "r06_bench_kpoints_graphene"):
    try:
        d = json.loads(open(f"gpurun_out/r06_final/{f}.json").read().strip().splitlines()[-1])
        r = d["roofline"]
        print(f, round(d["value"], 2), d["steps"], d["config"]["scf_wall_s"], d["config"]["E_total"], r.get("bound"), r.get("launches_per_step"), r.get("host_syncs_per_step"), (d.get("amdahl") or {}).get("predicted_speedup"), (d.get("amdahl") or {}).get("measured_share_step_ms"), (d["config"].get("parity") or {}).get("pass"))
    except Exception as e:
        print(f, "failed", e)
PY
# the k-point share step: phase timers, launch / synchronisation counts, and the kernel trace of the same command
python tools/kpoints_share_profile.py 8 > $O/r06_kpoints_share_step_N8.txt 2>&1
python tools/kpoints_share_profile.py 1 >> $O/r06_kpoints_share_step_N8.txt 2>&1
cd /tmp; rm -rf /tmp/ks
timeout -s KILL 240 rocprofv3 --kernel-trace -d /tmp/ks -o s -- python $R/tools/kpoints_share_profile.py 8 --no-phase-timers > /dev/null 2>&1
python $R/tools/rocpd_stats.py $(ls /tmp/ks/*results.db | head -1) 30 > $O/r06_kernel_trace_kpoints_share8.txt
rm -rf /tmp/ks
cd $R
DFTK_MI_GEMM_SHAPES=1 timeout 300 python tools/late_step_profile.py 5 8 6 > $O/r06_late_step_cfg5.txt 2> $O/late.err
head -24 $O/r06_late_step_cfg5.txt
DFTK_MI_GEMM_SHAPES=1 timeout 300 python tools/late_step_profile.py 5 0 1 --any > $O/r06_first_step_cfg5.txt 2> $O/first.err
head -14 $O/r06_first_step_cfg5.txt
DFTK_MI_ORTHO_CLOCKS=1 timeout 120 python tools/ortho_small_bench.py 6 > $O/r06_ortho_kernel_phase_clocks.txt 2>&1
