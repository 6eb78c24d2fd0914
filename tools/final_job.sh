# The end-of-round measurement run (through gpurun): full GPU suite, smoke(), the default bench under rocprofv3 --kernel-trace --stats
# (-> profiles/rNN_final_bench_n1.json + rNN_final_bench_kernel_stats.txt via tools/rocpd_stats.py), PMC counters on the bench's own launches,
# a plain bench, the other configurations.
set -x
export PYTHONPATH=$PWD/audio-mamba-aum_amd:$PYTHONPATH
JOB_OUT=${JOB_OUT:-job_out}      # this job's logs and results, relative to the repository root
mkdir -p $JOB_OUT/final
timeout 1500 python -m pytest tests -m gpu -x -q > $JOB_OUT/final/pytest_gpu.log 2>&1; tail -5 $JOB_OUT/final/pytest_gpu.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('SMOKE OK')" 2>&1 | tail -3
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
timeout 900 rocprofv3 --kernel-trace --stats -d /tmp/final_run -o bench -- python bench.py --full > $JOB_OUT/final/bench.json 2> $JOB_OUT/final/bench.err
tail -c 400 $JOB_OUT/final/bench.json
db=$(find /tmp/final_run -name "*.db" | head -1)
python tools/rocpd_stats.py $db $JOB_OUT/final/kernel_stats.txt | head -30
timeout 300 python bench.py --no-cpu-baseline > $JOB_OUT/final/bench_plain.json 2>/dev/null; python -c "import json;d=json.load(open('$JOB_OUT/final/bench_plain.json'));print('plain',d['ms_per_step'],d['value'])"
AUM_PMC_OUT=/tmp/pmc_tmb AUM_COMMIT=${AUM_COMMIT:-unknown} timeout 900 bash tools/pmc_tm_bench.sh bench > $JOB_OUT/final/pmc.log 2>&1; tail -30 $JOB_OUT/final/pmc.log
cp /tmp/pmc_tmb/pmc_traffic_tm.json /tmp/pmc_tmb/valu_busy_tm.json $JOB_OUT/final/ 2>/dev/null
timeout 900 python tools/variants_bench.py > $JOB_OUT/final/variants.log 2>&1; grep '"size"' $JOB_OUT/final/variants.log
