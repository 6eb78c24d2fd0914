# Round-end measurement recipe (run through gpurun): GPU parity tests, the default bench line, a per-kernel profile.
set -x
JOB_OUT=${JOB_OUT:-job_out}      # this job's logs and results, relative to the repository root
mkdir -p $JOB_OUT
export PYTHONPATH=$PWD/audio-mamba-aum_amd:$PYTHONPATH
timeout 900 python -m pytest tests -m gpu -x -q > $JOB_OUT/pytest_gpu.log 2>&1; echo "pytest rc=$?" >> $JOB_OUT/pytest_gpu.log
tail -5 $JOB_OUT/pytest_gpu.log
python bench.py --full > $JOB_OUT/bench_latest.json 2> $JOB_OUT/bench_latest.err; tail -1 $JOB_OUT/bench_latest.json
