#!/bin/bash
# The acceptance run on a GPU box: build, smoke, GPU test suite, the full bench line, a kernel table of the same command.
#   usage: bash tools/gpu_check.sh [output directory, default gpu_check_out]
OUT=$(realpath -m ${1:-gpu_check_out})
mkdir -p $OUT
R=$(pwd)
python -c "import __graft_entry__ as g; g.build()" > $OUT/build.log 2>&1 || { tail -20 $OUT/build.log; exit 1; }
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | grep -v amdgpu.ids | tail -2
timeout 1800 python -m pytest tests -m gpu -q --maxfail=40 --tb=short -p no:cacheprovider > $OUT/pytest_gpu.log 2>&1
echo "pytest exit $?" >> $OUT/pytest_gpu.log
tail -3 $OUT/pytest_gpu.log; grep -E "^(E |FAILED|ERROR)" $OUT/pytest_gpu.log | head -10
timeout 900 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench_full.json 2> $OUT/bench_full.err
python - $OUT/bench_full.json <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
r = d['roofline']
print('bench: %.0f %s (%s), %.0f rooms/s fixed work (best %.0f at %s slots), %.1f us per step of a slot; roofline %.3f of fp32 MFMA peak in the loop (%s...), dense %.2f; cpu %.1f steps/s' % (
    d['value'], d['unit'], d['config']['formulation'], d['rooms_per_sec'], d.get('fixed_work_best', {}).get('rooms_per_sec', float('nan')),
    d.get('fixed_work_best', {}).get('slots_per_gpu'), d['us_per_instance_step_per_slot'], r['frac'], r['kernel'][:28], r['dense']['frac'],
    d.get('cpu_baseline', {}).get('value', float('nan'))))
PY
cd /tmp && export TMPDIR=/tmp && rm -rf /tmp/kt_d
timeout 900 rocprofv3 --kernel-trace --stats -d /tmp/kt_d -o kt --output-format csv -- python $R/bench.py --gpus 1 --steps 20 --warmup 5 --full --cpu-seconds 0 --p0-rooms 0 --best-slots "" --steady-slots "" --one-room-ks= > /tmp/kt_d.log 2>&1
cp $(ls /tmp/kt_d/*/*kernel_stats.csv /tmp/kt_d/*kernel_stats.csv 2>/dev/null | head -1) $OUT/bench_kernel_stats.csv
head -7 $OUT/bench_kernel_stats.csv | cut -c1-160
