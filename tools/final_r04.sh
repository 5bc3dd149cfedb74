#!/bin/bash
# Round-4 bench lines on the MI355X box (run from the repo root through gpurun); one JSON line + kernel table per configuration.
OUT=gpurun_out/final_r04; mkdir -p $OUT
run() { name=$1; shift; python bench.py --full "$@" --kernel-table $OUT/kt_$name.json > $OUT/$name.json 2> $OUT/$name.err; tail -1 $OUT/$name.json | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('$name', round(d['value'],2), d['unit'], 'ms/step', round(d['ms_per_step'],1), d.get('conv_engine',{}).get('avg_tflops'))" || tail -3 $OUT/$name.err; }
run flex_fp32 --model flex --no-cpu-baseline
run lhbdc_fp16 --precision fp16 --no-cpu-baseline
run icip_fp16 --model icip2024 --precision fp16 --no-cpu-baseline
run icip_fp16_2160p --model icip2024 --precision fp16 --resolution 2160p --no-cpu-baseline
run flex_fp16 --model flex --precision fp16 --no-cpu-baseline
run icip_fp32 --model icip2024 --no-cpu-baseline
run lhbdc_fp16_2160p --precision fp16 --resolution 2160p --no-cpu-baseline
