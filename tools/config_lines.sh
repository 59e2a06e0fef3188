#!/bin/bash
# Headline bench line (with roofline and CPU baseline) and the secondary configuration lines, written to OUT
# (default: bench_out/; one .err log per line beside it).  Run on the GPU box:  bash tools/config_lines.sh [OUT] [TAG]
set -e
cd "$(dirname "$0")/.."
OUT=${1:-bench_out}; TAG=${2:-r03}
mkdir -p $OUT
python bench.py --full > $OUT/${TAG}_bench_line.json 2> $OUT/${TAG}_bench_line.err; tail -1 $OUT/${TAG}_bench_line.err
: > $OUT/${TAG}_config_lines.jsonl
python bench.py --full --stage 1 --no-cpu-baseline >> $OUT/${TAG}_config_lines.jsonl 2> $OUT/l1.err; tail -1 $OUT/l1.err
python bench.py --full --stage 1 --pairs-per-gpu 1024 --no-cpu-baseline >> $OUT/${TAG}_config_lines.jsonl 2> $OUT/l2.err; tail -1 $OUT/l2.err
python bench.py --full --vision-model openai/clip-vit-large-patch14 --text-model gpt2-large --seq-len 256 --pairs-per-gpu 64 --no-cpu-baseline --steps 5 --warmup 2 >> $OUT/${TAG}_config_lines.jsonl 2> $OUT/l3.err; tail -1 $OUT/l3.err
python bench.py --full --vision-model openai/clip-vit-large-patch14 --text-model gpt2-xl --seq-len 256 --pairs-per-gpu 32 --no-cpu-baseline --steps 5 --warmup 2 >> $OUT/${TAG}_config_lines.jsonl 2> $OUT/l4.err; tail -1 $OUT/l4.err
python bench.py --full --stage 1 --vision-model openai/clip-vit-large-patch14 --text-model gpt2-xl --seq-len 256 --pairs-per-gpu 128 --no-cpu-baseline --steps 5 --warmup 2 >> $OUT/${TAG}_config_lines.jsonl 2> $OUT/l5.err; tail -1 $OUT/l5.err
python bench.py --full --padded --pairs-per-gpu 256 --no-cpu-baseline >> $OUT/${TAG}_config_lines.jsonl 2> $OUT/l6.err; tail -1 $OUT/l6.err
