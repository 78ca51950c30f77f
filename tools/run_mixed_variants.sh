#!/bin/bash
# usage: run_variants.sh name...  -> error table for each build_variants/<name>.so
# (the lines and their stderr land beside the builds: build_variants/<name>.json, .err)
for v in "$@"; do
  MOD16_LIB=build_variants/$v.so timeout -k 10 200 python bench.py --full --dtype float32 --math mixed --no-cpu-baseline --no-plain --no-configs --steps 5 > build_variants/$v.json 2> build_variants/$v.err || exit 1
done
