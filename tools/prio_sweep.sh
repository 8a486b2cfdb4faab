#!/bin/bash
# issue-priority sweep on the default workload (diagnostic): PRF_PRIO = stage | busy<<2 | slack<<4 | flags<<6 | records<<8 | rows<<10 | hand-over<<12
# PRF_PRIO is read by the diagnostic build only (make -C colab-repeat-finder_amd/csrc EXTRA=-DPRF_DIAG BUILD=build_ab OUT=../libprf_diag.so)
# (the whole diagnostic build is 3-5 % slower than the product by its PRF_SKIP branches; PRF_PRIO and PRF_PLAN_W are read by plan.cpp
# alone, so the product's objects linked with a plan.o built with -DPRF_DIAG sweep the product kernel: profiles/scan_handover_notes.md)
export PRF_LIB=colab-repeat-finder_amd/libprf_diag.so
mkdir -p gpurun_out/prio
for cfg in 0x3A82 0x0A02 0x0A42 0x0A82 0x0AC2 0x2A02 0x2A42 0x2A82 0x2AC2 0x1A82 0x3A82 0x3AC2 0x000 0xA00 0xE02 0xF02 0x3A83 0x3A86 0x3A8A 0x3A82; do
  PRF_PRIO=$cfg python bench.py --steps 20 --warmup 5 --no-cpu-baseline > gpurun_out/prio/$cfg.json 2>/dev/null
  PRF_PRIO=$cfg python bench.py --workload hg38-random --steps 20 --warmup 5 --no-cpu-baseline > gpurun_out/prio/r$cfg.json 2>/dev/null
  python - <<PY
import json
a=json.load(open('gpurun_out/prio/$cfg.json')); b=json.load(open('gpurun_out/prio/r$cfg.json'))
print('$cfg', 'standin kernel_ms', a['roofline']['kernel_ms'], a['ms_per_step'], 'random kernel_ms', b['roofline']['kernel_ms'], b['ms_per_step'], flush=True)
PY
done
