#!/bin/bash
# Round profile set (run on the GPU box from the repo root): bench line, rocprofv3 kernel stats, HBM-traffic PMC passes, MFMA-busy PMC pass.
# usage: bash tools/profile_round.sh r03      -> profile_out/...; then `python tools/summarize_profiles.py r03` condenses into profiles/
# (rocprofv3: the program itself directly after `--`; counters in their own passes, kernel-trace / stats only)
R=${1:-r03}
O=profile_out
export TMPDIR=/tmp
mkdir -p $O
python bench.py --full --steps 50 --warmup 10 > $O/bench_${R}_train.json 2> $O/bench_${R}_train.err
python bench.py --full --mode eval --steps 20 --warmup 5 --no-cpu-baseline > $O/bench_${R}_eval.json 2> $O/bench_${R}_eval.err
python bench.py --full --steps 30 --warmup 10 --no-cpu-baseline --no-eval-leg --emulate-world 8 > $O/bench_${R}_emu.json 2> $O/bench_${R}_emu.err
MHR_DIST_BACKEND=gloo python bench.py --gpus 2 --steps 20 --warmup 8 > $O/bench_${R}_dp2_gloo.json 2> $O/bench_${R}_dp2_gloo.err
MHR_FORCE_DP=1 python bench.py --full --steps 30 --warmup 10 --no-cpu-baseline --no-eval-leg --no-kernel-events > $O/bench_${R}_dp1_rccl.json 2> $O/bench_${R}_dp1_rccl.err
echo bench lines done
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_${R}_train -- python bench.py --steps 20 --warmup 5 > $O/prof1.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_${R}_eval -- python bench.py --mode eval --steps 20 --warmup 5 > $O/prof_eval.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_${R}_fetch -- python bench.py --no-graph --steps 4 --warmup 4 > $O/pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_${R}_write -- python bench.py --no-graph --steps 4 --warmup 4 > $O/pmc_write.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_${R}_eval_fetch -- python bench.py --mode eval --steps 4 --warmup 2 > $O/pmc_efetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_${R}_eval_write -- python bench.py --mode eval --steps 4 --warmup 2 > $O/pmc_ewrite.log 2>&1
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_${R}_mfma -- python bench.py --no-graph --steps 4 --warmup 4 > $O/pmc_mfma.log 2>&1
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_${R}_eval_mfma -- python bench.py --mode eval --steps 4 --warmup 2 > $O/pmc_emfma.log 2>&1
echo profile set done
