#!/bin/bash
# round-3 profile batch: kernel trace + stats of the driver command, CU-time budget, PMC traffic (separate passes), config 5
mkdir -p runs
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
rocprofv3 --kernel-trace --stats --output-format csv -d runs/prof_r3_driver -- python3 bench.py --full --steps 20 --warmup 5 > runs/prof_r3_driver.json 2> runs/prof_r3_driver.err
python scripts/kernel_stats.py runs/prof_r3_driver > runs/r3_kernel_stats_driver.txt
python scripts/cu_time_budget.py runs/prof_r3_driver 0.6 > runs/r3_cu_time_budget.txt 2>&1
echo "--- budget"; cat runs/r3_cu_time_budget.txt
rocprofv3 --kernel-trace --stats --output-format csv -d runs/prof_r3_default -- python3 bench.py --full --no-cpu-baseline > runs/prof_r3_default.json 2> runs/prof_r3_default.err
python scripts/kernel_stats.py runs/prof_r3_default > runs/r3_kernel_stats_default.txt
cp runs/prof_r3_default/*/*kernel_stats.csv runs/r3_rocprofv3_kernel_stats_default.csv
cp runs/prof_r3_driver/*/*kernel_stats.csv runs/r3_rocprofv3_kernel_stats_driver.csv
echo "--- stats (default schedule)"; head -14 runs/r3_kernel_stats_default.txt
rocprofv3 --pmc FETCH_SIZE --output-format csv -d runs/pmc_r3_fetch -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-roofline > /dev/null 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d runs/pmc_r3_write -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-roofline > /dev/null 2>&1
python scripts/pmc_summary.py runs/pmc_r3_fetch runs/pmc_r3_write runs/r3_pmc_traffic.json 3 4 > runs/r3_pmc_hbm_traffic.txt 2>&1
echo "--- pmc"; head -20 runs/r3_pmc_hbm_traffic.txt
