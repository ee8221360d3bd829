#!/bin/bash
# end of a round: profiles of every workload (tools/dev/profile.sh), then the full bench line (bench.py --full) into $LOG_DIR
cd ${GRAFT_REPO_ROOT:-.}
bash tools/dev/profile.sh > gpurun_out/profile_sh.log 2>&1
tail -8 gpurun_out/profile_sh.log | cut -c1-200
LOG_DIR=${LOG_DIR:-bench_logs}; mkdir -p "$LOG_DIR"
( time timeout 1500 python bench.py --full ) > "$LOG_DIR/final_bench.log" 2>&1
tail -c 300 "$LOG_DIR/final_bench.log"
