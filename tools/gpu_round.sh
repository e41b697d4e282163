#!/bin/bash
# One full GPU round: parity tests, smoke, bench, kernel-trace profile, PMC passes.
# Every GPU step has its own time limit; a crash/timeout ends the script.
cd "${GRAFT_REPO_ROOT:-/root/repo}" || exit 1
RUN_DIR=${CMPC_RUN_DIR:-run_out}   # where this script writes (kept out of git)
mkdir -p $RUN_DIR
TAG=${1:-r2}
timeout -k 10 900 python -u -m pytest tests -m gpu -q -rf --timeout 300 --timeout-method thread > $RUN_DIR/test_$TAG.log 2>&1
rc=$?; echo "pytest rc=$rc" >> $RUN_DIR/test_$TAG.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $RUN_DIR/smoke_$TAG.log 2>&1 || exit $?
timeout -k 10 900 python bench.py --full > $RUN_DIR/bench_$TAG.json 2> $RUN_DIR/bench_$TAG.err || exit $?
export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats -T -d $RUN_DIR/prof_$TAG -o run --output-format csv -- python3 bench.py --steps 50 --warmup 5 --full --no-cpu --headline-only --markers > $RUN_DIR/benchprof_$TAG.json 2> $RUN_DIR/benchprof_$TAG.err || exit $?
# the headline's timed steps and iterate pass cut from that trace (markers)
python3 tools/headline_pass_stats.py $RUN_DIR/prof_$TAG/run_kernel_trace.csv $RUN_DIR/benchprof_$TAG.json $RUN_DIR/bench_$TAG.json $RUN_DIR/headline_pass_$TAG.csv > $RUN_DIR/headline_pass_$TAG.txt 2>&1
# the SURVEY configs' own kernels (no headline launches in this trace): their
# --stats averages against the configs section of the bench line above
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $RUN_DIR/cfgprof_$TAG -o run --output-format csv -- python3 bench.py --full --configs-only --no-cpu > $RUN_DIR/cfgprof_$TAG.json 2> $RUN_DIR/cfgprof_$TAG.err || exit $?
pmc() {  # name, counters...   (separate passes, kernel trace only)
  local name=$1; shift
  timeout -k 10 300 rocprofv3 --kernel-trace -T --kernel-include-regex 'cmpc_' \
     --pmc "$@" -d $RUN_DIR/pmc${TAG}_$name -o run --output-format csv -- \
     python3 bench.py --full --steps 3 --warmup 1 --no-cpu --headline-only --settle-seconds 0 > $RUN_DIR/pmc${TAG}_$name.json 2> $RUN_DIR/pmc${TAG}_$name.err
}
pmc sq1 SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU || exit $?
pmc sq2 SQ_INSTS_LDS SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS GRBM_GUI_ACTIVE SQ_INSTS_VALU_FMA_F64 || exit $?
pmc fetch FETCH_SIZE || exit $?
pmc write WRITE_SIZE || exit $?
bash tools/gpu_dist_rehearsal.sh > $RUN_DIR/dist_$TAG.txt 2>&1 || exit $?
echo ALLDONE
