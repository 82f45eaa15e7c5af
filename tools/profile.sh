#!/bin/bash
# rocprofv3 evidence for one workload: kernel statistics (--kernel-trace --stats) or the counter passes (--pmc with the kernel
# trace and nothing else, one run per counter group).  Results land in $PROFILE_OUT/<tag>/ (default build/profile/<tag>/, which git
# ignores): kernel_stats_<target>.csv, or pmc_<target>.txt with the raw passes under pmc_<target>/ -- the layout
# tools/make_counters.py reads.  Copy what should be judged into profiles/.
# usage (on a GPU machine, from the repository root):  bash tools/profile.sh <tag> <target> [stats|pmc]
#        or, for any other command:                    bash tools/profile.sh <tag> <name> [stats|pmc] -- <command ...>
# Every GPU step runs under its own time limit, and the script ends at the first step whose status is not 0: after a fault or a
# hang nothing more is started on the card.
set -u
[ $# -ge 2 ] || { sed -n '2,9p' "$0"; exit 2; }
TAG=$1; TARGET=$2; MODE=${3:-stats}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${PROFILE_OUT:-$R/build/profile}/$TAG
cd "$R" || exit 1

# target -> the command whose kernels are timed (stats) | counted (pmc: a few launches are enough, every pass repeats them)
if [ "${4:-}" = "--" ]; then
  shift 4
  STATS=("$@"); PMC=("$@")
else
  STATS=(); PMC=()
  case $TARGET in
    headline)       STATS=(python bench.py --no-cpu --no-extras --min-seconds 0)
                    PMC=(python tools/run_headline_kernel.py 5 64 512 500 scan) ;;          # the dense kernel, as counters.json has it
    headline_dense) STATS=(python bench.py --no-cpu --no-extras --min-seconds 0 --sampler scan) ;;
    bench_default)  STATS=(python bench.py --full --no-cpu --min-seconds 0) ;;
    scan_sparse)    PMC=(python tools/run_headline_kernel.py 5 64 512 500 scan_sparse) ;;
    c5_sparse)      PMC=(python tools/run_headline_kernel.py 4 64 2048 1000 scan_sparse) ;;
    race)           PMC=(python tools/run_headline_kernel.py 4 64 512 500 race) ;;
    race_head)      PMC=(python tools/run_headline_kernel.py 4 64 512 500 race_head) ;;
    deposit_heads)  PMC=(python bench.py --no-cpu --no-extras --min-seconds 0 --steps 5 --precondition-seconds 0) ;;
    b1)             STATS=(python tools/b1_modes.py 100) ;;
    b1_lds_heads)   PMC=(python tools/b1_modes.py 20) ;;
    c2)             PMC=(python tools/measure_configs.py c2) ;;
    c4)             PMC=(python tools/measure_configs.py c4) ;;
    c5)             PMC=(python tools/measure_configs.py c5shard) ;;
    nls)            STATS=(python tools/run_nls_c3.py 64); PMC=("${STATS[@]}") ;;
    gnn)            STATS=(python tools/time_gnn_batch.py); PMC=(python tools/run_gnn_batch.py 500 50 64 3) ;;
    train)          STATS=(python tools/run_train_step.py 5) ;;
    siblings)       STATS=(python tools/measure_siblings.py) ;;
    cvrp_ls)        PMC=(python tools/measure_cvrp_ls.py 16) ;;
    hgs_ls)         STATS=(python tools/bench_hgs_ls.py --batch 64 --no-short); PMC=("${STATS[@]}" --reps 2) ;;
    *) echo "profile.sh: unknown target '$TARGET' (see the table in this script, or give a command after --)" >&2; exit 2 ;;
  esac
fi

# gfx950 has 8 SQ and 4 TCC counter slots per pass (FETCH_SIZE takes 3 of the TCC ones)
CGROUPS=("SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES"
         "SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS GRBM_GUI_ACTIVE"
         "FETCH_SIZE TCC_HIT_sum"
         "WRITE_SIZE TCC_MISS_sum TCC_REQ_sum"
         "TCP_TCC_READ_REQ_sum TCP_TCC_READ_REQ_LATENCY_sum SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE"
         "TA_TA_BUSY_sum TA_BUSY_avr TD_TD_BUSY_sum TD_TC_STALL_sum"
         "TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum")

step() {   # step <log> <seconds> <command ...>: one GPU program under its own time limit; its failure ends the script
  local log=$1 secs=$2; shift 2
  timeout -k 10 "$secs" "$@" > "$log" 2>&1
  local rc=$?
  if [ $rc -ne 0 ]; then
    echo "profile.sh: status $rc from: $* (log: $log) -- stopping here" >&2
    tail -5 "$log" >&2
    exit $rc
  fi
}

mkdir -p "$OUT" || exit 1
case $MODE in
  stats)
    [ ${#STATS[@]} -gt 0 ] || { echo "profile.sh: target '$TARGET' has no stats command" >&2; exit 2; }
    step "$OUT/stats_$TARGET.log" 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/stats_$TARGET" -o p -- "${STATS[@]}"
    cp "$OUT/stats_$TARGET/p_kernel_stats.csv" "$OUT/kernel_stats_$TARGET.csv" || exit 1
    ;;
  pmc)
    [ ${#PMC[@]} -gt 0 ] || { echo "profile.sh: target '$TARGET' has no pmc command" >&2; exit 2; }
    i=0
    for grp in "${CGROUPS[@]}"; do
      i=$((i+1))
      # shellcheck disable=SC2086  (the group is a list of counter names)
      step "$OUT/pmc_$TARGET.$i.log" 200 rocprofv3 --pmc $grp --kernel-trace --output-format csv -d "$OUT/pmc_$TARGET/pmc_${TARGET}_$i" -o p -- "${PMC[@]}"
    done
    python tools/pmc_summary.py "$OUT/pmc_$TARGET" daco > "$OUT/pmc_$TARGET.txt" || exit 1
    ;;
  *) echo "profile.sh: mode is stats or pmc, not '$MODE'" >&2; exit 2 ;;
esac
ls "$OUT"
