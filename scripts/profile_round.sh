#!/bin/bash
# All rocprofv3 passes behind profiles/<tag>_*; run on the GPU box:
#   scripts/profile_round.sh r03                      headline workload, every pass
#   scripts/profile_round.sh r03 u8 --dtype u8        another BASELINE shape: kernel stats +
#                                                     FETCH/WRITE + SQ passes -> profiles/r03_u8_*
# The profiled command is `python bench.py --full --lean [args]` (the headline measurement and its
# own roofline figures only: the rest of --full also runs other datasets and the multi-shard point
# through the SAME kernel template, which would mix workloads in the per-kernel averages).  Counter
# passes never combine --pmc with the API-trace domains; each --pmc set is its own run.
# Raw rocprofv3 output goes to $OUT/<tag>[_sub]/ (default: runs/ in the repository root).
tag=${1:-r03}; shift
sub=""
if [ $# -gt 0 ]; then sub=$1; shift; fi
extra="$*"
R=$(cd "$(dirname "$0")/.." && pwd)
name=$tag${sub:+_$sub}
out=${OUT:-$R/runs}/$name
cd /tmp && export TMPDIR=/tmp
mkdir -p $out
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof -o bench -- \
  python $R/bench.py --full --lean --steps 20 --warmup 3 $extra > $out/bench_prof.json 2> $out/bench_prof.err
short="python $R/bench.py --full --lean --steps 3 --warmup 1 $extra"
pass() {  # name, counters...
  n=$1; shift
  rocprofv3 --pmc "$@" --kernel-trace --output-format csv -d $out/pmc_$n -o bench -- $short > /dev/null 2>&1
}
pass fetch FETCH_SIZE
pass write WRITE_SIZE
pass sq1 SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_WAVES
pass sq2 SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY
if [ -z "$sub" ]; then
  pass l2a TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum
  pass l2b TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum TCC_EA0_RDREQ_DRAM_sum TCC_BUBBLE_sum
  pass mfma SQ_WAVES SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F32
fi
cd $R && tail -1 $out/bench_prof.json > $out/bench_prof.tmp && mv $out/bench_prof.tmp $out/bench_prof.json
python scripts/summarize_profile.py $name $out "$extra"
