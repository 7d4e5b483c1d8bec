#!/bin/bash
# The A/B of the XCD mapping of the partition's consumers in one GPU visit: this library against the parent commit's
# (build/libfrlw_base.so; optionally build/libfrlw_v1.so, the first attempt with every consumer mapped) -- lab differential,
# per-kernel stats, FETCH_SIZE / WRITE_SIZE passes for every traffic file, output dumps, bench A/B with alternating arms.
# Output: $XCD_AB_OUT (default build/xcd_ab); tools/collect_xcd.py turns it into profiles/xcd_* and profiles/traffic_*.json.
set -u
R=$(pwd); K=${XCD_AB_OUT:-$R/build/xcd_ab}; mkdir -p $K; K=$(cd $K && pwd)
S=$(mktemp -d)   # raw traces stay outside the tree
T0=$(date +%s)
NEW=$R/frlw-evd_amd/csrc/libfrlw_evd.so; BASE=$R/build/libfrlw_base.so; V1=$R/build/libfrlw_v1.so
touch $NEW $R/frlw-evd_amd/csrc/libfrlw_evd_dev.so; find $R/oracle -name '*.so' -exec touch {} +
step() { local t=$1; shift; timeout -k 10 $t "$@"; local rc=$?; echo "rc=$rc t=$(( $(date +%s) - T0 ))s :: $*" | cut -c1-220; if [ $rc -ne 0 ]; then echo "STOP after rc=$rc"; exit $rc; fi; }
step 400 $R/build/enc_lab $BASE $NEW --cfg mpx,mpx_hot,mpx3,gen1,gen1x8,gen1x64,e2e64,small,ev1,evb1,evb64,evb64_hot,evb_small --reps 20 > $K/lab.txt 2>&1
grep -v "^evb.*per sequence" $K/lab.txt | awk '{print $1, $2, $3, $4}' | sed "s#$R/##"
step 100 $R/build/enc_lab $BASE $NEW --cfg evb1,evb_small --no-fadd --reps 20 > $K/lab_nofadd.txt 2>&1
awk '{print "no-fadd", $1, $2, $3, $4}' $K/lab_nofadd.txt | sed "s#$R/##"
cd $S && export TMPDIR=$S
prof() { # tag -- program args
  local tag=$1; shift; local O=$S/stats_$tag; rm -rf $O; mkdir -p $O
  step 200 rocprofv3 --kernel-trace --stats --output-format csv -d $O -o t -- "$@" > $O/run.log 2>&1
  cp "$(find $O -name '*kernel_stats.csv' | head -1)" $K/${tag}_kernel_stats.csv
}
pmc() { # tag -- program args   (counters in runs of their own: no other tracing next to them)
  local tag=$1; shift; local O=$S/pmc_$tag; rm -rf $O; mkdir -p $O/fetch $O/write
  step 200 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/fetch -o p -- "$@" > $O/fetch/run.log 2>&1
  step 200 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/write -o p -- "$@" > $O/write/run.log 2>&1
  python3 $R/tools/pmc_summary.py $O > $K/${tag}_pmc_summary.txt
}
prof parent_mpx_hot $R/build/enc_lab $BASE --cfg mpx_hot --reps 20
[ -f $V1 ] && prof v1_mpx_hot $R/build/enc_lab $V1 --cfg mpx_hot --reps 20
prof child_mpx_hot $R/build/enc_lab $NEW --cfg mpx_hot --reps 20
for c in mpx gen1 gen1x64 evb1 evb64 small; do
  prof parent_$c $R/build/enc_lab $BASE --cfg $c --reps 20
  prof child_$c $R/build/enc_lab $NEW --cfg $c --reps 20
done
prof parent_evb1_nofadd $R/build/enc_lab $BASE --cfg evb1 --no-fadd --reps 20
prof child_evb1_nofadd $R/build/enc_lab $NEW --cfg evb1 --no-fadd --reps 20
for W in sae eci; do
  export FRLW_LIB_PATH=$BASE; prof parent_$W python3 $R/tools/run_small_encoders.py $W 20
  export FRLW_LIB_PATH=$NEW; prof child_$W python3 $R/tools/run_small_encoders.py $W 20
done
for c in mpx mpx_hot gen1 gen1x64 evb1 evb64; do
  pmc child_$c $R/build/enc_lab $NEW --cfg $c --reps 3
  pmc parent_$c $R/build/enc_lab $BASE --cfg $c --reps 3
done
for W in sae eci; do
  export FRLW_LIB_PATH=$NEW; pmc child_$W python3 $R/tools/run_small_encoders.py $W 3
  export FRLW_LIB_PATH=$BASE; pmc parent_$W python3 $R/tools/run_small_encoders.py $W 3
done
echo "== profiles done t=$(( $(date +%s) - T0 ))s"
cd $R
lean="--no-detector --no-train --no-also --no-cpu-baseline"
for arm in parent child; do
  if [ $arm = parent ]; then export FRLW_LIB_PATH=$BASE; else export FRLW_LIB_PATH=$NEW; fi
  mkdir -p $K/dump_$arm
  step 200 python3 bench.py --gpus 1 --steps 5 --warmup 2 $lean --dump-outputs $K/dump_$arm > $K/dump_$arm.log 2>&1
done
cmp $K/dump_parent/taf_u8.npy $K/dump_child/taf_u8.npy && cmp $K/dump_parent/taf_state_sample.npy $K/dump_child/taf_state_sample.npy && echo "DUMPS CMP-EQUAL" || { echo "the two arms computed different outputs: stop"; exit 1; }
rm -rf $K/dump_parent $K/dump_child
# A/B rows: alternate parent / child on this box
ab() { # tag rounds timeout args...
  local tag=$1 n=$2 t=$3; shift 3
  for i in $(seq 1 $n); do
    for arm in parent child; do
      if [ $(( $(date +%s) - T0 )) -gt 1000 ]; then echo "deadline: $tag stops before round $i $arm"; return; fi
      if [ $arm = parent ]; then export FRLW_LIB_PATH=$BASE; else export FRLW_LIB_PATH=$NEW; fi
      step $t python3 bench.py "$@" > $K/ab_${tag}_${arm}_$i.log 2>&1
      grep '^{' $K/ab_${tag}_${arm}_$i.log | tail -1 > $K/ab_${tag}_${arm}_$i.json
    done
  done
}
ab gen1 5 120 --gpus 1 --workload taf_gen1 $lean
ab full 1 300 --gpus 1 --full --no-detector --no-train
echo "== lean rows done t=$(( $(date +%s) - T0 ))s"
ab head 5 200 --gpus 1
echo "xcd_ab done t=$(( $(date +%s) - T0 ))s"
