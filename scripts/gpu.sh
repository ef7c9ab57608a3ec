# One runner for every GPU-box recipe (replaces rounds 3-5's one-off gpu_r*.sh;
# they are in the git history).  Run through gpurun from the repo root:
#   gpurun -- bash scripts/gpu.sh STEP[,STEP...] TAG [args]
# Steps (each under its own time limit; the chain stops at the first failure,
# and nothing more touches the GPU after it):
#   tests     pytest -m gpu                          -> gpurun_out/TAG_pytest.log
#   smoke     __graft_entry__.smoke()
#   luwork    LU work of the HC_DIAG_LUWORK build    -> TAG_lu_work.json
#   bench     the full bench line (bench.py --full)  -> TAG_bench.json
#   profile   kernel trace + PMC passes + summary    -> TAG_pmc_summary.json, TAG_kernel_stats.csv
#   traffic   kernel trace + FETCH/WRITE passes only -> TAG_pmc_summary.json
#   datasets  held-out datasets (scripts/datasets.py)-> TAG_datasets.jsonl
#   n2        bare `bench.py --full --gpus 2` rehearsal, both ranks on cuda:0 -> TAG_bench_n2_rehearsal.json
#   ab        interleaved A/B of builds: extra args NAME=lib/libX.so ... (package-relative)
#   ttfp_ab   time to the first pose of builds NAME=lib/libX.so ... (package-relative): the abort-mode
#             parity tests on each, then 3 interleaved rounds of scripts/ttfp.py (config 3 in both
#             semantics, 12 runs each; the lone sample, 12 runs)      -> TAG_ttfp.jsonl
#   phases    per-phase cycles of the HC_DIAG_PHASES build (scripts/diag_phases.py)
#   stress    time slicing under concurrent streams (scripts/slice_stress.py: 4 cold, 4 warm, 8 cold)
#   multi     T sequential single-triplet runs against one grouped run (scripts/multi_triplet.py) -> TAG_multi.json
#   joint     per-view against joint pose selection, config-5 protocol (scripts/joint_pose.py [TRIALS [REPS]]) -> TAG_joint.json
#   refine    the joint selection against the same selection refined on its inliers, config-5 protocol
#             (scripts/refine_pose.py [TRIALS [REPS]]) -> TAG_refine.json
#   topk      the refined joint winner against the best of the K refined top-K candidates, K = 1..16, config-5 protocol
#             (scripts/topk_refine.py [TRIALS [REPS]]) -> TAG_topk.json
#   gated     the gated abort launch against plain tracking + joint selection, config-5 protocol
#             (scripts/gated_stop.py [TRIALS]) -> TAG_gated.json
#   gated_ab  the launches that existed before the gated one (scripts/gated_stop.py --existing) on builds
#             NAME=lib/libX.so ... (package-relative), alternately, 2 rounds -> TAG_gated_existing.jsonl
#   adaptive  the gated launch's adaptive sample limit against a fixed budget and the ratio gate, config-5 protocol
#             (scripts/adaptive_stop.py [TRIALS]) -> TAG_adaptive.json
#   adaptive_ab  config 2, one sample and the gated launch on the noisy 300-sample data (scripts/adaptive_stop.py
#             --existing) on builds NAME=lib/libX.so ... (package-relative), alternately, 2 rounds -> TAG_adaptive_existing.jsonl
#   scale     the relative scale fitted by three-view transfer support, config-5 protocol, selection by joint count
#             against selection by transfer count, and the cost of the scale step (scripts/scale_fit.py [TRIALS [REPS]])
#             -> TAG_scale.json
#   scale_ab  the refine calls with the scale mode off (scripts/scale_fit.py --existing) on builds NAME=lib/libX.so ...
#             (package-relative), alternately, 3 rounds -> TAG_scale_existing.jsonl
#   threeview the three-view refinement after the two-view refinement and the scale vote, config-5 protocol: verdicts,
#             rotation residuals, scale error and transfer inliers without and with the stage, and its cost
#             (scripts/threeview_fit.py [TRIALS [REPS]]) -> TAG_threeview.json
#   threeview_ab  the refine calls with the modes off (scripts/threeview_fit.py --existing) on builds NAME=lib/libX.so ...
#             (package-relative), alternately, 3 rounds -> TAG_threeview_existing.jsonl; config 2 and one sample: the ab step
#   structure the 3D edgels of the selected pose on the config-5 protocol: count, tangents and oriented per size, the median
#             sin3 on runs that pass and that fail the GT check, and the stage's cost against the same call in three-view
#             mode (scripts/structure_fit.py [TRIALS [REPS]]) -> TAG_structure.json
#   structure_ab  the refine calls with the modes off (scripts/threeview_fit.py --existing) on builds NAME=lib/libX.so ...
#             (package-relative), alternately, 3 rounds -> TAG_structure_existing.jsonl; config 2 and one sample: the ab step
#   p2c       the ablation ladder from the archived P2C tracker up: P2C, PH, PH_CodeOpt and the headline launch
#             alternately on config 2 (scripts/ablation_p2c.py [--reps R]) -> TAG_ablation_p2c.json
#   validate  tests,luwork,bench,profile,datasets
# Extra environment: BENCH_ARGS (bench step), AB_ROUNDS (ab step, default 3), AB_ARGS (more ab_track.py options), TTFP_ARGS (ttfp_ab step,
# e.g. "--dataset 10").
export TMPDIR=/tmp
cd ${GRAFT_REPO_ROOT:-$(dirname "$0")/..}
STEPS=$1; T=$2; shift 2
O=gpurun_out
L=$PWD/trifocal_pose_estimation_using_improved_gpuhc_amd/lib
P=$PWD/trifocal_pose_estimation_using_improved_gpuhc_amd
mkdir -p $O
[ "$STEPS" = validate ] && STEPS=tests,luwork,bench,profile,datasets
ver() { python -c 'import sys; sys.path.insert(0,"."); from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi; print(_abi.build_id())'; }
run() {   # run NAME SECONDS CMD...: one GPU step under its own limit
  local n=$1 s=$2; shift 2
  echo "[$n] $(date +%T) start" >&2
  timeout -k 10 $s "$@"; local rc=$?
  echo "[$n] $(date +%T) rc=$rc" >&2
  return $rc
}
for step in ${STEPS//,/ }; do
  case $step in
    tests) run tests 900 python -u -m pytest tests -m gpu -x -v --timeout 200 --timeout-method thread > $O/${T}_pytest.log 2>&1; rc=$?; tail -3 $O/${T}_pytest.log ;;
    smoke) run smoke 300 python -c 'import __graft_entry__ as g; g.smoke()'; rc=$? ;;
    luwork) HC_TRIFOCAL_LIB=$L/libhc_trifocal_luwork.so run luwork 200 python scripts/lu_work.py > $O/${T}_lu_work.json; rc=$?; cat $O/${T}_lu_work.json ;;
    bench) run bench 600 python bench.py --full $BENCH_ARGS > $O/${T}_bench.json 2> $O/${T}_bench.err; rc=$?; cat $O/${T}_bench.json ;;
    profile|traffic)
      B="python bench.py --full --steps 30 --warmup 3 --no-cpu-baseline --no-small-launch --abort-samples 0 --noisy-trials 0 --streams 1 --pipelined-streams 0"
      run trace 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/${T}_trace -o run -- $B > $O/${T}_trace.log 2>&1; rc=$?
      if [ $step = profile ]; then
        SETS=("SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_INSTS_LDS SQ_WAIT_INST_ANY SQ_WAIT_ANY"
              "SQC_ICACHE_MISSES SQC_ICACHE_HITS SQ_INSTS_SALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR"
              "SQ_INSTS_SMEM SQ_ACTIVE_INST_SCA SQ_INSTS_BRANCH SQ_ACTIVE_INST_MISC SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INST_LEVEL_LDS SQ_IFETCH"
              "FETCH_SIZE" "WRITE_SIZE"
              "TCC_HIT_sum TCC_MISS_sum" "TCC_REQ_sum TCC_READ_sum" "TCP_TCC_READ_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum")
      else
        SETS=("FETCH_SIZE" "WRITE_SIZE")
      fi
      i=0
      for set in "${SETS[@]}"; do
        [ $rc -eq 0 ] || break
        i=$((i+1))
        run pmc$i 300 rocprofv3 --pmc $set --output-format csv -d $O/${T}_pmc$i -o run -- $B > $O/${T}_pmc$i.log 2>&1; rc=$?
      done
      if [ $rc -eq 0 ]; then
        python scripts/pmc_summary.py $T $O/${T}_pmc_summary.json > /dev/null; rc=$?
        cp $O/${T}_trace/run_kernel_stats.csv $O/${T}_kernel_stats.csv
      fi ;;
    datasets) run datasets 900 python scripts/datasets.py $L/libhc_trifocal_luwork.so "$@" > $O/${T}_datasets.jsonl; rc=$?; cat $O/${T}_datasets.jsonl ;;
    n2) HC_BENCH_DEVICE=0 HC_BENCH_BACKEND=gloo run n2 700 python3 bench.py --full --gpus 2 > $O/${T}_bench_n2_rehearsal.json 2> $O/${T}_bench_n2.err; rc=$?; cat $O/${T}_bench_n2_rehearsal.json ;;
    ab)
      args=""; last=""
      for kv in "$@"; do args="$args ${kv%%=*}=$P/${kv#*=}"; last=$P/${kv#*=}; done
      HC_TRIFOCAL_LIB=$last run ab_parity 600 python -u -m pytest tests/test_gpu_parity.py -x -q -m gpu --timeout 200 --timeout-method thread -k "not cli" > $O/${T}_parity.log 2>&1; rc=$?; tail -3 $O/${T}_parity.log
      [ $rc -eq 0 ] && { run ab 900 python -u scripts/ab_track.py $args --rounds ${AB_ROUNDS:-3} $AB_ARGS > $O/${T}_ab.jsonl; rc=$?; cat $O/${T}_ab.jsonl; } ;;
    ttfp_ab)
      rc=0
      for kv in "$@"; do
        HC_TRIFOCAL_LIB=$P/${kv#*=} run parity_${kv%%=*} 600 python -u -m pytest tests/test_gpu_configs.py tests/test_gpu_parity.py -x -q -m gpu --timeout 300 --timeout-method thread -k "abort or config3 or row_permuted" > $O/${T}_parity_${kv%%=*}.log 2>&1; rc=$?; tail -1 $O/${T}_parity_${kv%%=*}.log
        [ $rc -eq 0 ] || break
      done
      for rd in 0 1 2; do
        [ $rc -eq 0 ] || break
        for kv in "$@"; do
          for mode in "" "--inflight" "--samples 1"; do
            HC_TRIFOCAL_LIB=$P/${kv#*=} run ttfp 120 python scripts/ttfp.py 12 $mode $TTFP_ARGS > $O/${T}_tmp.json; rc=$?
            [ $rc -eq 0 ] || break 2
            python -c "import json,sys; d=json.load(open('$O/${T}_tmp.json')); d.update(build='${kv%%=*}', round=$rd); print(json.dumps(d))" >> $O/${T}_ttfp.jsonl
          done
        done
      done
      [ -f $O/${T}_ttfp.jsonl ] && python -c "
import json,collections
g=collections.defaultdict(list)
for l in open('$O/${T}_ttfp.jsonl'):
    d=json.loads(l); g[(d['build'],d['samples'],d['inflight_stop'])].append(d['median'])
for k,v in sorted(g.items()): print(k, v)" ;;
    phases) HC_TRIFOCAL_LIB=$L/libhc_trifocal_phases.so run phases 300 python scripts/diag_phases.py > $O/${T}_phases.json; rc=$?; cat $O/${T}_phases.json ;;
    multi) run multi 300 python scripts/multi_triplet.py "$@" > $O/${T}_multi.json; rc=$?; cat $O/${T}_multi.json ;;
    joint) run joint 600 python scripts/joint_pose.py "$@" > $O/${T}_joint.json; rc=$?; cat $O/${T}_joint.json ;;
    refine) run refine 600 python scripts/refine_pose.py "$@" > $O/${T}_refine.json; rc=$?; tail -c 1500 $O/${T}_refine.json ;;
    topk) run topk 600 python scripts/topk_refine.py "$@" > $O/${T}_topk.json; rc=$?; tail -c 1500 $O/${T}_topk.json ;;
    gated) run gated 900 python scripts/gated_stop.py "$@" > $O/${T}_gated.json; rc=$?; tail -c 600 $O/${T}_gated.json ;;
    adaptive) run adaptive 900 python scripts/adaptive_stop.py "$@" > $O/${T}_adaptive.json; rc=$?; tail -c 600 $O/${T}_adaptive.json ;;
    adaptive_ab)
      rc=0
      for rd in 0 1; do
        for kv in "$@"; do
          HC_TRIFOCAL_LIB=$P/${kv#*=} run existing_${kv%%=*} 200 python scripts/adaptive_stop.py --existing > $O/${T}_tmp.json; rc=$?
          [ $rc -eq 0 ] || break 2
          python -c "import json; d=json.load(open('$O/${T}_tmp.json')); d.update(build='${kv%%=*}', round=$rd); print(json.dumps(d))" >> $O/${T}_adaptive_existing.jsonl
        done
      done
      [ -f $O/${T}_adaptive_existing.jsonl ] && cat $O/${T}_adaptive_existing.jsonl ;;
    scale) run scale 900 python scripts/scale_fit.py "$@" > $O/${T}_scale.json; rc=$?; tail -c 600 $O/${T}_scale.json ;;
    scale_ab)
      rc=0
      for rd in 0 1 2; do
        for kv in "$@"; do
          HC_TRIFOCAL_LIB=$P/${kv#*=} run existing_${kv%%=*} 200 python scripts/scale_fit.py --existing > $O/${T}_tmp.json; rc=$?
          [ $rc -eq 0 ] || break 2
          python -c "import json; d=json.load(open('$O/${T}_tmp.json')); d.update(build='${kv%%=*}', round=$rd); print(json.dumps(d))" >> $O/${T}_scale_existing.jsonl
        done
      done
      [ -f $O/${T}_scale_existing.jsonl ] && cat $O/${T}_scale_existing.jsonl ;;
    threeview) run threeview 900 python scripts/threeview_fit.py "$@" > $O/${T}_threeview.json; rc=$?; tail -c 600 $O/${T}_threeview.json ;;
    threeview_ab)
      rc=0
      for rd in 0 1 2; do
        for kv in "$@"; do
          HC_TRIFOCAL_LIB=$P/${kv#*=} run existing_${kv%%=*} 200 python scripts/threeview_fit.py --existing > $O/${T}_tmp.json; rc=$?
          [ $rc -eq 0 ] || break 2
          python -c "import json; d=json.load(open('$O/${T}_tmp.json')); d.update(build='${kv%%=*}', round=$rd); print(json.dumps(d))" >> $O/${T}_threeview_existing.jsonl
        done
      done
      [ -f $O/${T}_threeview_existing.jsonl ] && cat $O/${T}_threeview_existing.jsonl ;;
    structure) run structure 900 python scripts/structure_fit.py "$@" > $O/${T}_structure.json; rc=$?; tail -c 600 $O/${T}_structure.json ;;
    structure_ab)
      rc=0
      for rd in 0 1 2; do
        for kv in "$@"; do
          HC_TRIFOCAL_LIB=$P/${kv#*=} run existing_${kv%%=*} 200 python scripts/threeview_fit.py --existing > $O/${T}_tmp.json; rc=$?
          [ $rc -eq 0 ] || break 2
          python -c "import json; d=json.load(open('$O/${T}_tmp.json')); d.update(build='${kv%%=*}', round=$rd); print(json.dumps(d))" >> $O/${T}_structure_existing.jsonl
        done
      done
      [ -f $O/${T}_structure_existing.jsonl ] && cat $O/${T}_structure_existing.jsonl ;;
    p2c) run p2c 300 python scripts/ablation_p2c.py --out $O/${T}_ablation_p2c.json "$@"; rc=$? ;;
    gated_ab)
      rc=0
      for rd in 0 1; do
        for kv in "$@"; do
          HC_TRIFOCAL_LIB=$P/${kv#*=} run existing_${kv%%=*} 200 python scripts/gated_stop.py --existing > $O/${T}_tmp.json; rc=$?
          [ $rc -eq 0 ] || break 2
          python -c "import json; d=json.load(open('$O/${T}_tmp.json')); d.update(build='${kv%%=*}', round=$rd); print(json.dumps(d))" >> $O/${T}_gated_existing.jsonl
        done
      done
      [ -f $O/${T}_gated_existing.jsonl ] && cat $O/${T}_gated_existing.jsonl ;;
    stress)
      run stress4 300 python scripts/slice_stress.py $O/${T}_stress4.jsonl 4 4 > /dev/null 2>&1; rc=$?
      [ $rc -eq 0 ] && { run stress4w 300 python scripts/slice_stress.py $O/${T}_stress4w.jsonl 4 4 --warm-streams > /dev/null 2>&1; rc=$?; }
      [ $rc -eq 0 ] && { run stress8 300 python scripts/slice_stress.py $O/${T}_stress8.jsonl 8 3 > /dev/null 2>&1; rc=$?; } ;;
    *) echo "unknown step $step"; rc=2 ;;
  esac
  [ $rc -eq 0 ] || { echo "step $step failed (rc=$rc): stopping"; exit $rc; }
done
echo "build $(ver)"
