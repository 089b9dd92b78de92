#!/usr/bin/env bash
# Regenerates round 2's judged artifacts under gpurun_out/profiles_r02 (copy into profiles/ afterwards).
# usage (GPU box): bash scripts/refresh_profiles_r02.sh [part ...]   parts: bench prof traffic ranks sift (default: all)
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/gpurun_out/profiles_r02
mkdir -p $out
parts=${*:-bench prof traffic ranks sift}
cd $root
has() { [[ " $parts " == *" $1 "* ]]; }
if has bench; then
  timeout -k 10 500 python bench.py --full > $out/r02_bench_20models.json 2>$out/bench20.err || { tail -3 $out/bench20.err; exit 1; }
  echo "bench 20 done"
  timeout -k 10 500 python bench.py --full --no-adaptive --no-cpu-baseline > $out/r02_bench_20models_no_adaptive.json 2>>$out/bench20.err || exit 1
  MH_MATCH_SCREEN=0 timeout -k 10 500 python bench.py --full --no-cpu-baseline --frames-per-step 256 > $out/r02_bench_20models_exact_f32_match.json 2>>$out/bench20.err || exit 1
  echo "bench 20 variants done"
  timeout -k 10 600 python bench.py --full --models 200 --frames-per-step 256 --steps 10 --warmup 2 > $out/r02_bench_200models.json 2>$out/bench200.err || { tail -3 $out/bench200.err; exit 1; }
  echo "bench 200 done"
  timeout -k 10 500 python bench.py --full --models 50 --depth-kind 1 --frames-per-step 512 > $out/r02_bench_50models_depth.json 2>$out/bench50.err || { tail -3 $out/bench50.err; exit 1; }
  timeout -k 10 500 python bench.py --full --models 50 --depth-kind 1 --moped3d-frontend --frames-per-step 512 --no-cpu-baseline > $out/r02_bench_50models_moped3d_frontend.json 2>$out/bench50f.err || { tail -3 $out/bench50f.err; exit 1; }
  timeout -k 10 500 python bench.py --full --models 50 --depth-kind 1 --moped3d-frontend --depthfill --frames-per-step 512 --no-cpu-baseline > $out/r02_bench_50models_moped3d_frontend_depthfill.json 2>$out/bench50d.err || { tail -3 $out/bench50d.err; exit 1; }
  echo "bench 50 done"
fi
if has prof; then
  cd /tmp && export TMPDIR=/tmp
  # the same command as the judged line under the profiler: default depth, and one frame on the chip at a time
  for d in default 1; do
    a=""; [ $d = 1 ] && a="--depth 1 --frames-per-step 128"
    rm -rf /tmp/rp_$d
    timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/rp_$d -- python3 $root/bench.py --full --no-cpu-baseline --h2d-steps 0 $a > $out/r02_bench_20models_depth${d}_under_rocprof.json 2>/tmp/rp_$d.err || { tail -3 /tmp/rp_$d.err; exit 1; }
    cp $(find /tmp/rp_$d -name "*kernel_stats.csv" | head -1) $out/r02_bench_20models_depth${d}_kernel_stats.csv
    echo "rocprof depth $d done"
  done
  rm -rf /tmp/rp_200
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/rp_200 -- python3 $root/bench.py --full --models 200 --depth 1 --frames-per-step 32 --steps 4 --warmup 1 --no-cpu-baseline --h2d-steps 0 > $out/r02_bench_200models_depth1_under_rocprof.json 2>/tmp/rp_200.err || { tail -3 /tmp/rp_200.err; exit 1; }
  cp $(find /tmp/rp_200 -name "*kernel_stats.csv" | head -1) $out/r02_bench_200models_depth1_kernel_stats.csv
  cd $root
fi
if has traffic; then
  # HBM traffic of the two-stage MATCH's kernels per launch (separate --pmc passes, never with a trace); FETCH_SIZE
  # doubled as MI355X_MICROARCH.md prescribes for gfx950
  cd /tmp && export TMPDIR=/tmp
  echo "{" > $out/traffic_r02.json
  for mq in "20 3000" "20 12000" "20 24000" "200 3000" "200 12000" "200 24000" "50 3000" "50 12000"; do
    set -- $mq; m=$1; q=$2
    for c in FETCH_SIZE WRITE_SIZE; do
      rm -rf /tmp/trs_$m$c
      timeout -k 10 300 rocprofv3 --pmc $c --output-format csv -d /tmp/trs_$m$c -- python3 $root/scripts/screen_probe.py $m $q 5 > /tmp/trs_$m$c.log 2>&1 || { tail -3 /tmp/trs_$m$c.log; exit 1; }
    done
    python3 - $m $q >> $out/traffic_r02.json <<'PY'
import csv, glob, sys, collections
m, q = sys.argv[1], sys.argv[2]
names = {"screen_b": "screen_kernel<1", "screen_a": "screen_kernel<0", "rescore": "rescore_kernel", "match": "match_mfma_kernel"}
res = {}
for c in ("FETCH_SIZE", "WRITE_SIZE"):
    f = glob.glob(f"/tmp/trs_{m}{c}/**/*counter_collection.csv", recursive=True)[0]
    rows = list(csv.DictReader(open(f)))
    for k, pat in names.items():
        v = [float(r["Counter_Value"]) for r in rows if pat in r["Kernel_Name"]]
        if v:
            res[(k, c)] = sum(v) / len(v)
for k in names:
    if (k, "FETCH_SIZE") in res:
        print(f' "{k}_{m}m_{q}q": {int(res[(k, "FETCH_SIZE")] * 1024 * 2)},')
        print(f' "_raw_{k}_{m}m_{q}q": "FETCH_SIZE {res[(k, "FETCH_SIZE")]:.1f} KB raw (x2 on gfx950), WRITE_SIZE {res.get((k, "WRITE_SIZE"), 0):.1f} KB per launch",')
PY
  done
  echo ' "_note": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE per launch over scripts/screen_probe.py (scripts/refresh_profiles_r02.sh traffic), KB*1024, FETCH doubled per MI355X_MICROARCH.md"' >> $out/traffic_r02.json
  echo "}" >> $out/traffic_r02.json
  cat $out/traffic_r02.json
  cd $root
  bash scripts/pmc_screen.sh gpurun_out/profiles_r02/r02_screen_sq_counters.txt 20 3000 "screen_kernel<1" > /dev/null 2>&1
fi
if has ranks; then
  # one GPU carrying what each rank carries at N = 8 / 4 / 2 (a DB of 20/N resp. 200/N models behind the exchange path)
  { for a in "--models 3 --force-exchange" "--models 5 --force-exchange" "--models 10 --force-exchange" "--models 3 --force-exchange --batch 1"; do
      echo "bench.py --full $a"; timeout -k 10 400 python bench.py $a --no-cpu-baseline --no-roofline 2>/dev/null | tail -1; done; } > $out/r02_per_rank_load_n8.txt 2>&1
  { for a in "--models 100 --frames-per-step 256 --steps 10" "--models 50 --frames-per-step 512" "--models 25"; do
      echo "bench.py --full $a --force-exchange"; timeout -k 10 500 python bench.py $a --force-exchange --no-cpu-baseline --no-roofline 2>/dev/null | tail -1; done; } > $out/r02_per_rank_load_200models.txt 2>&1
fi
if has sift; then
  # FEAT and the image -> objects path on the reference's bundled frames
  timeout -k 10 300 python tests/tools/sift_probe.py > $out/r02_sift_probe.txt 2>&1
  timeout -k 10 300 python scripts/image_frame_bench.py 20 16 3000 > $out/r02_image_frame_bench.txt 2>&1
  timeout -k 10 300 python scripts/image_frame_bench.py 20 4 3000 >> $out/r02_image_frame_bench.txt 2>&1
  timeout -k 10 300 python scripts/image_frame_bench.py 20 16 4000 4 >> $out/r02_image_frame_bench.txt 2>&1    # four images per MATCH launch sequence
  timeout -k 10 300 python scripts/image_frame_bench.py 20 16 4000 8 >> $out/r02_image_frame_bench.txt 2>&1
  GPU_MAX_HW_QUEUES=4 timeout -k 10 300 python scripts/image_frame_bench.py 20 16 3000 >> $out/r02_image_frame_bench.txt 2>&1   # ROCm's default queue count
  cd /tmp && export TMPDIR=/tmp
  rm -rf /tmp/rp_sift
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/rp_sift -- python3 $root/tests/tools/sift_probe.py > /tmp/rp_sift.log 2>&1
  cp $(find /tmp/rp_sift -name "*kernel_stats.csv" | head -1) $out/r02_sift_kernel_stats.csv
  cd $root
  timeout -k 10 300 python tests/tools/ms_bench.py > $out/r02_meanshift_bench.txt 2>&1
  # CLUSTER's phases (cycles of thread 0) on a -DMS_PROF build, if one lies beside the product:
  #   make -C moped_amd/csrc EXTRA=-DMS_PROF BUILD=build_prof OUT=../libmoped_hip_prof.so
  [ -f moped_amd/libmoped_hip_prof.so ] && MH_LIB_PATH=$root/moped_amd/libmoped_hip_prof.so timeout -k 10 300 python tests/tools/ms_prof.py > $out/r02_meanshift_phases.txt 2>&1
  timeout -k 10 300 python tests/tools/depthfill_bench.py > $out/r02_depthfill_bench.txt 2>&1
  # image -> objects kernel totals with 16 frames in flight
  cd /tmp
  rm -rf /tmp/rp_img
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/rp_img -- python3 $root/scripts/image_frame_bench.py 20 16 2000 > /tmp/rp_img.log 2>&1
  cp $(find /tmp/rp_img -name "*kernel_stats.csv" | head -1) $out/r02_image_frame_kernel_stats.csv
  cd $root
fi
ls -la $out
