#!/bin/bash
# Build the MI355X engine library: every .hip translation unit -> zeggs/libzeggs_hip.so (gfx950 only).
set -e
cd "$(dirname "$0")"
# measurement builds: ZEGGS_DEFS="-DZEGGS_TPSTAT" ZEGGS_OUT=../zeggs/libzeggs_alt.so ZEGGS_BUILD_DIR=build_v_alt bash build.sh ; load with
# ZEGGS_LIB=<path>  (the switches the sources test: tools/README.md, "Compile-time switches")
OUT=${ZEGGS_OUT:-../zeggs/libzeggs_hip.so}
BD=${ZEGGS_BUILD_DIR:-build}
mkdir -p $BD
pids=()
SRC="gemm gemm_split kernels attention encoders options decoder decoder_fast sweep_sync decode_persistent train_persistent train_dual train_bwd_persistent loudness loss misc mel anim spline prepare style_gru hostio text funcs mirror live live_loudness live_snapshot live_gaze live_plant live_styles live_refilter live_frames live_retime live_resample"
for f in $SRC; do
  stale=0
  [ -f $BD/$f.o ] || stale=1
  for dep in $f.hip *.h ../../include/zeggs_hip.h ../../include/zeggs_hip_live.h ../../include/zeggs_hip_loudness.h ../../include/zeggs_hip_resample.h ../../include/zeggs_hip_frames.h ../../include/zeggs_hip_retime.h ../../include/zeggs_hip_refilter.h ../../include/zeggs_hip_snapshot.h ../../include/zeggs_hip_gaze.h ../../include/zeggs_hip_styles.h ../../include/zeggs_hip_plant.h ../../include/zeggs_hip_mirror.h; do     # every header: one missing from a list means stale objects
    if [ $dep -nt $BD/$f.o ]; then stale=1; fi
  done
  if [ $stale = 1 ]; then
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result $ZEGGS_DEFS -c $f.hip -o $BD/$f.o &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
OBJ=""
for f in $SRC; do OBJ="$OBJ $BD/$f.o"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT $OBJ
echo "built $OUT"
