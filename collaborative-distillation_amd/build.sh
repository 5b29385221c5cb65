#!/bin/bash
# Build libwct_hip.so for gfx950 (cross-compiles without a GPU).  In-tree so that it travels with the repo snapshot.
# One object per source, compiled in parallel and only when the source or a header changed (build/ is git-ignored).
#   build.sh [-f]          -f: rebuild everything
#   WCT_DEFS="-DWCT_SP_TIMING" build.sh -f     instrumented builds (tools/experiments/*.sh)
set -e
cd "$(dirname "$0")"
SRC="conv3x3 conv3x3_f16 conv3x3_sp level1 moments solve misc transform rotate noise color smooth swap attn scale resize bgrid regions cluster blend video motion wct_api api_model api_sharded api_image api_multi api_swap api_attn api_video api_motion api_diverse api_bgrid jpeg api_jpeg jdec api_jdec"
HDR="csrc/wct_common.h csrc/conv_f16_dev.h csrc/mm_f64_dev.h csrc/philox_dev.h csrc/wct_ctx.h csrc/wct_clip.h ../include/wct_hip.h ../include/wct_hip_color.h ../include/wct_hip_guided.h ../include/wct_hip_scale.h ../include/wct_hip_smooth.h ../include/wct_hip_swap.h ../include/wct_hip_attn.h ../include/wct_hip_transform.h ../include/wct_hip_video.h ../include/wct_hip_motion.h ../include/wct_hip_diverse.h ../include/wct_hip_bgrid.h ../include/wct_hip_jpeg.h csrc/jpeg_tables.h ../include/wct_hip_jdec.h csrc/jdec_parse.h build.sh"
OUT=${WCT_OUT:-libwct_hip.so}
OBJ=build/obj${WCT_DEFS:+_$(echo "$WCT_DEFS" | md5sum | cut -c1-8)}
mkdir -p "$OBJ"
[ "$1" = "-f" ] && rm -f "$OBJ"/*.o
pids=""
for s in $SRC; do
  o="$OBJ/$s.o"
  stale=0
  [ -f "$o" ] || stale=1
  for f in csrc/$s.hip $HDR; do [ "$f" -nt "$o" ] && stale=1; done
  if [ $stale -eq 1 ]; then
    ( /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $WCT_DEFS -c csrc/$s.hip -o "$o.tmp" && mv "$o.tmp" "$o" ) &
    pids="$pids $!"
  fi
done
fail=0
for p in $pids; do wait $p || fail=1; done
[ $fail -eq 0 ] || { echo "compile failed"; exit 1; }
if [ -n "$pids" ] || [ ! -f "$OUT" ]; then
  objs=""; for s in $SRC; do objs="$objs $OBJ/$s.o"; done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -o "$OUT" $objs -ldl
  echo "built $(pwd)/$OUT"
else
  echo "libwct_hip.so up to date"
fi
