# per-phase cycle breakdown of enc_head_kernel: builds a second library with -DWCT_HEAD_TIMING
set -e
WCT_DEFS=-DWCT_HEAD_TIMING WCT_OUT=libwct_hip_timing.so bash collaborative-distillation_amd/build.sh
echo "built collaborative-distillation_amd/libwct_hip_timing.so; on the GPU box: WCT_LIB_PATH=\$PWD/collaborative-distillation_amd/libwct_hip_timing.so python tools/experiments/head_timing.py"
