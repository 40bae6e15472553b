# developer tool (GPU box): step time of BASELINE cfg 2 for several sub-chunk ramps / sub-chunk sizes (lib_sub<N>.so built with
# -DRN_SUB_FRAMES=N -DCRISPY_DEV_KNOBS).  Every ramp grows by at most 1.5x per step (crispy_api.cpp: sub_frames).
run() { echo "== lib $(basename ${1:-default}) ramp $2"; CRISPY_HIP_LIB=$1 CRISPY_RN_RAMP=$2 timeout -k 10 100 python tools/step_timeline.py 2>&1 | grep -E "frame-kernel sum" || return 1; }
V=$PWD/crispy_amd/csrc/build/variants
for rep in 1 2 3; do
run $V/lib_sub12.so "3,4,5,7,10" || exit 1
run $V/lib_sub12.so "3,4,6,9" || exit 1
run $V/lib_sub16.so "3,4,6,9,13" || exit 1
run $V/lib_sub20.so "3,4,6,9,13,19" || exit 1
run $V/lib_sub24.so "3,4,6,9,13,19" || exit 1
run $V/lib_sub24.so "3,4,5,7,10,15,22" || exit 1
done
