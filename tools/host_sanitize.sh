#!/bin/bash
# The CPU tier of the device code (tests/host/*.cpp: the blob extraction, the voting item, the tail geometry and the
# libstdc++ / glibc restatement, compiled for the host) under AddressSanitizer + UndefinedBehaviorSanitizer:
#   tools/host_sanitize.sh [pytest args]        (GPU sanitizers are not available on this pool; this is the CPU build)
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R
ASAN=$(g++ -print-file-name=libasan.so)   # (the test libraries are loaded by python: the ASan runtime must come first)
rc=0
for t in tests/test_k1b_host.py tests/test_geometry_host.py tests/test_ddmath_host.py tests/test_vote_host.py; do
  MPE_HOST_CXXFLAGS="-g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer" \
  LD_PRELOAD=$ASAN ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=print_stacktrace=1 \
    python -m pytest $t -x -q -p no:cacheprovider -s "$@" 2>&1 | grep -E "runtime error|ERROR: AddressSanitizer|passed|failed|error" || true
  [ ${PIPESTATUS[0]} -ne 0 ] && rc=1
done
# the block table of the mixed-set-up brute-force launch (csrc/mpe_brute_blocks.h): a stand-alone program with its own
# main, linked against the sanitizer runtimes itself
BB=$(mktemp -d)/brute_blocks_host
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
    -I rpg_monocular_pose_estimator_amd/csrc tests/host/brute_blocks_host.cpp -o $BB && $BB || rc=1
rm -rf "$(dirname $BB)"
# the peel-and-compact logic of k3_peel_wide (csrc/mpe_wide_peel.h) against the oracle's correspondencesFromHistogram: a
# stand-alone program as well, the oracle's (uninstrumented) shared library linked in
make -s -C oracle || rc=1
WP=$(mktemp -d)/wide_peel_host
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
    -I rpg_monocular_pose_estimator_amd/csrc tests/host/wide_peel_host.cpp -o $WP -L oracle -lmpe_oracle -Wl,-rpath,$R/oracle && $WP || rc=1
rm -rf "$(dirname $WP)"
# the nearest-neighbour correspondences of k_nn_wide (csrc/mpe_wide_nn.h), the 64-lane form against the plain double loop:
# a stand-alone program too
WN=$(mktemp -d)/wide_nn_host
g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
    -I rpg_monocular_pose_estimator_amd/csrc tests/host/wide_nn_host.cpp -o $WN && $WN || rc=1
rm -rf "$(dirname $WN)"
# the joint Gauss-Newton of a rig's cameras, k_rig_refine's logic (csrc/mpe_rig_gn.h) behind the tail helpers cut out of
# mpe_k3.hip: a stand-alone program too (one camera with the identity extrinsic against k3_gauss_newton bit for bit,
# rigs of up to 256 rows back to their true pose, the short problems)
RG=$(mktemp -d)
python -c "
import rpg_monocular_pose_estimator_amd as mpe
hip = mpe.device_source(); i = hip.index('struct T34 {')
open('$RG/k3_extract.inc', 'w').write(hip[i:hip.index('#define K3_GROUP', i)])" && \
g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
    -DRIG_GN_HOST_MAIN -I $RG -I tests/host/stub -I rpg_monocular_pose_estimator_amd/csrc tests/host/rig_gn_host.cpp \
    -o $RG/rig_gn_host && $RG/rig_gn_host || rc=1
rm -rf "$RG"
# the steps of the rig calibration, the k_rig_ba_* kernels' logic (csrc/mpe_rig_ba.h) behind mpe_rig_gn.h and the same cut
# of mpe_k3.hip, driven by the library's own row rules and iteration (csrc/mpe_rig_ba_plan.h): a stand-alone program too
# (exact-pixel rigs of 2 .. 16 cameras back to their extrinsics, again in chunks of one view bit for bit, the row rules)
RB=$(mktemp -d)
python -c "
import rpg_monocular_pose_estimator_amd as mpe
hip = mpe.device_source(); i = hip.index('struct T34 {')
open('$RB/k3_extract.inc', 'w').write(hip[i:hip.index('#define K3_GROUP', i)])" && \
g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
    -DRIG_BA_HOST_MAIN -I $RB -I tests/host/stub -I rpg_monocular_pose_estimator_amd/csrc tests/host/rig_ba_host.cpp \
    -o $RB/rig_ba_host && $RB/rig_ba_host || rc=1
rm -rf "$RB"
# the steps of the marker calibration, the k_body_ba_* kernels' logic (csrc/mpe_body_ba.h) behind mpe_rig_ba.h and the
# same cut of mpe_k3.hip, driven by the library's own row rules (csrc/mpe_body_ba_plan.h) and iteration: a stand-alone
# program too (exact-pixel bodies of 4 .. 16 markers back to their shape, again in chunks of one view bit for bit, the
# row rules)
BB=$(mktemp -d)
python -c "
import rpg_monocular_pose_estimator_amd as mpe
hip = mpe.device_source(); i = hip.index('struct T34 {')
open('$BB/k3_extract.inc', 'w').write(hip[i:hip.index('#define K3_GROUP', i)])" && \
g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
    -DBODY_BA_HOST_MAIN -I $BB -I tests/host/stub -I rpg_monocular_pose_estimator_amd/csrc tests/host/body_ba_host.cpp \
    -o $BB/body_ba_host && $BB/body_ba_host || rc=1
rm -rf "$BB"
exit $rc
