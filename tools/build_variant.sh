#!/bin/bash
# usage: build_variant.sh <name> <extra -D flags...>   -> gama_tts_amd/lib_variants/libgama_vtm_<name>.so
set -e
name=$1; shift
cd "$(dirname "$(readlink -f "$0")")/../gama_tts_amd/csrc"
mkdir -p _obj_$name ../lib_variants
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden "$@" -c vtm_kernels.hip -o _obj_$name/vtm_kernels.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden "$@" -c vtm_kernels_m5v.hip -o _obj_$name/vtm_kernels_m5v.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden "$@" -c vtm_kernels_targets.hip -o _obj_$name/vtm_kernels_targets.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden "$@" -c vtm_kernels_targets_voices.hip -o _obj_$name/vtm_kernels_targets_voices.o
# the float class of model 5 (its kernels use vtm_math.hpp too): no FMA contraction, as in the Makefile
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -ffp-contract=off "$@" -c vtm_kernels_m5f.hip -o _obj_$name/vtm_kernels_m5f.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -ffp-contract=off "$@" -c vtm_kernels_m5fv.hip -o _obj_$name/vtm_kernels_m5fv.o
# the host side of the C ABI (the extra flags reach vtm_capi_launch.cpp, which reads GVTM_NOISE_TABLE); the hooks as in the diagnostics library
for f in plan launch tracks host stream modification targets; do
	/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden $([ $f = targets ] && echo -ffp-contract=off) "$@" -x hip -c vtm_capi_$f.cpp -o _obj_$name/vtm_capi_$f.o
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden "$@" -DGVTM_DIAGNOSTICS -x hip -c vtm_capi_hooks.cpp -o _obj_$name/vtm_capi_hooks.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../lib_variants/libgama_vtm_$name.so _obj_$name/vtm_kernels.o _obj_$name/vtm_kernels_m5v.o _obj_$name/vtm_kernels_targets.o _obj_$name/vtm_kernels_targets_voices.o _obj_$name/vtm_capi_*.o _obj_$name/vtm_kernels_m5f.o _obj_$name/vtm_kernels_m5fv.o _obj/vtm_tracks.o _obj/vtm_pack.o _obj/vtm_intonation.o _obj/vtm_modification.o _obj/vtm_design.o _obj/vtm_diag_kernels.o
echo built $name
