# build an experimental variant of the library: tools/build_variant.sh NAME [-DFLAG ...]
# (the kernels compiled anew with the flags, linked with the objects `make` has left in freesasa_amd/lib;
#  CSRC=dir compiles another copy of freesasa_amd/csrc, e.g. one with a kernel header changed on purpose)
NAME=$1; shift
CSRC=${CSRC:-freesasa_amd/csrc}
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off "$@" -c $CSRC/gpu_kernels.hip -o /tmp/ge_$NAME.o && \
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -Wl,--version-script=freesasa_amd/csrc/exports.map -o freesasa_amd/lib/libvar_$NAME.so /tmp/ge_$NAME.o $(ls freesasa_amd/lib/*.o | grep -v '/gpu_kernels\.o$') && echo built libvar_$NAME.so
