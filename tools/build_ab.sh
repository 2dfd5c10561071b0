#!/bin/bash
# Build A/B copies of libvoidin_hip.so with extra -D flags: tools/build_ab.sh NAME "-DFOO=1" -> build/ab/NAME/libvoidin_hip.so
# AB_SRC=DIR: compile every file from DIR (the csrc directory of another checkout, e.g. `git worktree add` of the parent commit)
# instead of this tree's: the other leg of an A/B against an earlier commit (tools/ab_tlas_lbvh.py).
set -e
cd "$(dirname "$0")/.."
name=$1; shift
d=build/ab/$name; mkdir -p $d
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -Wno-unused-function"
src=${AB_SRC:-voidin_amd/csrc}
for f in $(cd $src && ls *.hip | sed 's/\.hip$//'); do
  X=""; if [ "$f" = blas ]; then X="-mllvm -amdgpu-kernarg-preload-count=16"; fi   # the Makefile's per-file flag: both legs of an A/B get it
  if [ -n "$AB_SRC" ] || [ "$f" = "${AB_FILE:-cull}" ] || [ ! -f voidin_amd/csrc/$f.o ]; then /opt/rocm/bin/hipcc $F $X "$@" -c $src/$f.hip -o $d/$f.o; else cp voidin_amd/csrc/$f.o $d/$f.o; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $d/libvoidin_hip.so $d/*.o
rm -f $d/*.o
echo built $d
