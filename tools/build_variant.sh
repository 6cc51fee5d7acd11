#!/bin/bash
# one A/B build of the product library with extra compile flags for ONE translation unit:
#   [SRC=other/bloom.hip] bash tools/build_variant.sh <tag> <shade|bloom|ibl|...> [-DPBR_EXP_...]
# -> tools/ab/libpbr_<tag>.so (git-ignored; travels to the GPU box), used through PBR_HIP_LIB / tools/ab_libs.sh / tools/ab_shade_ms.sh
# The unit's compile flags and the library's object list are the Makefile's own (make -n), so the variant differs from the product
# library in that unit alone.  SRC: another source for the unit (a parent commit's copy, say); it includes the headers of csrc.
tag=$1; tu=$2; shift 2
[ -n "$SRC" ] && SRC=$(realpath "$SRC")
cd "$(dirname "$0")/../direct12pbrrenderer_amd/csrc" && mkdir -p ../../tools/ab && make -s ../libpbr_hip.so || exit 1
compile=$(make -n -B $tu.o | grep -- " -c $tu.hip -o $tu.o") || { echo "no rule for $tu.o"; exit 1; }
objs=""; for o in $(sed -n 's/^OBJS *:= *//p' Makefile); do [ $o = $tu.o ] && objs="$objs ../../tools/ab/${tu}_$tag.o" || objs="$objs $o"; done
${compile% -c $tu.hip -o $tu.o} -I. "$@" -c ${SRC:-$tu.hip} -o ../../tools/ab/${tu}_$tag.o &&
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o ../../tools/ab/libpbr_$tag.so $objs -ldl && echo built $tag
