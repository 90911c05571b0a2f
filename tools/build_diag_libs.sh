#!/bin/bash
# Diagnostic builds of libs2sr.so for the split-operand tail convs (conv3x3.hip), made next to the shipped library
# (csrc/diag/*.so, git-ignored):
#   libs2sr_f8diag{1,2,4,8}.so  -DS2SR_DIAG_F8=n   1 no LDS-DMA, 2 no MFMA, 4 no epilogue, 8 epilogue without stores (tools/tail_anatomy.sh)
#   libs2sr_f8diag16.so         no diagnostic bit that changes a kernel: the shipped conv3x3 under another name (fewer workgroups: the
#                               shipped library's S2SR_GRID_CAP=<workgroups>, which took over from this build's S2SR_DIAG_GRID)
# Each links every object of the shipped build (csrc/Makefile's OBJS) except conv3x3.o, which it recompiles.
# Usage: tools/build_diag_libs.sh [names...]   (default: all);  rm -rf csrc/diag afterwards.
set -e
C=sentinel2-super-resolution-poc_amd/csrc
make -C $C > /dev/null
mkdir -p $C/diag
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -Wno-unused-result -Wno-unused-value -ffp-contract=off"
OBJS=$(make -C $C -s --no-print-directory -f Makefile -f - objs <<< 'objs: ; @echo $(filter-out conv3x3.o,$(OBJS))')
build() {  # name, define
  /opt/rocm/bin/hipcc $FLAGS $2 -c $C/conv3x3.hip -o $C/diag/conv3x3_$1.o
  (cd $C && /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o diag/libs2sr_$1.so $OBJS diag/conv3x3_$1.o)
  rm -f $C/diag/conv3x3_$1.o
  echo built $C/diag/libs2sr_$1.so
}
want=${@:-f8diag1 f8diag2 f8diag4 f8diag8 f8diag16}
for n in $want; do
  case $n in
    f8diag*) build $n "-DS2SR_DIAG_F8=${n#f8diag}" & ;;
    *) echo "unknown $n"; exit 1 ;;
  esac
done
wait
