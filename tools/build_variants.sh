#!/bin/bash
# Developer tool: builds libgarage_amd variants with different GEMM tile macros
# into garage_amd/_C/variants/ for A/B runs (tools/gemm_sweep.py --lib ...).
set -e
cd "$(dirname "$0")/.."
make -s
OUT=garage_amd/_C/variants
mkdir -p $OUT
build() {  # name, flags...
  name=$1; shift
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 "$@" -c garage_amd/csrc/gemm.hip -o $OUT/gemm_$name.o
  objs=$(ls garage_amd/_C/*.o | grep -v '/gemm.o' | grep -v fused_entries_shim)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs $OUT/gemm_$name.o -ldl -o $OUT/lib_$name.so
  echo built $name
}
build occ6 -DGA_GEMM_WAVES_PER_EU=6 &
# fused_train.hip with the Makefile's flags: the two items of fwd_dgrad_kernel's r06 work
# switched back to approximately the parent's code -- the staged loop's explicit unroll
# and the struct that holds its fragments are outside the macros, so measure the parent
# commit itself beside ft_none (GA_FT_NO_BUFFER_ADDR: vector addresses instead of
# scalar-offset buffer accesses; GA_FT_NO_EARLY_DZ: E6, then E5 with the dZ2 stores in
# front of the data gradient's first loads) for tools/bench_variant.py
build_ft() {  # name, flags...
  name=$1; shift
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -fno-slp-vectorize -fvisibility=hidden -fvisibility-inlines-hidden "$@" -c garage_amd/csrc/fused_train.hip -o $OUT/fused_train_$name.o
  objs=$(ls garage_amd/_C/*.o | grep -v '/fused_train.o' | grep -v fused_entries_shim)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs $OUT/fused_train_$name.o -ldl -o $OUT/lib_$name.so
  echo built $name
}
build_ft ft_none -DGA_FT_NO_BUFFER_ADDR -DGA_FT_NO_EARLY_DZ &
build_ft ft_addr -DGA_FT_NO_EARLY_DZ &
build_ft ft_early_dz -DGA_FT_NO_BUFFER_ADDR &
# gemm.hip with the Makefile's flags: the three items of gemm_rr_paired_kernel (the
# paired-column weight-gradient GEMM, r07) switched back one at a time and all together
# (GA_GEMM_NO_PAIRED_COLS: 64 x 32 wave tiles and ds_read_b32 fragments, which also puts
# the slab back through LDS; GA_GEMM_NO_DIRECT_STORE: the staged epilogue;
# GA_GEMM_NO_BUFFER_ADDR: 64-bit vector addresses).  The parent's kernel itself is
# GARAGE_AMD_WGRAD_PAIRED=0 with any of these libraries.
build_rr() {  # name, flags...
  name=$1; shift
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -fno-slp-vectorize -fvisibility=hidden -fvisibility-inlines-hidden "$@" -c garage_amd/csrc/gemm.hip -o $OUT/gemm_$name.o
  objs=$(ls garage_amd/_C/*.o | grep -v '/gemm.o' | grep -v fused_entries_shim)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs $OUT/gemm_$name.o -ldl -o $OUT/lib_$name.so
  echo built $name
}
build_rr rr_none -DGA_GEMM_NO_PAIRED_COLS -DGA_GEMM_NO_DIRECT_STORE -DGA_GEMM_NO_BUFFER_ADDR &
build_rr rr_no_paired -DGA_GEMM_NO_PAIRED_COLS &
build_rr rr_no_direct -DGA_GEMM_NO_DIRECT_STORE &
build_rr rr_no_buffer -DGA_GEMM_NO_BUFFER_ADDR &
build_rr rr_paired_only -DGA_GEMM_NO_DIRECT_STORE -DGA_GEMM_NO_BUFFER_ADDR &
build_rr rr_buffer_only -DGA_GEMM_NO_PAIRED_COLS -DGA_GEMM_NO_DIRECT_STORE &
wait
