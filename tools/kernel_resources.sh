#!/bin/bash
# Registers, scratch and LDS of every kernel of the library, from the compiler's own resource remarks (device-only compile of
# each .hip file with the Makefile's flags).  Usage: tools/kernel_resources.sh [file.hip ...] > profiles/rNN_kernel_resources.txt
cd "$(dirname "$0")/../mcmc-date_amd/csrc" || exit 1
files=("$@"); [ ${#files[@]} -eq 0 ] && files=(k_*.hip)
for f in "${files[@]}"; do
  { read -r extra; mapfile -t defs; } < <(make -s flags SRC="$f")   # the Makefile's flags of this source, and the defines of each object it makes
  for def in "${defs[@]}"; do
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-fast-math -ffp-contract=off --cuda-device-only $def $extra -c "$f" -o /dev/null \
      -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs:|AGPRs:|VGPRs Spill|ScratchSize|LDS Size|Occupancy" \
      | sed 's/.*remark: *//; s/ *\[-Rpass.*//' | paste - - - - - - - | while IFS=$'\t' read -r name v a sc oc sp lds; do
        printf "%-14s %s | %s | %s | %s | %s | %s | %s\n" "$f" "$(echo "${name#Function Name: }" | c++filt | sed 's/(.*//' | cut -c1-70)" "$v" "$a" "$sp" "$sc" "$lds" "$oc"
      done
  done
done
