#!/bin/bash
# Per-kernel register/scratch/occupancy table from the compiler's
# resource remarks (plain kernels-only compile, no torch headers):
#   bash csrc/tools/check_resources.sh                # all kernel TUs
#   bash csrc/tools/check_resources.sh csrc/fmha.hip  # one file
# Compare against profiles/raw/kernel_resources.txt before merging a
# change to these kernels: they sit on occupancy steps.
set -e -o pipefail
cd "$(dirname "$0")/../.."
if [ $# -gt 0 ]; then SRCS=("$@"); else
  SRCS=(csrc/fmha.hip csrc/wgemm.hip csrc/fgemm.hip csrc/probes.hip
        csrc/layernorm.hip csrc/gelu.hip csrc/dropout.hip
        csrc/drop_path.hip csrc/transpose.hip)
fi
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
printf '%-58s %5s %5s %8s %4s %7s\n' kernel VGPR AGPR scratchB occ vspills
for SRC in "${SRCS[@]}"; do
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -DVITFSDP_KERNELS_ONLY \
    -Rpass-analysis=kernel-resource-usage -c "$SRC" -o "$OUT/ra.o" \
    2> "$OUT/remarks.txt" || { cat "$OUT/remarks.txt" >&2; exit 1; }
  sed -n 's/.*remark: *\(.*\) \[-Rpass-analysis.*/\1/p' "$OUT/remarks.txt" |
    awk -F': ' '
      $1 == "Function Name" { name = $2 }
      $1 == "VGPRs" { v = $2 }
      $1 == "AGPRs" { a = $2 }
      $1 ~ /^ScratchSize/ { s = $2 }
      $1 ~ /^Occupancy/ { o = $2 }
      $1 == "VGPRs Spill" { print name, v, a, s, o, $2 }' |
    while read -r name v a s o sp; do
      short=$(c++filt "$name")
      short=${short#void }
      short=${short#(anonymous namespace)::}
      printf '%-58s %5s %5s %8s %4s %7s\n' "${short%%(*}" "$v" "$a" "$s" "$o" "$sp"
    done
done
