#!/bin/bash
# Register / scratch / LDS usage of every kernel of a .hip source, from the gfx950 code object's notes.
# (a kernel's note starts at its "- " list item, whichever key comes first: keys before .name belong to the kernel that follows)
# Usage: bash scripts/kernel_resources.sh neptune_amd/csrc/qp_kernels.hip [extra hipcc flags]
SRC=$1; shift
OUT=/tmp/$(basename "$SRC" .hip).gfx950.co
FP=""; case "$SRC" in *geom_kernels*|*tether_kernels*|*audit_kernels*|*audit_span_kernels*|*fleet_kernels*|*fleet_mission_kernels*|*fleet_moveback_kernels*|*fleet_effort_kernels*) FP="-ffp-contract=off";; esac
QF=""; case "$SRC" in *geom_kernels*) QF="-mllvm -disable-machine-licm";; *qp_reg_kernel*) QF="-mllvm -disable-machine-licm -mllvm -amdgpu-sched-strategy=max-ilp";; esac
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 $FP $QF "$@" --cuda-device-only --no-gpu-bundle-output -c "$SRC" -o "$OUT" || exit 1
/opt/rocm/lib/llvm/bin/llvm-readelf --notes "$OUT" | grep -E "\.name:|\.vgpr_count|\.agpr_count|\.sgpr_count|vgpr_spill|sgpr_spill|private_segment_fixed|group_segment_fixed" \
  | sed -e 's/^ *//' | awk '{new=sub(/^- /,"")} new{if(name)print name rest; name=""; rest=""} /^\.name:/{name=$2; next} {rest=rest"  "$1$2} END{print name rest}' | c++filt
