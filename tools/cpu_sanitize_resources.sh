#!/bin/bash
# AddressSanitizer + UndefinedBehaviourSanitizer run of the owning resource types (csrc/r3d_resources.h), the arena, the staging
# helpers and the shared refusals and read-back of the entry points (csrc/r3d_internal.h), and the mesh entry points' size limits
# and array staging (csrc/r3d_mesh.h) on the CPU.
# On a machine without a GPU every HIP create call fails cleanly, so the stand-alone program tests/host/resources_main.hip walks
# exactly the failure paths that cannot be provoked on a shared card; with a GPU present the program skips.  Only the host half is
# instrumented, and the program is run directly (nothing is preloaded).  Usage: tools/cpu_sanitize_resources.sh
set -euo pipefail
root="$(cd "$(dirname "$0")/.." && pwd)"
tmp="$(mktemp -d /tmp/r3d_res.XXXXXX)"
trap 'rm -rf "$tmp"' EXIT
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
"$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Wall -Wno-unused-function -Xarch_host -fsanitize=address,undefined \
    -Xarch_host -fno-omit-frame-pointer "$root/tests/host/resources_main.hip" -o "$tmp/resources_main"
"$tmp/resources_main"
