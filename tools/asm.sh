#!/bin/bash
# tools/asm.sh <file-stem> [extra flags]: device ISA of one csrc/*.hip into /tmp/<stem>.s, with per-kernel register / scratch use.
# Built with the Makefile's flags for that file (HIPFLAGS and FLAGS_<stem>): what it shows is what ships.
stem=$1; shift
cd "$(dirname "$0")/../wgpu-path-tracing_amd"
mk() { make -s --no-print-directory --eval='print-%: ; @echo $($*)' print-$1; }
/opt/rocm/bin/hipcc $(mk HIPFLAGS) $(mk FLAGS_$stem) "$@" -S --cuda-device-only -o /tmp/$stem.s csrc/$stem.hip 2>&1 | grep -v "warning\|^$" | tail -3
grep "\.name:\|\.vgpr_count\|private_segment_fixed\|\.sgpr_count" /tmp/$stem.s | paste - - - - | awk '{print $2, "scratch", $4, "sgpr", $6, "vgpr", $8}' | sed 's/_ZN12_GLOBAL__N_1//'
