#!/bin/sh
# VGPR / SGPR / scratch / LDS / occupancy of every kernel, from the compiler's
# -Rpass-analysis=kernel-resource-usage remarks (no GPU needed).
#   tools/kernel_resources.sh            main TU + resolve + variant 2 (8 waves)
#   tools/kernel_resources.sh 1 8        variant 1, 8 waves per workgroup
#   tools/kernel_resources.sh all        every object of the library that holds a probe or resolve kernel (the
#                                        Makefile's TU_OBJS), the two files of the row sorters (csr_rows.h) and the
#                                        four of the all-against-all calls (allpairs.h), one "== object ==" block each, JOBS (default 8) compilations side by side
cd "$(dirname "$0")/.." || exit 1
FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -c -Rpass-analysis=kernel-resource-usage -o /dev/null"
run() {
  /opt/rocm/bin/hipcc $FLAGS "$@" 2>&1 |
  awk '/Function Name:/ {name=$0; sub(/.*Function Name: /,"",name); sub(/ \[.*/,"",name)}
       /TotalSGPRs:/ {sg=$(NF-1)} / VGPRs:/ {vg=$(NF-1)} /ScratchSize/ {sc=$(NF-1)}
       /Occupancy/ {oc=$(NF-1)}
       /LDS Size/ {printf "%-70s vgpr=%s sgpr=%s scratch=%s occ=%s lds=%s\n", name, vg, sg, sc, oc, $(NF-1)}' |
  sed 's/_ZN4cmpr//; s/ENS_11ProbeParamsE//; s/EvNS_11ProbeParamsE//' | c++filt
}
if [ "$1" = all ]; then
  tmp=$(mktemp -d) || exit 1
  trap 'rm -rf "$tmp"' EXIT
  n=0
  one() {      # one <object name> <flags and file ...>
    name=$1; shift
    n=$((n + 1))
    { echo "== $name =="; run "$@"; } > "$tmp/$(printf %02d $n)" &
    [ $((n % ${JOBS:-8})) -eq 0 ] && wait
  }
  TU=compairr_amd/csrc/probe_tu.hip
  one probe_v0 -DTU_VARIANT=0 $TU
  one resolve -DTU_VARIANT=9 $TU
  one probe_pairs2 -DTU_VARIANT=3 $TU
  for nw in 4 8 16; do
    one probe_v1_nw$nw -DTU_VARIANT=1 -DTU_NW=$nw $TU
    one probe_v2_nw$nw -DTU_VARIANT=2 -DTU_NW=$nw -DTU_INLINE=0 $TU
    one probe_v2i_nw$nw -DTU_VARIANT=2 -DTU_NW=$nw -DTU_INLINE=1 $TU
    one probe_v2w_nw$nw -DTU_VARIANT=2 -DTU_NW=$nw -DTU_INLINE=0 -DTU_WIDE $TU
    one probe_v2wi_nw$nw -DTU_VARIANT=2 -DTU_NW=$nw -DTU_INLINE=1 -DTU_WIDE $TU
  done
  one neighbors compairr_amd/csrc/neighbors.hip
  one existence compairr_amd/csrc/existence.hip
  one allpairs compairr_amd/csrc/allpairs.hip
  one hamming compairr_amd/csrc/hamming.hip
  one edit compairr_amd/csrc/edit.hip
  one tcrdist compairr_amd/csrc/tcrdist.hip
  wait
  cat "$tmp"/* | grep -v 'rocprim::'          # (the library's own kernels: hipcub's instantiations are hundreds)
elif [ -n "$1" ]; then
  run -DTU_VARIANT="$1" -DTU_NW="${2:-8}" compairr_amd/csrc/probe_tu.hip
else
  run compairr_amd/csrc/compairr_hip.hip
  run -DTU_VARIANT=9 compairr_amd/csrc/probe_tu.hip
  run -DTU_VARIANT=2 -DTU_NW=8 compairr_amd/csrc/probe_tu.hip
fi
