#!/bin/bash
# Developer builds of libseirhip into tools/dev/variants/libseirhip_<tag>.so
#   bash tools/dev/build_variant.sh <tag> [-DNAME=VALUE ...]   a stamped build (the tags below) with its flags, plus any given;
#                                                              any other tag: an experiment with just the flags given
#   bash tools/dev/build_variant.sh --all                      every stamped build
#   bash tools/dev/build_variant.sh --list                     the table below
set -e
# The stamped builds: tag | flags.  One line per entry of VARIANTS in covid19uk_amd/csrc/stamps.h (the families, their words
# and the tools that read them are stated there; tests/test_stamps_table.py holds the two lists together)
variants() { cat <<'EOF'
seirst|-DSEIR_STAMPS -DSEIR_STAMP_SLOT=1
propst|-DSEIR_STAMPS -DSEIR_STAMP_PROPOSE -DSEIR_STAMP_SLOT=1 -DSEIR_STAMP_ROLE=1
pairst|-DPAIR_STAMPS=1 -mllvm -disable-machine-licm
leapst|-DLEAP_STAMPS=1 -mllvm -disable-machine-licm
leapst2|-DLEAP_STAMPS=2 -DLEAP_CPROBE -mllvm -disable-machine-licm
tailst|-DTAIL_STAMPS -mllvm -disable-machine-licm
sest|-DSE_STAMPS
evst|-DEVAL_STAMPS=1 -mllvm -disable-machine-licm
EOF
}
root=$(cd "$(dirname "$0")/../.." && pwd)
build() {
    local tag=$1; shift
    mkdir -p "$root/tools/dev/variants"
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wno-pass-failed "$@" \
        -o "$root/tools/dev/variants/libseirhip_${tag}.so" "$root/covid19uk_amd/csrc/seir_hip.hip"
    echo "built variant $tag: $*"
}
case "$1" in
--list) variants ;;
--all) variants | while IFS='|' read -r tag flags; do build "$tag" $flags; done ;;
*)  tag=$1; shift
    flags=$(variants | awk -F'|' -v t="$tag" '$1 == t { print $2 }')
    build "$tag" $flags "$@" ;;
esac
