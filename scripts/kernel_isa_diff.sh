#!/bin/bash
# Are the gfx950 kernels of two versions of the sources the same code?  Compiles every instance of lds_inst.hip, or the host sources
# named, from both csrc directories to assembly (the Makefile's flags + --cuda-device-only -S), normalises both sides and compares them:
# the check behind a device-side refactor that claims to change no instruction.
# usage: scripts/kernel_isa_diff.sh <csrc A> <csrc B> [item ...]
#   item = an LDS instance (F32_13, F64X_14, ...) or a source of the directory by name (transforms.hip, keyswitch.hip, ...), whose kernels
#   are the ones that source launches.  Default: the Makefile's LDS_INST.
#   The flags and the default instance list are read from the Makefile of <csrc B> ONLY and used for both sides: a change of CXXFLAGS
#   between A and B is not seen by this script (A is compiled under B's flags).
#   ISA_DIFF_DIR=dir  keep the assembly there; an item whose .s is newer than every file of its csrc directory is not compiled again
#                     (only files directly in that directory are looked at, not the flags and not a generator elsewhere: after a change
#                     of CXXFLAGS or of what writes wide_asm.inc, empty the directory)
#   JOBS=n            compiles at a time (default 16, at most 16)
# Normalisation: comment lines and .file / .ident / .loc / .section directives dropped, .L<...><digits> labels rewritten to one token,
# __hip_cuid_* lines ignored, and ntt_ct_a_kernel<F, LOGN, MINW, COMPACT_OUT, false> (the form with the EARLY parameter, removed since)
# renamed to ntt_ct_a_kernel<F, LOGN, MINW, COMPACT_OUT>.  Whole files are compared, so the kernels must also come out in the same ORDER
# (the order in which the host code first names them); where files differ, the kernels whose own text differs are listed with the
# number of differing lines, and none listed means a different order only.  Exit status 0: every item equal, with the same set of kernels.
# no pipefail / -e: a compile that fails leaves no .s file, and the comparison loop reports exactly that
set -u
[ $# -ge 2 ] || { sed -n '2,14p' "$0"; exit 2; }
A=$(cd "$1" && pwd) && B=$(cd "$2" && pwd) || exit 2
shift 2
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS=$(make -s -C "$B" print-CXXFLAGS) || exit 2
INST=${*:-$(make -s -C "$B" print-LDS_INST)}
JOBS=${JOBS:-16}; [ "$JOBS" -le 16 ] || JOBS=16
OUT=${ISA_DIFF_DIR:-$(mktemp -d)}
mkdir -p "$OUT/a" "$OUT/b"

compile() {   # <csrc> <out dir> <item>
    local s=$2/$3.s src=lds_inst.hip defs="-DFHE_FIELD=${3%_*} -DFHE_LOGN=${3#*_}"
    case $3 in *.hip) src=$3; defs=;; esac
    [ -s "$s" ] && [ -z "$(find "$1" -maxdepth 1 -type f -newer "$s" -print -quit)" ] && return 0
    (cd "$1" && $HIPCC $FLAGS --cuda-device-only -S $defs -o "$s.tmp" $src) > "$2/$3.log" 2>&1 && mv "$s.tmp" "$s"
}
for i in $INST; do
    for side in a b; do
        while [ "$(jobs -rp | wc -l)" -ge "$JOBS" ]; do wait -n; done
        if [ $side = a ]; then compile "$A" "$OUT/a" $i & else compile "$B" "$OUT/b" $i & fi
    done
done
wait

normalise() {
    grep -vE '^[[:space:]]*(;|//|\.file|\.ident|\.loc|\.section)|__hip_cuid_' "$1" |
        sed -E 's/[[:space:]]*(;|\/\/).*$//; s/\.L[A-Za-z_$.]*[0-9]+/.L#/g; s/(ntt_ct_a_kernelINS_[0-9A-Z]+ELi[0-9]+ELi[0-9]+ELb[01]E)Lb0E/\1/g'
}
kernels() { sed -nE 's/^[[:space:]]*\.amdhsa_kernel[[:space:]]+//p' "$1" | sort; }
body() { awk -v k="$2:" '$0 == k { on = 1 } on { print } on && /^[[:space:]]*\.end_amdhsa_kernel/ { exit }' "$1"; }   # a kernel's code and descriptor

bad=0
for i in $INST; do
    if [ ! -s "$OUT/a/$i.s" ] || [ ! -s "$OUT/b/$i.s" ]; then echo "$i: COMPILE FAILED (see $OUT/{a,b}/$i.log)"; bad=1; continue; fi
    normalise "$OUT/a/$i.s" > "$OUT/a/$i.norm"; normalise "$OUT/b/$i.s" > "$OUT/b/$i.norm"
    nk=$(kernels "$OUT/b/$i.norm" | wc -l); nl=$(wc -l < "$OUT/b/$i.norm")
    if ! diff <(kernels "$OUT/a/$i.norm") <(kernels "$OUT/b/$i.norm") > "$OUT/$i.kernels.diff"; then
        echo "$i: DIFFERENT SET OF KERNELS"; sed 's/^/    /' "$OUT/$i.kernels.diff" | head -20; bad=1
    elif ! cmp -s "$OUT/a/$i.norm" "$OUT/b/$i.norm"; then
        echo "$i: DIFFERENT  $nk kernels, $(diff "$OUT/a/$i.norm" "$OUT/b/$i.norm" | grep -c '^[<>]') of $nl lines differ (diff $OUT/a/$i.norm $OUT/b/$i.norm)"; bad=1
        for k in $(kernels "$OUT/b/$i.norm"); do
            d=$(diff <(body "$OUT/a/$i.norm" $k) <(body "$OUT/b/$i.norm" $k) | grep -c '^[<>]')
            [ "$d" = 0 ] || echo "    $k: $d of $(body "$OUT/b/$i.norm" $k | wc -l) lines differ"
        done
    else
        echo "$i: equal  $nk kernels, $nl lines"
    fi
done
[ $bad = 0 ] && echo "all $(echo $INST | wc -w) items equal" || echo "DIFFERENCES FOUND"
[ -n "${ISA_DIFF_DIR:-}" ] || [ $bad != 0 ] || rm -rf "$OUT"
exit $bad
