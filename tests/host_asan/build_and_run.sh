#!/bin/bash
# Builds the HOST half of libmod16hip with AddressSanitizer + UndefinedBehaviorSanitizer against the
# HIP runtime stand-in of this directory, links one driver of this directory against it and runs it:
#   bash tests/host_asan/build_and_run.sh NAME [OUTDIR]      NAME: driver, or a family (trend, zonal, ...)
# (hipcc --cuda-host-only: the library's own source, its host side exactly as shipped; no GPU needed)
# The library's and the stand-in's objects are the same for every driver: they are compiled once per
# content of their sources into ${MOD16_HOST_ASAN_CACHE:-${TMPDIR:-/tmp}/mod16_host_asan}/<digest>/.
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
NAME=$1
[ -n "$NAME" ] && [ -f "$HERE/$NAME.cpp" ] || { echo "usage: $0 NAME [OUTDIR], NAME.cpp being a driver of $HERE" >&2; exit 2; }
PROG=host_asan_$NAME
[ "$NAME" = driver ] && PROG=host_asan
OUT=${2:-$(mktemp -d)}
mkdir -p "$OUT"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1"
# every file the two objects are made of, the compiler and its flags: an edit to any gives another directory
CSRC="$ROOT/mod16_amd/csrc"
DIGEST=$(set -o pipefail; export LC_ALL=C
         { echo "$SAN"; $HIPCC --version
           cat "$CSRC"/*.hip "$CSRC"/*.hpp "$CSRC"/capi/* "$ROOT/include/mod16_hip.h" "$HERE/hip_stub.hip"; } | sha256sum | cut -d' ' -f1)
CACHE=${MOD16_HOST_ASAN_CACHE:-${TMPDIR:-/tmp}/mod16_host_asan}
LIB="$CACHE/$DIGEST"
NEW=
if [ ! -r "$LIB/capi.o" ] || [ ! -r "$LIB/stub.o" ]; then
  # no locks: compiled into a directory of its own and published with one mv; whoever comes second drops its copy
  # (a cache this user cannot write or read, another user's in a shared /tmp: both objects go to OUTDIR)
  if mkdir -p "$CACHE" 2>/dev/null && NEW=$(mktemp -d "$LIB.XXXXXX" 2>/dev/null); then
    chmod a+rx "$NEW"
    trap 'rm -rf "$NEW"' EXIT
  else
    NEW=$OUT LIB=$OUT
  fi
  # the driver and the stub are small: compile them while the library compiles
  $HIPCC --cuda-host-only $SAN -std=c++17 -w -c "$CSRC/mod16_capi.hip" -o "$NEW/capi.o" &
  $HIPCC --cuda-host-only $SAN -std=c++17 -w -c "$HERE/hip_stub.hip" -o "$NEW/stub.o"
fi
$HIPCC --cuda-host-only $SAN -std=c++17 -w -x hip -c "$HERE/$NAME.cpp" -o "$OUT/driver.o"
if [ -n "$NEW" ]; then
  wait $!
  [ "$NEW" = "$LIB" ] || mv -T "$NEW" "$LIB" 2>/dev/null || rm -rf "$NEW"
fi
# host-only objects refer to the device code object of their translation unit by a hashed symbol: define them
: > "$OUT/fatbin.c"
for o in "$LIB/capi.o" "$LIB/stub.o" "$OUT/driver.o"; do
  for s in $(nm "$o" | awk '$1 == "U" && $2 ~ /^__hip_fatbin/ {print $2}'); do echo "const char $s[8] = {0};" >> "$OUT/fatbin.c"; done
done
/opt/rocm/lib/llvm/bin/clang $SAN -c "$OUT/fatbin.c" -o "$OUT/fatbin.o"
/opt/rocm/lib/llvm/bin/clang++ $SAN "$OUT/driver.o" "$LIB/capi.o" "$LIB/stub.o" "$OUT/fatbin.o" -lpthread -o "$OUT/$PROG"
if [ "$NAME" != driver ]; then
  ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/$PROG"
  exit 0
fi
ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 UBSAN_OPTIONS=print_stacktrace=1 MOD16_HOST_THREADS=3 "$OUT/host_asan"
# ... and the harness sees a fault when there is one (exit code != 0 expected)
if "$OUT/host_asan" --fault > "$OUT/fault.log" 2>&1; then echo "host_asan: the planted fault was NOT detected"; cat "$OUT/fault.log"; exit 1; fi
grep -q "lies outside every live device allocation" "$OUT/fault.log" && echo "host_asan: planted fault detected: $(grep 'hip_stub:' "$OUT/fault.log" | head -1 | cut -c1-160)"
