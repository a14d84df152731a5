#!/bin/bash
# The C++ host layer's CPU tests under AddressSanitizer + UndefinedBehaviorSanitizer (CPU build only: GPU sanitizers are not available
# on the test pool).  usage: bash tools/asan_host_tests.sh [test program, default host_tests; e.g. points_tests]
#   -> "... N checks, 0 failures" and no sanitizer report.  The program is stand-alone: the host sources and the test's main in one binary.
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
H=$ROOT/nextsimdg_amd/host
TEST=${1:-host_tests}
OUT=${TMPDIR:-/tmp}/nsdg_asan
mkdir -p $OUT
SRCS=$(ls $H/src/*.cpp | grep -v -e '/main\.cpp$' -e '/make_forcing\.cpp$')
g++ -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -std=c++17 -D__HIP_PLATFORM_AMD__ -I$H/include -I/opt/rocm/include \
    $SRCS $H/test/$TEST.cpp -o $OUT/${TEST}_asan \
    -L$ROOT/nextsimdg_amd/lib -lnsdg -L/opt/rocm/lib -lamdhip64 -lpthread -Wl,-rpath,$ROOT/nextsimdg_amd/lib -Wl,-rpath,/opt/rocm/lib
NSDG_GOLDEN_DIR=$ROOT/tests/golden ASAN_OPTIONS=detect_leaks=0:protect_shadow_gap=0 $OUT/${TEST}_asan
