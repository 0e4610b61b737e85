#!/bin/sh
# tests/wave_emulator/poison_driver.sh -- TEST INFRASTRUCTURE: builds poison_driver.cpp together with the engine's device code for the
# wave emulator under AddressSanitizer and UndefinedBehaviorSanitizer, and runs it: a stand-alone executable on the CPU (no Python, no
# preloaded runtime, never on a GPU).  Exit status 0 and a last line "poison driver: clean" are the evidence.
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
OUT=${1:-/tmp/bo_poison_driver}
g++ -std=c++17 -O1 -g -DBO_WAVE_EMU -Wall -Wno-unknown-pragmas -Wno-unused-function -ffp-contract=off -fno-fast-math \
    -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -I"$HERE" -I"$ROOT/betaone_amd/csrc" -I"$ROOT/include" \
    "$HERE/poison_driver.cpp" "$ROOT/betaone_amd/csrc/bo_engine.cpp" -o "$OUT" -lm
ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0 UBSAN_OPTIONS=print_stacktrace=1 "$OUT"
