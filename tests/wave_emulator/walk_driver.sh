#!/bin/sh
# tests/wave_emulator/walk_driver.sh [OUT [TREE]] -- TEST INFRASTRUCTURE: builds walk_driver.cpp together with the engine's device code
# for the wave emulator under AddressSanitizer (leak detection on) and UndefinedBehaviorSanitizer, and runs it: a stand-alone executable
# on the CPU (no Python, no preloaded runtime, never on a GPU).  Exit status 0 and a last line "walk driver: done" are the evidence of
# memory safety; the lines before it are the transcript of bo_perft, bo_mate, bo_anchor, bo_anchor_q and bo_anchor_eval.
# TREE: another checkout whose betaone_amd/csrc and include are compiled instead of this one's, with this driver and this emulator:
#   walk_driver.sh /tmp/a > a.txt && walk_driver.sh /tmp/b /path/to/other/checkout > b.txt && cmp a.txt b.txt
# shows that a change of the walk's host code left every output byte, error code and error text as it was.
# The emulator runs every lane as a fibre, and a fibre switch is dear under AddressSanitizer: expect minutes, not seconds (some three
# to compile the engine and five to seven to run, where the unsanitized emulator needs 15 s for the same calls).
# Where LeakSanitizer cannot run (it needs ptrace), WALK_DRIVER_LEAKS=0 keeps the rest.
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
OUT=${1:-/tmp/bo_walk_driver}
TREE=${2:-$ROOT}
g++ -std=c++17 -O1 -g -DBO_WAVE_EMU -Wall -Wno-unknown-pragmas -Wno-unused-function -ffp-contract=off -fno-fast-math \
    -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -I"$HERE" -I"$TREE/betaone_amd/csrc" -I"$TREE/include" \
    "$HERE/walk_driver.cpp" "$TREE/betaone_amd/csrc/bo_engine.cpp" -o "$OUT" -lm
ASAN_OPTIONS=detect_leaks=${WALK_DRIVER_LEAKS:-1}:detect_stack_use_after_return=0 UBSAN_OPTIONS=print_stacktrace=1 "$OUT"
