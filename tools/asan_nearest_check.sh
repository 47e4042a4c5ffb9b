#!/bin/bash
# The PLY point reader and the host statement of K18 (host/ply_read.cpp, host/nearest.cpp over csrc/eg3d_nearest_core.h)
# under AddressSanitizer + UBSan, as a stand-alone program: tools/nearest_asan_main.cpp with its own main, the two host
# sources compiled into it (without OpenMP: the statement runs sequentially). No GPU, nothing loaded into Python, nothing
# preloaded. The reader parses files from outside the project: the program feeds it malformed files and every prefix of a
# well-formed ASCII and binary file.
set -e
cd "$(dirname "$0")/.."
tmp=$(mktemp -d)
trap 'rm -rf $tmp' EXIT
g++ -O1 -g -std=c++17 -ffp-contract=off -fno-fast-math -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -fno-omit-frame-pointer -Wall -Wno-unknown-pragmas -I include -I edgegraph3d_amd/csrc -o $tmp/nearest_asan tools/nearest_asan_main.cpp \
    edgegraph3d_amd/host/ply_read.cpp edgegraph3d_amd/host/nearest.cpp
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 $tmp/nearest_asan $tmp
