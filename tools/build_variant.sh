#!/usr/bin/env bash
# A/B build of libsbr with extra -D flags (every source of the Makefile's SRCS):
#   tools/build_variant.sh NAME "-DFOO -DBAR=2"  ->  replication-social-bank-runs_amd/lib_var/NAME/libsbr.so
# (run bench.py / tests against it with SBR_LIB=<that path>)
set -eu
cd "$(dirname "$0")/../replication-social-bank-runs_amd"
name=$1; defs=${2:-}
make -s -j"${MAX_JOBS:-8}" BUILD="build_var/$name" LIB="lib_var/$name" EXTRA="$defs"
echo "lib_var/$name/libsbr.so"
