#!/bin/bash
# Build the library of a git revision (default HEAD) as build/variants/lib_<name>.so
# for A/B runs against the working tree (scripts/ab_lib.sh <name>): that
# revision's sources, both translation units, through this tree's `variant` rule.
#   build_base.sh [REV] [NAME]
REV=${1:-HEAD}; NAME=${2:-base}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d /tmp/rhmc_base.XXXX)
git -C "$ROOT" archive "$REV" hmc-stellar-toy-model_amd/csrc include | tar -x -C "$T" || exit 1
make -s -C "$ROOT/hmc-stellar-toy-model_amd" variant NAME="$NAME" \
  SRCDIR="$T/hmc-stellar-toy-model_amd/csrc" INCDIR="$T/include" &&
echo "built lib_$NAME.so from $REV"
rm -rf "$T"
