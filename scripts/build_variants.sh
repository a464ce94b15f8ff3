#!/bin/bash
# Build librhmc.so variants with extra -D flags for A/B runs on the GPU box:
#   build_variants.sh name1="-DFOO=1" name2="-DBAR=2" ...
# -> build/variants/lib_<name>.so (select at run time with RHMC_LIB=...)
# Both translation units, through the Makefile's `variant` rule.
cd "$(dirname "$0")/../hmc-stellar-toy-model_amd" || exit 1
for spec in "$@"; do
  name=${spec%%=*}; flags=${spec#*=}
  ( make -s variant NAME="$name" FLAGS="$flags" && echo "built $name" ) &
done
wait
