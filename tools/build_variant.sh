#!/bin/bash
# build_variant.sh NAME "EXTRA HIPCC FLAGS" -> tools/ab/NAME.so
# A library variant for A/B runs and probes: the project's Makefile, so the
# same units and per-unit flags as librtmi.so, into a build directory of its
# own (nim-raytracer_amd/build/var/NAME), every unit compiled with -DRTMI_DIAG
# (the RTMI_* diagnostic environment knobs are read only by such builds,
# rt_common.h diag_env) and the extra flags. F32_FLAGS in the environment
# replaces the float32 kernels' flags, as for the Makefile itself.
set -e
cd "$(dirname "$0")/../nim-raytracer_amd"
mkdir -p ../tools/ab
make -s -j8 BUILD="build/var/$1" OUT="../tools/ab/$1.so" \
  CXXFLAGS="-O3 -std=c++17 -fPIC -Wall -Wno-unused-result -DRTMI_DIAG $2"
