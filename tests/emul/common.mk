# What every model library under tests/emul*/ is built with and depends on (test infrastructure; included by the
# Makefile beside each model, which is run from its own directory).
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++20 -fPIC -pthread -ffp-contract=off -fno-fast-math -mfma -Wall -Wno-unused-function -Wno-unknown-pragmas
CSRC := ../../gr-ais_amd/csrc
HDR := $(wildcard $(CSRC)/*.h) ../../include/aisx.h ../emul/emul.cpp ../emul/emul_plan.h ../emul/common.mk
SANFLAGS := -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all
