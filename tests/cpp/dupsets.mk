# The C++ test program of the duplicate sets (tests/test_dupsets_host.py).
# Run from this directory:
#   make -f dupsets.mk            (__graft_entry__.build() does)
CXX ?= g++
ROOT := ../..
CXXFLAGS ?= -std=c++17 -O2 -g -Wall -Wextra -Wno-unused-parameter
LIBS := -L$(ROOT)/spacedrive_amd -lsdcore -lsdcas \
        -Wl,-rpath,'$$ORIGIN/../../../spacedrive_amd' -Wl,-rpath-link,/opt/rocm/lib

all: build/test_dupsets

# without arguments: reclaim_report_from on hand-made arrays, no GPU;
# --gpu DIR: the identifier job with checksums, then reclaim_report
build/test_dupsets: test_dupsets.cpp $(ROOT)/include/sdcore.hpp $(ROOT)/spacedrive_amd/libsdcore.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -I$(ROOT)/include -o $@ test_dupsets.cpp $(LIBS)

.PHONY: all
