# The C++ test program of the duplicate directories (tests/test_dirtree_host.py).
# Run from this directory:
#   make -f dirtree.mk            (__graft_entry__.build() does)
CXX ?= g++
ROOT := ../..
CXXFLAGS ?= -std=c++17 -O2 -g -Wall -Wextra -Wno-unused-parameter
LIBS := -L$(ROOT)/spacedrive_amd -lsdcore -lsdcas \
        -Wl,-rpath,'$$ORIGIN/../../../spacedrive_amd' -Wl,-rpath-link,/opt/rocm/lib

all: build/test_dirtree

# without arguments: tree_shape_from / tree_report_from on hand-made rows, no GPU;
# --gpu DIR: the identifier job with checksums over DIR/loc, then tree_report
build/test_dirtree: test_dirtree.cpp $(ROOT)/include/sdcore.hpp $(ROOT)/spacedrive_amd/libsdcore.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -I$(ROOT)/include -o $@ test_dirtree.cpp $(LIBS)

.PHONY: all
