# The C++ test program of the files that share most of their bytes (tests/test_chunks_host.py).
# Run from this directory:
#   make -f chunks.mk            (__graft_entry__.build() does)
CXX ?= g++
ROOT := ../..
CXXFLAGS ?= -std=c++17 -O2 -g -Wall -Wextra -Wno-unused-parameter
LIBS := -L$(ROOT)/spacedrive_amd -lsdcore -lsdcas \
        -Wl,-rpath,'$$ORIGIN/../../../spacedrive_amd' -Wl,-rpath-link,/opt/rocm/lib

all: build/test_chunks

# without arguments: similarity_report_from on hand-made rows, no GPU;
# --gpu DIR: similarity_report over the files under DIR/loc on both libraries
build/test_chunks: test_chunks.cpp $(ROOT)/include/sdcore.hpp $(ROOT)/spacedrive_amd/libsdcore.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -I$(ROOT)/include -o $@ test_chunks.cpp $(LIBS)

.PHONY: all
