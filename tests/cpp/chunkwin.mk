# The C++ test program of the chunk windows (tests/test_chunk_windows_host.py).
# Run from this directory:
#   make -f chunkwin.mk            (__graft_entry__.build() does)
CXX ?= g++
ROOT := ../..
CXXFLAGS ?= -std=c++17 -O2 -g -Wall -Wextra -Wno-unused-parameter
LIBS := -L$(ROOT)/spacedrive_amd -lsdcore -lsdcas \
        -Wl,-rpath,'$$ORIGIN/../../../spacedrive_amd' -Wl,-rpath-link,/opt/rocm/lib

all: build/test_chunk_windows

# without arguments: plan_chunk_windows and merge_chunk_windows on hand-made input, no GPU;
# --gpu DIR W: similarity_report_streamed against similarity_report over the files under DIR/loc
build/test_chunk_windows: test_chunk_windows.cpp $(ROOT)/include/sdcore.hpp $(ROOT)/spacedrive_amd/libsdcore.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -I$(ROOT)/include -o $@ test_chunk_windows.cpp $(LIBS)

.PHONY: all
