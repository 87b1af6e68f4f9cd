# The C++ test program of the duplicates confirmed by checksum
# (tests/test_confirm_host.py). Run from this directory:
#   make -f confirm.mk            (__graft_entry__.build() does)
CXX ?= g++
ROOT := ../..
CXXFLAGS ?= -std=c++17 -O2 -g -Wall -Wextra -Wno-unused-parameter
LIBS := -L$(ROOT)/spacedrive_amd -lsdcore -lsdcas \
        -Wl,-rpath,'$$ORIGIN/../../../spacedrive_amd' -Wl,-rpath-link,/opt/rocm/lib

all: build/test_confirm

# without arguments: duplicate_report_from and file_paths_with_checksum, no GPU;
# --gpu DIR: the identifier job with checksums, then confirm_duplicates
build/test_confirm: test_confirm.cpp $(ROOT)/include/sdcore.hpp $(ROOT)/spacedrive_amd/libsdcore.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -I$(ROOT)/include -o $@ test_confirm.cpp $(LIBS)

.PHONY: all
