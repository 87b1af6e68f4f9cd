# The C++ test program of the chunk index (tests/test_chunk_index_host.py).
# Run from this directory:
#   make -f chunkindex.mk          (__graft_entry__.build() does)
CXX ?= g++
ROOT := ../..
CXXFLAGS ?= -std=c++17 -O2 -g -Wall -Wextra -Wno-unused-parameter
LIBS := -L$(ROOT)/spacedrive_amd -lsdcore -lsdcas -l:libsqlite3.so.0 \
        -Wl,-rpath,'$$ORIGIN/../../../spacedrive_amd' -Wl,-rpath-link,/opt/rocm/lib

all: build/test_chunk_index

# without arguments: SqliteLibrary's chunk tables, no GPU (it spoils a table through SQLite's own API);
# --gpu DIR: similarity_report_indexed step by step against similarity_report_streamed over everything
build/test_chunk_index: test_chunk_index.cpp $(ROOT)/include/sdcore.hpp $(ROOT)/spacedrive_amd/host/sqlite3_min.h \
                        $(ROOT)/spacedrive_amd/libsdcore.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -I$(ROOT)/include -I$(ROOT)/spacedrive_amd/host -o $@ test_chunk_index.cpp $(LIBS)

.PHONY: all
