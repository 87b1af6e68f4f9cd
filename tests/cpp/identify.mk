# The C++ test programs of the one-pass cas_id + checksum (TEST INFRASTRUCTURE:
# test_identify_job links the oracle as checker). Run from this directory:
#   make -f identify.mk            both programs (__graft_entry__.build() does)
#   make -f identify.mk sanitize   test_identify_io under ASan + UBSan
CXX ?= g++
ROOT := ../..
CXXFLAGS ?= -std=c++17 -O2 -g -Wall -Wextra -Wno-unused-parameter
LIBS := -L$(ROOT)/spacedrive_amd -lsdcore -lsdcas -L$(ROOT)/oracle/build -loracle \
        -Wl,-rpath,'$$ORIGIN/../../../spacedrive_amd' -Wl,-rpath,'$$ORIGIN/../../../oracle/build' \
        -Wl,-rpath-link,/opt/rocm/lib
CAS_IO := $(ROOT)/spacedrive_amd/host/cas_io.cpp $(ROOT)/spacedrive_amd/host/cas_io.hpp
ASAN := -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer

all: build/test_identify_job build/test_identify_io

# the identifier job that also fills integrity_checksum: its flag without a GPU,
# and (--gpu) against job + validator
build/test_identify_job: test_identify_job.cpp $(ROOT)/include/sdcore.hpp $(ROOT)/spacedrive_amd/libsdcore.so $(ROOT)/oracle/build/liboracle.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -I$(ROOT)/include -o $@ test_identify_job.cpp $(LIBS)

# sdcas_identify_checksums' GPU-free open helper (a FIFO is never opened)
build/test_identify_io: test_identify_io.cpp $(CAS_IO)
	@mkdir -p build
	$(CXX) -std=c++17 -O1 -g -Wall -o $@ test_identify_io.cpp $(ROOT)/spacedrive_amd/host/cas_io.cpp -lpthread

build/test_identify_io_asan: test_identify_io.cpp $(CAS_IO)
	@mkdir -p build
	$(CXX) -std=c++17 -O1 -g $(ASAN) -o $@ test_identify_io.cpp $(ROOT)/spacedrive_amd/host/cas_io.cpp -lpthread

sanitize: build/test_identify_io_asan

.PHONY: all sanitize
