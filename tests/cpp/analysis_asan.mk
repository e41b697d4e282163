# analysis_asan: the plant analysis entry points that run on the host
# (csrc/abi_analysis.cpp, with csrc/abi_common.cpp for the error text) under
# ASan + UBSan (host code only), the rest from libcmpc.so; built and run by
# tests/test_analysis_asan.py:  make -C tests/cpp -f analysis_asan.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC = ../../compressor-mpc_amd/csrc
LIBDIR = ../../compressor-mpc_amd/cmpc

analysis_asan: analysis_asan.cpp $(CSRC)/abi_analysis.cpp $(CSRC)/abi_common.cpp $(CSRC)/abi_sim.h $(CSRC)/abi_common.h \
    $(CSRC)/eig_body.h $(CSRC)/gains_body.h $(CSRC)/target_body.h $(CSRC)/equilibrium_body.h $(CSRC)/plant_model.h \
    $(CSRC)/cmpc_internal.h $(LIBDIR)/libcmpc.so
	$(HIPCC) -O1 -g -std=c++17 -Wall -ffp-contract=off -fno-omit-frame-pointer -Xarch_host -fsanitize=address \
	  -Xarch_host -fsanitize=undefined -o $@ analysis_asan.cpp $(CSRC)/abi_analysis.cpp $(CSRC)/abi_common.cpp \
	  -L$(LIBDIR) -lcmpc -Wl,-rpath,'$$ORIGIN/../../compressor-mpc_amd/cmpc'

clean:
	rm -f analysis_asan
.PHONY: clean
