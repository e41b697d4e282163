# freq_asan: the frequency responses' host arithmetic (csrc/freq_body.h) under
# ASan + UBSan, stand-alone (no library, no device); built and run by
# tests/test_freq.py:  make -C tests/cpp -f freq_asan.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC = ../../compressor-mpc_amd/csrc

freq_asan: freq_asan.cpp $(CSRC)/freq_body.h $(CSRC)/gains_body.h $(CSRC)/target_body.h $(CSRC)/equilibrium_body.h $(CSRC)/plant_model.h
	$(HIPCC) --cuda-host-only -O1 -g -std=c++17 -Wall -ffp-contract=off -fno-omit-frame-pointer -Xarch_host -fsanitize=address \
	  -Xarch_host -fsanitize=undefined -o $@ freq_asan.cpp

clean:
	rm -f freq_asan
.PHONY: clean
