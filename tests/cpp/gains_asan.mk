# gains_asan: the steady-state gains' host arithmetic (csrc/gains_body.h) under
# ASan + UBSan, stand-alone (no library, no device); built and run by
# tests/test_gains.py:  make -C tests/cpp -f gains_asan.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC = ../../compressor-mpc_amd/csrc

gains_asan: gains_asan.cpp $(CSRC)/gains_body.h $(CSRC)/target_body.h $(CSRC)/equilibrium_body.h $(CSRC)/plant_model.h
	$(HIPCC) --cuda-host-only -O1 -g -std=c++17 -Wall -ffp-contract=off -fno-omit-frame-pointer -Xarch_host -fsanitize=address \
	  -Xarch_host -fsanitize=undefined -o $@ gains_asan.cpp

clean:
	rm -f gains_asan
.PHONY: clean
