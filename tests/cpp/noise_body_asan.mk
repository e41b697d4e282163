# noise_body_asan: the seeded noise's host arithmetic (csrc/noise_body.h) under
# ASan + UBSan, stand-alone (no library, no device); built and run by
# tests/test_noise.py:  make -C tests/cpp -f noise_body_asan.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC = ../../compressor-mpc_amd/csrc

noise_body_asan: noise_body_asan.cpp $(CSRC)/noise_body.h
	$(HIPCC) -O1 -g -std=c++17 -Wall -ffp-contract=off -fno-omit-frame-pointer -Xarch_host -fsanitize=address \
	  -Xarch_host -fsanitize=undefined -o $@ noise_body_asan.cpp

clean:
	rm -f noise_body_asan
.PHONY: clean
