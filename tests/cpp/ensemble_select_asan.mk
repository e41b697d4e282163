# ensemble_select_asan: the quantile selection's host arithmetic
# (csrc/ensemble_select.h) under ASan + UBSan, stand-alone (no library, no
# device); built and run by tests/test_quantiles.py:
#   make -C tests/cpp -f ensemble_select_asan.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC = ../../compressor-mpc_amd/csrc

ensemble_select_asan: ensemble_select_asan.cpp $(CSRC)/ensemble_select.h
	$(HIPCC) -O1 -g -std=c++17 -Wall -ffp-contract=off -fno-omit-frame-pointer -Xarch_host -fsanitize=address \
	  -Xarch_host -fsanitize=undefined -o $@ ensemble_select_asan.cpp

clean:
	rm -f ensemble_select_asan
.PHONY: clean
