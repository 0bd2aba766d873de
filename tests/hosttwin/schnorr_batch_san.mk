# The batch-verification twin (hosttwin_schnorr_batch.cpp) as a program of its own under AddressSanitizer and
# UndefinedBehaviorSanitizer:  make -C tests/hosttwin -f schnorr_batch_san.mk && tests/hosttwin/schnorr_batch_san
# (a sanitizer build is never loaded into Python; the shared library of the twins is the Makefile's)
CXX := /opt/rocm/lib/llvm/bin/clang++
CSRC := ../../rustcrypto-elliptic-curves_amd/csrc
schnorr_batch_san: hosttwin_schnorr_batch.cpp $(wildcard $(CSRC)/*.hpp) $(wildcard $(CSRC)/*.inc)
	$(CXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -DHOSTTWIN_SCHNORR_BATCH_MAIN -I$(CSRC) -Wall -Wno-unused-function $< -o $@
clean:
	rm -f schnorr_batch_san
