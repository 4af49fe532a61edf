#!/bin/sh
# Re-record tests/golden/reference_vectors.npz: what the reference's own code (the oracle/_ref builds that oracle/Makefile makes from the
# reference's sources: libtce_ref*.so, glue_harness) returns on the inputs tests/test_oracle.py, tests/test_oracle_glue.py and
# tests/test_w8a8_adversarial_host.py build.
# Run after build(), where the reference tree is present; elsewhere those tests read the recorded results.
cd "$(dirname "$0")/../.." || exit 1
for f in libtce_ref.so libtce_ref_avx.so libtce_ref_x86naive.so libtce_ref_armnaive.so libtce_ref_metalnaive.so glue_harness; do
  [ -e "oracle/_ref/$f" ] || { echo "oracle/_ref/$f is not built: nothing to record from" >&2; exit 1; }
done
rm -f tests/golden/reference_vectors.npz
TCE_RECORD_REFERENCE_VECTORS=1 python -m pytest -q -p no:cacheprovider tests/test_oracle.py tests/test_oracle_glue.py tests/test_w8a8_adversarial_host.py
