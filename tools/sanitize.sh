#!/bin/bash
# Host-side sanitizer pass: the HOST half of every translation unit of the library is compiled with
# -fsanitize=address,undefined (the device code is untouched: -Xarch_host), linked into fastecc_amd/lib/libfastecc_hip_asan.so, and the
# test harness is run against it (FASTECC_HIP_LIB) with the sanitizer runtime preloaded into python.
#   tools/sanitize.sh build            compile + link (no GPU needed)
#   tools/sanitize.sh cpu  [outdir]    tests/test_host_logic.py + tests/test_abi.py + tests/test_scrub_host.py + tests/test_scrub_batch_host.py +
#                                      tests/test_update_batch_host.py + tests/test_scrub_erasures_abi.py (no GPU needed)
#   tools/sanitize.sh gpu-all [outdir] the whole -m gpu suite
#   tools/sanitize.sh gpu  [outdir]    one small GPU round trip per row of the scope table (encode, ntt, pack, decode / repair on both paths, mixed
#                                      radix, 64-bit field, sharded incl. all-to-all and fault injection, host stripes)
# Leak checking is off (python itself never frees everything); every other report fails the run: the logs must not contain "ERROR: AddressSanitizer"
# or "runtime error:".
set -u
R=$(cd "$(dirname "$0")/.." && pwd); cd "$R"
MODE=${1:-build}; OUT=${2:-gpurun_out/sanitize}; mkdir -p "$OUT"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
# The runtime: GCC's libasan + libubsan, preloaded.  ROCm's own compiler-rt ASan intercepts hsa_amd_memory_pool_allocate and needs an
# ASan build of the ROCm stack ("AddressSanitizer: out of memory" at the first device allocation with the stock libraries); GCC's runtime has no
# such interceptors and serves the same __asan_* / __ubsan_* ABI (v8), so the library is linked WITHOUT a runtime and takes the preloaded one.
RT="$(gcc -print-file-name=libasan.so) $(gcc -print-file-name=libubsan.so)"
LIB=fastecc_amd/lib/libfastecc_hip_asan.so
OBJ=fastecc_amd/lib/asan; mkdir -p "$OBJ"
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize=function,vptr -Xarch_host -fno-omit-frame-pointer"
build() {
  local pids=()
  for f in fastecc_amd/csrc/*.hip; do
    o=$OBJ/$(basename "${f%.hip}").o
    if [ ! -f "$o" ] || [ "$f" -nt "$o" ] || [ -n "$(find fastecc_amd/csrc include -name '*.h*' -newer "$o" | head -1)" ]; then
      $HIPCC --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -Wno-unused-function $SAN -c "$f" -o "$o" & pids+=($!)
    fi
  done
  for p in "${pids[@]:-}"; do [ -n "$p" ] && { wait "$p" || exit 1; }; done
  $HIPCC --offload-arch=gfx950 -shared -fPIC -Wl,--allow-shlib-undefined $OBJ/*.o -o $LIB || exit 1
  echo "built $LIB"
}
run() { # name, pytest args...
  local name=$1; shift
  # (the runtime's dlopen interceptor loses the caller's RUNPATH: torch finds its own libraries through LD_LIBRARY_PATH)
  LD_LIBRARY_PATH="$(python -c 'import torch, os; print(os.path.join(os.path.dirname(torch.__file__), "lib"))'):${LD_LIBRARY_PATH:-}" \
  LD_PRELOAD="$RT" ASAN_OPTIONS=detect_leaks=0:halt_on_error=1:abort_on_error=0:protect_shadow_gap=0 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
    FASTECC_HIP_LIB="$R/$LIB" timeout 1500 python -m pytest "$@" -x -q -p no:cacheprovider ${PYTEST_EXTRA:-} > "$OUT/$name.log" 2>&1
  local rc=$?
  tail -3 "$OUT/$name.log"
  if grep -q "ERROR: AddressSanitizer\|runtime error:" "$OUT/$name.log"; then echo "SANITIZER REPORT in $OUT/$name.log"; grep -n "ERROR: AddressSanitizer\|runtime error:" "$OUT/$name.log" | head; rc=1; fi
  echo "$name rc=$rc"
  return $rc
}
case $MODE in
  build) build ;;
  cpu) [ -f $LIB ] || build; run cpu tests/test_host_logic.py tests/test_abi.py tests/test_scrub_host.py tests/test_scrub_batch_host.py tests/test_update_batch_host.py tests/test_scrub_erasures_abi.py -m "not gpu" ;;
  gpu) [ -f $LIB ] || build
       run gpu tests -m gpu -k "test_encode_matches_oracle or test_ntt_matches or test_scale_blocks or test_few_losses or test_repair_restores or test_split_transform_matches or test_host_stripes or test_mixed_radix_encode or test_other_n_k_over_the_64 or test_decode_transform_is_folded or test_block_distributed or test_a_failure_half_way or test_sharded_decode_and_repair or test_pack or test_first_call or test_codes_with_fewer_parity or test_few_parity_blocks" ;;
  # (the tests that load oracle/_ref are left out: the UNMODIFIED reference frees a new[] array through std::unique_ptr<T> — ntt.cpp:333, noted in
  #  SURVEY.md appendix E — which the preloaded runtime rightly reports as alloc-dealloc-mismatch and aborts on; that is the checker, not the product)
  gpu-all) [ -f $LIB ] || build; run gpu_all tests -m gpu -k "not unmodified_reference and not test_ntt_equals and not test_encode_equals" ;;
  one) [ -f $LIB ] || build; shift; shift; run one "$@" ;;
  *) echo "usage: $0 build|cpu|gpu|gpu-all [outdir]"; exit 2 ;;
esac
