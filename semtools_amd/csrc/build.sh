#!/usr/bin/env bash
# Builds semtools_amd/lib/libsemtools_hip.so for gfx950 (cross-compiles without a GPU).
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
out="$here/../lib"
mkdir -p "$out"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS=(--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-result -fno-gpu-rdc)
objs=()
pids=()
n_cpu="$(nproc)"
jobs_max="${BUILD_JOBS:-$(( n_cpu < 16 ? n_cpu : 16 ))}"   # min(nproc, 16): the build machines are shared
newest_hdr="$(ls -t "$here"/*.h "$here"/host/*.h "$here"/../../include/*.h | head -1)"
for src in api.cpp search.cpp corpus_io.cpp group.cpp group_exchange.cpp sharded_search.cpp sharded.cpp scan_topk.hip scan_pair.hip scan_wide.hip scan_deep.hip scan_launch.hip select.hip merge.hip range_tables.hip embed_kernels.hip tokenize_kernels.hip wordpiece_kernels.hip wordpiece_utf8_kernels.hip unigram_kernels.hip unigram_utf8_kernels.hip unigram_long_kernels.hip unigram_long_rules_kernels.hip unigram_rules_kernels.hip lower_kernels.hip gemm_topk.hip gemm_rowreg.hip gemm_ldsrow.hip gemm_level.hip largek.hip topk_large.hip compact.hip threshold.hip domain.hip ivfpq_build.hip ivfpq_search.hip ivfpq_io.hip ivfpq_compact.hip host/host.cpp host/store.cpp host/output.cpp host/hf_tokenizer.cpp host/device_tokenize.cpp host/host_capi.cpp; do
  base="$(basename "${src%.*}")"
  obj="$out/$base.o"
  if [[ ! -f "$obj" || "$here/$src" -nt "$obj" || "$newest_hdr" -nt "$obj" ]]; then
    "$HIPCC" "${FLAGS[@]}" -x hip -c "$here/$src" -o "$obj" ${EXTRA_HIPCC_FLAGS:-} &
    pids+=($!)
    while (( $(jobs -rp | wc -l) >= jobs_max )); do wait -n || { echo "compile failed" >&2; exit 1; }; done
  fi
  objs+=("$obj")
done
for pid in "${pids[@]}"; do wait "$pid" || { echo "compile failed" >&2; exit 1; }; done
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -pthread "${objs[@]}" -ldl -o "$out/libsemtools_hip.so"
echo "built $out/libsemtools_hip.so"
# CLI replica (host-only C++), finds the library next to it
bin="$here/../bin"
mkdir -p "$bin"
g++ -O2 -std=c++17 -Wall "$here/host/cli.cpp" -o "$bin/semtools" -L"$out" -lsemtools_hip -Wl,-rpath,'$ORIGIN/../lib' -Wl,-rpath,/opt/rocm/lib
echo "built $bin/semtools"
