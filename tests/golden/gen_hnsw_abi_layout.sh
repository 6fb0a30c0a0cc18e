#!/bin/bash
# Generates tests/golden/hnsw_abi_layout.txt from the REFERENCE's C headers (run where the reference tree exists), the
# way gen_vamana_abi_layout.sh does for the Vamana structs.
set -e
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$(cd "$HERE/../.." && pwd)
REF=${REF:-/root/reference}
STUB=$(mktemp -d)
cat > $STUB/cuda_runtime.h <<'EOS'
typedef struct CUstream_st* cudaStream_t;
typedef enum { CUDA_R_16F = 2, CUDA_R_32F = 0, CUDA_R_8I = 3, CUDA_R_8U = 8 } cudaDataType_t;
EOS
mkdir -p $STUB/dlpack && cp $ROOT/include/dlpack/dlpack.h $STUB/dlpack/
gcc -I$STUB -I$REF/c/include $HERE/hnsw_abi_probe.c -o $STUB/probe_ref
$STUB/probe_ref > $HERE/hnsw_abi_layout.txt
echo "wrote $HERE/hnsw_abi_layout.txt"
