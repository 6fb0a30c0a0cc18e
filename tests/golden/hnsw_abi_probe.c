/* Prints sizes/offsets of the HNSW C-ABI structs and the values of its enumerators. Compiled twice: against the reference's
 * c/include (tests/golden/gen_hnsw_abi_layout.sh -> hnsw_abi_layout.txt, committed) and against this repo's include/. */
#include <stddef.h>
#include <stdio.h>
#include <cuvs/neighbors/hnsw.h>
#define SZ(T) printf("sizeof " #T " %zu\n", sizeof(T))
#define OFF(T, F) printf("offsetof " #T "." #F " %zu\n", offsetof(T, F))
int main(void)
{
  printf("enum NONE %d CPU %d GPU %d\n", (int)NONE, (int)CPU, (int)GPU);
  SZ(enum cuvsHnswHierarchy);
  SZ(struct cuvsHnswAceParams);
  OFF(struct cuvsHnswAceParams, npartitions); OFF(struct cuvsHnswAceParams, build_dir); OFF(struct cuvsHnswAceParams, use_disk);
  OFF(struct cuvsHnswAceParams, max_host_memory_gb); OFF(struct cuvsHnswAceParams, max_gpu_memory_gb);
  SZ(struct cuvsHnswIndexParams);
  OFF(struct cuvsHnswIndexParams, hierarchy); OFF(struct cuvsHnswIndexParams, ef_construction);
  OFF(struct cuvsHnswIndexParams, num_threads); OFF(struct cuvsHnswIndexParams, M); OFF(struct cuvsHnswIndexParams, metric);
  OFF(struct cuvsHnswIndexParams, ace_params);
  SZ(cuvsHnswIndex);
  OFF(cuvsHnswIndex, addr); OFF(cuvsHnswIndex, dtype);
  SZ(struct cuvsHnswExtendParams);
  OFF(struct cuvsHnswExtendParams, num_threads);
  SZ(struct cuvsHnswSearchParams);
  OFF(struct cuvsHnswSearchParams, ef); OFF(struct cuvsHnswSearchParams, num_threads);
  SZ(cuvsHnswIndex_t); SZ(cuvsHnswIndexParams_t); SZ(cuvsHnswAceParams_t); SZ(cuvsHnswExtendParams_t); SZ(cuvsHnswSearchParams_t);
  return 0;
}
