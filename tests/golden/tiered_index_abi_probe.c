/* Prints sizes/offsets of the tiered-index C-ABI structs and its enum values. Compiled twice: against the reference's c/include
 * (tests/golden/gen_tiered_index_abi_layout.sh -> tiered_index_abi_layout.txt, committed) and against this repo's include/. */
#include <stddef.h>
#include <stdio.h>
#include <cuvs/neighbors/tiered_index.h>
#define SZ(T) printf("sizeof " #T " %zu\n", sizeof(T))
#define OFF(T, F) printf("offsetof " #T "." #F " %zu\n", offsetof(T, F))
#define VAL(E) printf("value " #E " %d\n", (int)(E))
int main(void)
{
  SZ(cuvsTieredIndexANNAlgo);
  VAL(CUVS_TIERED_INDEX_ALGO_CAGRA); VAL(CUVS_TIERED_INDEX_ALGO_IVF_FLAT); VAL(CUVS_TIERED_INDEX_ALGO_IVF_PQ);
  SZ(cuvsTieredIndex);
  OFF(cuvsTieredIndex, addr); OFF(cuvsTieredIndex, dtype); OFF(cuvsTieredIndex, algo);
  SZ(struct cuvsTieredIndexParams);
  OFF(struct cuvsTieredIndexParams, metric); OFF(struct cuvsTieredIndexParams, algo);
  OFF(struct cuvsTieredIndexParams, min_ann_rows); OFF(struct cuvsTieredIndexParams, create_ann_index_on_extend);
  OFF(struct cuvsTieredIndexParams, cagra_params); OFF(struct cuvsTieredIndexParams, ivf_flat_params);
  OFF(struct cuvsTieredIndexParams, ivf_pq_params);
  return 0;
}
