/* Prints sizes/offsets of the Vamana C-ABI structs. Compiled twice: against the reference's c/include
 * (tests/golden/gen_vamana_abi_layout.sh -> vamana_abi_layout.txt, committed) and against this repo's include/. */
#include <stddef.h>
#include <stdio.h>
#include <cuvs/neighbors/vamana.h>
#define SZ(T) printf("sizeof " #T " %zu\n", sizeof(T))
#define OFF(T, F) printf("offsetof " #T "." #F " %zu\n", offsetof(T, F))
int main(void)
{
  SZ(struct cuvsVamanaIndexParams);
  OFF(struct cuvsVamanaIndexParams, metric); OFF(struct cuvsVamanaIndexParams, graph_degree);
  OFF(struct cuvsVamanaIndexParams, visited_size); OFF(struct cuvsVamanaIndexParams, vamana_iters);
  OFF(struct cuvsVamanaIndexParams, alpha); OFF(struct cuvsVamanaIndexParams, max_fraction);
  OFF(struct cuvsVamanaIndexParams, batch_base); OFF(struct cuvsVamanaIndexParams, queue_size);
  OFF(struct cuvsVamanaIndexParams, reverse_batchsize);
  SZ(cuvsVamanaIndexParams_t);
  SZ(cuvsVamanaIndex);
  OFF(cuvsVamanaIndex, addr); OFF(cuvsVamanaIndex, dtype);
  SZ(cuvsVamanaIndex_t);
  return 0;
}
