/* Prints sizes/offsets of the IVF-SQ C-ABI structs. Compiled twice: against the reference's c/include
 * (tests/golden/gen_ivf_sq_abi_layout.sh -> ivf_sq_abi_layout.txt, committed) and against this repo's include/. */
#include <stddef.h>
#include <stdio.h>
#include <cuvs/neighbors/ivf_sq.h>
#define SZ(T) printf("sizeof " #T " %zu\n", sizeof(T))
#define OFF(T, F) printf("offsetof " #T "." #F " %zu\n", offsetof(T, F))
int main(void)
{
  SZ(struct cuvsIvfSqIndexParams);
  OFF(struct cuvsIvfSqIndexParams, metric); OFF(struct cuvsIvfSqIndexParams, metric_arg);
  OFF(struct cuvsIvfSqIndexParams, add_data_on_build); OFF(struct cuvsIvfSqIndexParams, n_lists);
  OFF(struct cuvsIvfSqIndexParams, kmeans_n_iters); OFF(struct cuvsIvfSqIndexParams, max_train_points_per_cluster);
  OFF(struct cuvsIvfSqIndexParams, conservative_memory_allocation);
  SZ(struct cuvsIvfSqSearchParams);
  OFF(struct cuvsIvfSqSearchParams, n_probes);
  SZ(cuvsIvfSqIndex);
  OFF(cuvsIvfSqIndex, addr); OFF(cuvsIvfSqIndex, dtype);
  return 0;
}
