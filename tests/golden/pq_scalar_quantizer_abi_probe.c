/* Prints sizes/offsets of the product and scalar quantizers' C-ABI structs. Compiled twice: against the reference's c/include
 * (tests/golden/gen_pq_scalar_quantizer_abi_layout.sh -> pq_scalar_quantizer_abi_layout.txt, committed) and against this
 * repo's include/. */
#include <stddef.h>
#include <stdio.h>
#include <cuvs/preprocessing/quantize/pq.h>
#include <cuvs/preprocessing/quantize/scalar.h>
#define SZ(T) printf("sizeof " #T " %zu\n", sizeof(T))
#define OFF(T, F) printf("offsetof " #T "." #F " %zu\n", offsetof(T, F))
#define VAL(E) printf("value " #E " %d\n", (int)(E))
int main(void)
{
  SZ(cuvsKMeansType);
  VAL(CUVS_KMEANS_TYPE_KMEANS); VAL(CUVS_KMEANS_TYPE_KMEANS_BALANCED);
  SZ(struct cuvsProductQuantizerParams);
  OFF(struct cuvsProductQuantizerParams, pq_bits); OFF(struct cuvsProductQuantizerParams, pq_dim);
  OFF(struct cuvsProductQuantizerParams, use_subspaces); OFF(struct cuvsProductQuantizerParams, use_vq);
  OFF(struct cuvsProductQuantizerParams, vq_n_centers); OFF(struct cuvsProductQuantizerParams, kmeans_n_iters);
  OFF(struct cuvsProductQuantizerParams, pq_kmeans_type); OFF(struct cuvsProductQuantizerParams, max_train_points_per_pq_code);
  OFF(struct cuvsProductQuantizerParams, max_train_points_per_vq_cluster);
  SZ(cuvsProductQuantizer);
  OFF(cuvsProductQuantizer, addr); OFF(cuvsProductQuantizer, dtype);
  SZ(struct cuvsScalarQuantizerParams);
  OFF(struct cuvsScalarQuantizerParams, quantile);
  SZ(cuvsScalarQuantizer);
  OFF(cuvsScalarQuantizer, min_); OFF(cuvsScalarQuantizer, max_);
  return 0;
}
