/* Prints sizes/offsets of the PCA C-ABI struct and its enum values. Compiled twice: against the reference's c/include
 * (tests/golden/gen_pca_abi_layout.sh -> pca_abi_layout.txt, committed) and against this repo's include/. */
#include <stddef.h>
#include <stdio.h>
#include <cuvs/preprocessing/pca.h>
#define SZ(T) printf("sizeof " #T " %zu\n", sizeof(T))
#define OFF(T, F) printf("offsetof " #T "." #F " %zu\n", offsetof(T, F))
#define VAL(E) printf("value " #E " %d\n", (int)(E))
int main(void)
{
  SZ(enum cuvsPcaSolver);
  VAL(CUVS_PCA_COV_EIG_DQ); VAL(CUVS_PCA_COV_EIG_JACOBI);
  SZ(struct cuvsPcaParams);
  OFF(struct cuvsPcaParams, n_components); OFF(struct cuvsPcaParams, copy); OFF(struct cuvsPcaParams, whiten);
  OFF(struct cuvsPcaParams, algorithm); OFF(struct cuvsPcaParams, tol); OFF(struct cuvsPcaParams, n_iterations);
  SZ(cuvsPcaParams_t);
  return 0;
}
