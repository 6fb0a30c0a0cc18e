/* Prints sizes/offsets/values of the binary quantizer's C-ABI structs and enum. Compiled twice: against the reference's
 * c/include (tests/golden/gen_binary_quantizer_abi_layout.sh -> binary_quantizer_abi_layout.txt, committed) and against this
 * repo's include/. */
#include <stddef.h>
#include <stdio.h>
#include <cuvs/preprocessing/quantize/binary.h>
#define SZ(T) printf("sizeof " #T " %zu\n", sizeof(T))
#define OFF(T, F) printf("offsetof " #T "." #F " %zu\n", offsetof(T, F))
#define VAL(E) printf("value " #E " %d\n", (int)(E))
int main(void)
{
  SZ(enum cuvsBinaryQuantizerThreshold);
  VAL(ZERO); VAL(MEAN); VAL(SAMPLING_MEDIAN);
  SZ(struct cuvsBinaryQuantizerParams);
  OFF(struct cuvsBinaryQuantizerParams, threshold); OFF(struct cuvsBinaryQuantizerParams, sampling_ratio);
  SZ(cuvsBinaryQuantizer);
  OFF(cuvsBinaryQuantizer, addr); OFF(cuvsBinaryQuantizer, dtype);
  return 0;
}
