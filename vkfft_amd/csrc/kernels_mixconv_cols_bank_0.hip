// Translation unit of the merged convolution along a strided 7-smooth last axis against a bank of kernels (kernel_mix_conv_col_bank.h), table part 0 (generated mix_conv_col_bank_table_0.inc).
#include "kernel_mix_conv_col_bank.h"
namespace vkfft_mi355x {
static const MixConvColVariant kTable[] = {
#include "mix_conv_col_bank_table_0.inc"
};
const MixConvColVariant* mix_conv_cols_bank_table_0(int* count) { *count = (int)(sizeof(kTable) / sizeof(kTable[0])); return kTable; }
} // namespace vkfft_mi355x
