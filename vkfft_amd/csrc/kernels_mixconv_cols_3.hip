// Translation unit of the merged convolution along a strided 7-smooth last axis (kernel_mix_conv_col.h), table part 3 (generated mix_conv_col_table_3.inc).
#include "kernel_mix_conv_col.h"
namespace vkfft_mi355x {
static const MixConvColVariant kTable[] = {
#include "mix_conv_col_table_3.inc"
};
const MixConvColVariant* mix_conv_cols_table_3(int* count) { *count = (int)(sizeof(kTable) / sizeof(kTable[0])); return kTable; }
} // namespace vkfft_mi355x
