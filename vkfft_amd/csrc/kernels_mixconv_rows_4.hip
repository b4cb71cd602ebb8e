// Translation unit of the one-launch convolution on 7-smooth rows (kernel_mix_conv.h), table part 4 (generated mix_conv_table_4.inc).
#include "kernel_mix_conv.h"
namespace vkfft_mi355x {
static const MixConvRowVariant kTable[] = {
#include "mix_conv_table_4.inc"
};
const MixConvRowVariant* mix_conv_rows_table_4(int* count) { *count = (int)(sizeof(kTable) / sizeof(kTable[0])); return kTable; }
} // namespace vkfft_mi355x
