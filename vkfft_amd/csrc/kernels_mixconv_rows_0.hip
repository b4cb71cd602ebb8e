// Translation unit of the one-launch convolution on 7-smooth rows (kernel_mix_conv.h), table part 0 (generated mix_conv_table_0.inc).
#include "kernel_mix_conv.h"
namespace vkfft_mi355x {
static const MixConvRowVariant kTable[] = {
#include "mix_conv_table_0.inc"
};
const MixConvRowVariant* mix_conv_rows_table_0(int* count) { *count = (int)(sizeof(kTable) / sizeof(kTable[0])); return kTable; }
} // namespace vkfft_mi355x
