// Merged convolution along a STRIDED last axis whose length is 7-smooth and no power of two (the last axis of a 2-D / 3-D performConvolution plan): forward
// FFT of a tile of neighbouring columns -> product with the kernel spectrum -> inverse FFT (swap identity) -> scale, store, in place.  The column-tile sibling
// of mix_conv_row_kernel (kernel_mix_conv.h) and the mixed-radix sibling of pow2_col_blue_kernel MODE 6 (kernel_pow2.h); the reference's convolution-merged
// axis (vkFFT_Convolution.h:125).  It is the COL = 1 Bluestein arm of mixconv_kernel (kernel_mixconv.h) without the two chirp products: mc_stage (mix_stage.h)
// between two functors on a compile-time MixSched, ONE LDS buffer of L x (TC + 1) elements that is the exchange buffer of the stages and carries the spectrum
// times the kernel spectrum between the phases; the caller's kernel spectrum stands where FFT(chirp) stood.  One read and one write of the data where the
// separate passes (last axis forward, conv_pointwise_kernel, last axis backwards) make three of each.
//
// One workgroup per tile of TC neighbouring columns, TPF threads per column, lanes along the columns (f = tid % TC, tau = tid / TC): every global access is a
// TC-element segment.  Element j of column x sits at x * dim[0].inStride + j * inStrideJ.  dim[1] is the other spatial dimension (3-D plans), dim[2] the
// systems b * cf + v (batch b, coordinate v of cf = coordinateFeatures): system g2 is multiplied element-wise with kernel system g2 % cf.  No kernel matrix
// here (all m systems of a tile at once do not fit LDS at a useful tile width): such plans keep conv_pointwise_kernel.
// On an R2C plan the last axis is a complex axis over size[0] / 2 + 1 columns: the same kernel, no pairing, every conjugation mode.
#pragma once
#include "engine.h"
#include "butterflies.h"
#include "memops.h"
#include "mix_sched.h"
#include "mix_stage.h"

namespace vkfft_mi355x {

// PassParams: dim[0] = columns (count W, stride between neighbouring columns), dim[1] / dim[2] as above, inStrideJ = elements between consecutive points of a
// column, tilesPerG0 = tiles of TC columns, convCf, convConj (0, 1: conj of the data spectrum, 2: conj of the kernel), scale, padInL / padInN: the zero-padded
// range of the axis (not read, not written), lut = stage twiddles of SCH, out = the data.  aux2 = kernel spectra, addressed as pow2_col_blue_kernel MODE 6
// addresses them: value (x, k) of kernel system v at x + k * convKerStrideJ + g1 * convKerStride1 + g2 * convKerStride2 + v * convKerSysStride.
template <typename T, typename SCH, int TPF, int TC>
__global__ void __launch_bounds__(TPF * TC) mix_conv_col_kernel(const PassParams p) {
	constexpr int L = SCH::N, NT = TPF * TC;
	constexpr int LS = TC + 1; // LDS pitch between consecutive elements of one column: lanes along the columns, conflict-free without padding
	constexpr bool waveOnly = NT <= 64; // the whole tile is one wavefront
	constexpr uint32_t ES = (uint32_t)sizeof(cx<T>);
	static_assert((size_t)L * LS * sizeof(cx<T>) <= 160 * 1024, "LDS");
	__shared__ cx<T> lds[L * LS];
	const uint32_t tid = threadIdx.x;
	const uint32_t f = tid % TC, tau = tid / TC;
	uint32_t wg = p.reverseTiles ? gridDim.x - 1u - blockIdx.x : blockIdx.x;
	const uint32_t tile = wg % p.tilesPerG0;
	wg /= p.tilesPerG0;
	const uint32_t g1 = wg % p.dim[1].count, g2 = wg / p.dim[1].count;
	const uint32_t col0 = tile * TC;
	const bool valid = col0 + f < p.dim[0].count; // (columns beyond the last one: out-of-range lane offsets, no branches around memory operations)
	const GBuf glut = make_gbuf(p.lut);
	const GBuf gdat = make_gbuf((cx<T>*)p.out + ((int64_t)g1 * p.dim[1].outStride + (int64_t)g2 * p.dim[2].outStride + (int64_t)col0 * p.dim[0].outStride));
	const GBuf gker = make_gbuf((const cx<T>*)p.aux2 + ((int64_t)g1 * p.convKerStride1 + (int64_t)g2 * p.convKerStride2 + (int64_t)(g2 % p.convCf) * p.convKerSysStride + (int64_t)col0));
	// element j of this thread's column: byte offset lane + j * sJ; kernel value k: klane + k * sK (unit stride along the tile)
	const uint32_t sJ = (uint32_t)p.outStrideJ * ES, sK = (uint32_t)p.convKerStrideJ * ES;
	const uint32_t lane = valid ? f * (uint32_t)p.dim[0].outStride * ES : kGbInvalid, klane = valid ? f * ES : kGbInvalid;
	const bool kconj = p.convConj == 2, xconj = p.convConj == 1;
	const T sc = (T)p.scale;
	cx<T>* const col = lds + f;
	auto padded = [&](uint32_t j) -> bool { return j - p.padInL < p.padInN; }; // the caller's zero-padded range (vkFFT_Zeropad.h:28)
	auto fsync = [&]() { if (waveOnly) VKFFT_WAVE_SYNC(); else VKFFT_SYNC(); };

	mc_stage<T, SCH, 0, TPF, LS, false, false, true>(col, glut, tau, waveOnly,
	                                   [&](uint32_t t, uint32_t c) -> cx<T> { // lanes of the padded range load nothing: zero
		                                   return gb_load<T>(gdat, (valid && !padded(t + c)) ? lane + t * sJ : kGbInvalid, c * sJ);
	                                   },
	                                   // spectrum point k = t + c times its kernel value, re/im swapped for the inverse transform, into the carrier
	                                   [&](uint32_t t, uint32_t c, cx<T> v) {
		                                   cx<T> h = gb_load<T>(gker, valid ? klane + t * sK : kGbInvalid, c * sK);
		                                   if (kconj) h = cconj(h);
		                                   if (xconj) v = cconj(v);
		                                   col[(t + c) * LS] = cswap(cmul(h, v));
	                                   });
	fsync();
	mc_stage<T, SCH, 0, TPF, LS, false, true, false>(col, glut, tau, waveOnly, [&](uint32_t t, uint32_t c) -> cx<T> { return col[(t + c) * LS]; },
	                                   [&](uint32_t t, uint32_t c, cx<T> v) { // ... and store nothing
		                                   cx<T> y = cswap(v);
		                                   if (sc != (T)1) y = cscale(y, sc);
		                                   gb_store<T>(gdat, (valid && !padded(t + c)) ? lane + t * sJ : kGbInvalid, c * sJ, y);
	                                   });
}

// ---- registry ---------------------------------------------------------------------------------------------------
struct MixConvColVariant {
	int n; bool dp; int rad[5]; int tpf; int tc;
	void (*launch)(const PassParams&, dim3, hipStream_t);
};
template <typename T, typename SCH, int TPF, int TC> void mix_conv_col_launch(const PassParams& prm, dim3 grid, hipStream_t s) {
	hipLaunchKernelGGL((mix_conv_col_kernel<T, SCH, TPF, TC>), grid, dim3(TPF * TC), 0, s, prm);
}
#define VKFFT_MCC(T, dp, r0, r1, r2, r3, r4, tpf, tc) \
	{ (r0) * (r1) * (r2) * (r3) * (r4), dp, {r0, r1, r2, r3, r4}, tpf, tc, &mix_conv_col_launch<T, MixSched<r0, r1, r2, r3, r4>, tpf, tc> },

} // namespace vkfft_mi355x
