// Merged convolution along a strided 7-smooth last axis against a BANK of kernels (numberKernels = K > 1 of a 2-D / 3-D performConvolution plan): the
// column-tile sibling of mix_conv_col_kernel (kernel_mix_conv_col.h) that transforms its tile ONCE, keeps the spectrum in registers and runs
// product -> inverse FFT -> scale, store once per kernel.  One read of the data and K writes where the separate passes (last axis forward,
// conv_pointwise_kernel, K times the last axis backwards) make 2 + 2 K reads and writes.  A kernel of its own name, not a flag of mix_conv_col_kernel: the
// plan of one kernel stays that kernel's.
//
// Tile, lanes, strides and the padding test are those of mix_conv_col_kernel.  The last forward stage leaves its outputs in registers (McRegSink of
// mix_stage.h): y[b][k] = spectrum point tau + b * TPF + k * S, S the stride of the last stage; L / TPF values per thread.  The kernels are taken from the
// last to the first (conv_pointwise_kernel's order): result 0 replaces the input, and since a workgroup reads only its own tile, and only once, before it stores
// anything, that order is all the in-place layout needs.  Result f of system g2 lies f * convBankStride elements behind result 0, kernel f's spectra
// f * convKerBankStride elements behind kernel 0's; both resources are re-based per f in 64 bits, so that the spans the planner checked are those of one
// result and one kernel.  The LDS carrier of L x (TC + 1) elements is the only buffer, as in the sibling.  No kernel matrix.
#pragma once
#include "kernel_mix_conv_col.h"

namespace vkfft_mi355x {

// PassParams as for mix_conv_col_kernel, and convNk = K, convBankStride, convKerBankStride.  dim[2] = the coordinates (one batch: the planner rejects a bank
// together with several batches)
template <typename T, typename SCH, int TPF, int TC>
__global__ void __launch_bounds__(TPF * TC) mix_conv_col_bank_kernel(const PassParams p) {
	constexpr int L = SCH::N, NT = TPF * TC;
	constexpr int LS = TC + 1;
	constexpr bool waveOnly = NT <= 64;
	constexpr uint32_t ES = (uint32_t)sizeof(cx<T>);
	// what the last stage of the schedule hands each thread: P butterflies of R outputs, output k of butterfly t at t + k * S
	constexpr int R = SCH::rad[SCH::NS - 1], NB = L / R, P = (NB + TPF - 1) / TPF, S = SCH::S(SCH::NS - 1);
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
	const int64_t datB = (int64_t)g1 * p.dim[1].outStride + (int64_t)g2 * p.dim[2].outStride + (int64_t)col0 * p.dim[0].outStride;
	const int64_t kerB = (int64_t)g1 * p.convKerStride1 + (int64_t)g2 * p.convKerStride2 + (int64_t)(g2 % p.convCf) * p.convKerSysStride + (int64_t)col0;
	const uint32_t sJ = (uint32_t)p.outStrideJ * ES, sK = (uint32_t)p.convKerStrideJ * ES;
	const uint32_t lane = valid ? f * (uint32_t)p.dim[0].outStride * ES : kGbInvalid, klane = valid ? f * ES : kGbInvalid;
	const bool kconj = p.convConj == 2, xconj = p.convConj == 1;
	const T sc = (T)p.scale;
	cx<T>* const col = lds + f;
	auto padded = [&](uint32_t j) -> bool { return j - p.padInL < p.padInN; }; // the caller's zero-padded range (vkFFT_Zeropad.h:28)
	auto fsync = [&]() { if (waveOnly) VKFFT_WAVE_SYNC(); else VKFFT_SYNC(); };

	cx<T> y[P][R]; // the spectrum of this thread's points, kept over the kernels
	{
		const GBuf gdat = make_gbuf((const cx<T>*)p.out + datB);
		mc_stage<T, SCH, 0, TPF, LS, false, false, false>(col, glut, tau, waveOnly,
		                                   [&](uint32_t t, uint32_t c) -> cx<T> { // lanes of the padded range load nothing: zero
			                                   return gb_load<T>(gdat, (valid && !padded(t + c)) ? lane + t * sJ : kGbInvalid, c * sJ);
		                                   },
		                                   McRegSink<T, R>{y});
	}
	if (xconj) {
#pragma unroll
		for (int b = 0; b < P; b++) {
#pragma unroll
			for (int k = 0; k < R; k++) y[b][k] = cconj(y[b][k]);
		}
	}
	for (uint32_t fk = p.convNk; fk-- > 0;) {
		const GBuf gker = make_gbuf((const cx<T>*)p.aux2 + (kerB + (int64_t)fk * p.convKerBankStride));
		const GBuf gres = make_gbuf((cx<T>*)p.out + (datB + (int64_t)fk * p.convBankStride));
		// slower threads may still read the carrier: the last forward stage (first kernel taken; SCH::NS > 1) or the previous inverse's first stage (one-stage
		// schedules read it there and nowhere else)
		fsync();
		// spectrum point t + k * S times its value of kernel fk, re/im swapped for the inverse transform, into the carrier
#pragma unroll
		for (int b = 0; b < P; b++) {
			const uint32_t t = tau + b * TPF;
			if ((b + 1) * TPF <= NB || t < (uint32_t)NB) {
#pragma unroll
				for (int k = 0; k < R; k++) {
					cx<T> h = gb_load<T>(gker, valid ? klane + t * sK : kGbInvalid, (uint32_t)(k * S) * sK);
					if (kconj) h = cconj(h);
					col[(t + (uint32_t)(k * S)) * LS] = cswap(cmul(h, y[b][k]));
				}
			}
		}
		fsync();
		mc_stage<T, SCH, 0, TPF, LS, false, true, false>(col, glut, tau, waveOnly, [&](uint32_t t, uint32_t c) -> cx<T> { return col[(t + c) * LS]; },
		                                   [&](uint32_t t, uint32_t c, cx<T> v) { // ... and store nothing
			                                   cx<T> r = cswap(v);
			                                   if (sc != (T)1) r = cscale(r, sc);
			                                   gb_store<T>(gres, (valid && !padded(t + c)) ? lane + t * sJ : kGbInvalid, c * sJ, r);
		                                   });
	}
}

// ---- registry: the entries are MixConvColVariant, as the sibling's ------------------------------------------------
template <typename T, typename SCH, int TPF, int TC> void mix_conv_col_bank_launch(const PassParams& prm, dim3 grid, hipStream_t s) {
	hipLaunchKernelGGL((mix_conv_col_bank_kernel<T, SCH, TPF, TC>), grid, dim3(TPF * TC), 0, s, prm);
}
#define VKFFT_MCCB(T, dp, r0, r1, r2, r3, r4, tpf, tc) \
	{ (r0) * (r1) * (r2) * (r3) * (r4), dp, {r0, r1, r2, r3, r4}, tpf, tc, &mix_conv_col_bank_launch<T, MixSched<r0, r1, r2, r3, r4>, tpf, tc> },

} // namespace vkfft_mi355x
