// One-launch convolution of unit-stride rows whose length is 7-smooth and no power of two (a ONE-dimensional performConvolution plan): forward FFT ->
// product with the row's kernel spectrum -> inverse FFT (swap identity) -> scale, store.  The mixed-radix sibling of pow2_conv_row_kernel
// (kernel_pow2_conv.h) and the single-kernel form of the reference's convolution-merged axis (vkFFT_Convolution.h:125).  It is the Bluestein arm of
// mixconv_kernel (kernel_mixconv.h, RADER = 0, COL = 0) without the two chirp products: mc_stage (mix_stage.h) between two functors on a compile-time
// MixSched, ONE LDS buffer per row that is the exchange buffer of the stages and carries the spectrum times the kernel spectrum between the phases; the
// caller's kernel spectrum stands where FFT(chirp) stood.  One read and one write of the data instead of three each.
//
// Row slot r = b * cf + v (batch b, coordinate v of cf = coordinateFeatures) is multiplied with kernel system v, the layout conv_pointwise_kernel reads
// (kernels_aux.hip).  One workgroup per tile of FPW slots, TPF threads each; the kernel spectrum is read per tile (N points shared by every batch: cache
// traffic).
//
// REAL (performR2C, even N, in-place layout of N + 2 reals per row): two real rows a, b of the same coordinate travel as z = a + i b through ONE complex
// transform, as in kernel_pow2_conv.h.  A slot is the pair of rows (2 q cf + v, (2 q + 1) cf + v); H[k] is read from the half spectrum for k <= N/2 and
// is conj(H[N - k]) above, the imaginary parts of H[0] and H[N/2] are ignored.  The last batch of an odd count runs with a zero imaginary part and nothing
// is stored for the missing partner; the two padding reals of a row are neither read nor written.
//
// DENSE (compile time, from TPF): when the threads of one row cover less than a 256-byte segment a wave's lanes are whole rows apart.
// Such instances move the tile as contiguous runs into the carrier rows and out of them (the denseIn / denseOut loops of the Rader arm) and mc_stage
// reads and writes the buffer (SF / SL).  Longer rows load in the first stage of the forward transform and store in the last stage of the inverse one.
#pragma once
#include "engine.h"
#include "butterflies.h"
#include "memops.h"
#include "mix_sched.h"
#include "mix_stage.h"

namespace vkfft_mi355x {

// PassParams: dim[0].count = slots, dim[0].inStride = row pitch (complex elements; REAL: reals), convCf, convConj (0, 1: conj of the data spectrum,
// 2: conj of the kernel; REAL: 0), convKerSysStride = complex elements between kernel systems, opN = real rows in the buffer (REAL), scale,
// padInL / padInN: the zero-padded range of the axis (not read, not written), lut = stage twiddles of SCH, aux2 = kernel spectra, out = the data
template <typename T, typename SCH, int TPF, int FPW, bool REAL>
__global__ void __launch_bounds__(TPF * FPW) mix_conv_row_kernel(const PassParams p) {
	constexpr int N = SCH::N, NT = TPF * FPW;
	constexpr uint32_t ES = (uint32_t)sizeof(cx<T>), RS = (uint32_t)sizeof(T);
	constexpr bool DENSE = (uint32_t)TPF * (REAL ? RS : ES) < 256u;
	constexpr int EXPF = SCH::NS > 1 ? MixPad<SCH, TPF, (int)sizeof(cx<T>)>::elems() : 1;
	constexpr int SP = (EXPF > N ? EXPF : N) | 1; // rows of a tile: odd pitch
	constexpr bool waveOnly = (TPF <= 64) && (64 % TPF == 0); // a transform never straddles wavefronts
	static_assert(!REAL || N % 2 == 0, "pairs of real rows: even lengths");
	static_assert((size_t)FPW * SP * sizeof(cx<T>) <= 160 * 1024, "LDS");
	__shared__ cx<T> rows[FPW * SP];
	const uint32_t tid = threadIdx.x;
	const uint32_t f = tid / TPF, tau = tid % TPF;
	const GBuf glut = make_gbuf(p.lut), gker = make_gbuf(p.aux2);
	const uint32_t cf = p.convCf, pitch = (uint32_t)p.dim[0].inStride, slots = p.dim[0].count;
	const bool kconj = p.convConj == 2, xconj = p.convConj == 1;
	const uint32_t tile = p.reverseTiles ? gridDim.x - 1u - blockIdx.x : blockIdx.x;
	const uint32_t s0 = tile * FPW, slot = s0 + f;
	const bool valid = slot < slots;
	// (REAL: rows of the tile's first slot and of this thread's slot, 2 q cf + v; lane offsets from the former)
	const uint32_t row0 = REAL ? (s0 / cf) * cf + s0 : s0, row = REAL ? (slot / cf) * cf + slot : slot;
	const GBuf gdat = make_gbuf((char*)p.out + (int64_t)row0 * pitch * (REAL ? RS : ES));
	const uint32_t laneA = valid ? (row - row0) * pitch * (REAL ? RS : ES) : kGbInvalid;
	const uint32_t laneB = REAL && valid && row + cf < p.opN ? laneA + cf * pitch * RS : kGbInvalid;
	const uint32_t kbase = (valid ? slot % cf : 0u) * (uint32_t)p.convKerSysStride * ES;
	const T sc = (T)p.scale;
	cx<T>* const line = rows + f * SP;
	auto padded = [&](uint32_t j) -> bool { return j - p.padInL < p.padInN; }; // the caller's zero-padded range (vkFFT_Zeropad.h:28)
	auto fsync = [&]() { if (waveOnly) VKFFT_WAVE_SYNC(); else VKFFT_SYNC(); };
	auto fromLine = [&](uint32_t t, uint32_t c) -> cx<T> { return line[t + c]; };
	// spectrum point k = t + c of this thread's row times its kernel value, re/im swapped for the inverse transform, into the carrier row
	auto product = [&](uint32_t t, uint32_t c, cx<T> v) {
		const uint32_t k = t + c;
		cx<T> h;
		if constexpr (REAL) {
			const bool upper = k > (uint32_t)(N / 2);
			h = gb_load<T>(gker, kbase + (upper ? (uint32_t)N - k : k) * ES, 0);
			if (upper) h = cconj(h);
			if (k == 0u || k == (uint32_t)(N / 2)) h.y = (T)0;
		} else {
			h = gb_load<T>(gker, kbase + t * ES, c * ES);
			if (kconj) h = cconj(h);
			if (xconj) v = cconj(v);
		}
		line[k] = cswap(cmul(h, v));
	};
	auto fin = [&](cx<T> v) -> cx<T> { v = cswap(v); if (sc != (T)1) v = cscale(v, sc); return v; };

	if constexpr (DENSE) {
		// the tile as it lies in memory -> carrier rows.  C2C: FPW * N consecutive elements.  REAL: 2 FPW real rows, local row r2 = (slot r2 / 2, half r2 % 2):
		// consecutive rows of memory when cf = 1, runs of N reals otherwise
		constexpr uint32_t TOT = (uint32_t)(REAL ? 2 : 1) * FPW * N;
		constexpr int CNT = (int)((TOT + NT - 1) / NT);
		const uint32_t here = slots - s0 < (uint32_t)FPW ? slots - s0 : (uint32_t)FPW;
		auto realOff = [&](uint32_t ls, uint32_t h, uint32_t j) -> uint32_t { // byte offset of real j of half h of local slot ls, or invalid
			const uint32_t s = s0 + ls, r = (s / cf) * cf + s + h * cf;
			return (ls < here && r < p.opN && !padded(j)) ? ((r - row0) * pitch + j) * RS : kGbInvalid;
		};
#pragma unroll
		for (int i = 0; i < CNT; i++) {
			const uint32_t e = tid + (uint32_t)(i * NT);
			if ((uint32_t)((i + 1) * NT) <= TOT || e < TOT) {
				const uint32_t r = e / (uint32_t)N, j = e % (uint32_t)N;
				if constexpr (REAL) {
					const T x = gb_load_real<T>(gdat, realOff(r >> 1, r & 1u, j), 0);
					if (r & 1u) rows[(r >> 1) * SP + j].y = x; else rows[(r >> 1) * SP + j].x = x;
				} else rows[r * SP + j] = gb_load<T>(gdat, (r < here && !padded(j)) ? e * ES : kGbInvalid, 0);
			}
		}
		VKFFT_SYNC();
		mc_stage<T, SCH, 0, TPF, 1, true, true, true>(line, glut, tau, waveOnly, fromLine, product);
		fsync();
		mc_stage<T, SCH, 0, TPF, 1, true, true, true>(line, glut, tau, waveOnly, fromLine, [&](uint32_t t, uint32_t c, cx<T> v) { line[t + c] = fin(v); });
		VKFFT_SYNC();
#pragma unroll
		for (int i = 0; i < CNT; i++) {
			const uint32_t e = tid + (uint32_t)(i * NT);
			if ((uint32_t)((i + 1) * NT) <= TOT || e < TOT) {
				const uint32_t r = e / (uint32_t)N, j = e % (uint32_t)N;
				if constexpr (REAL) {
					const cx<T> y = rows[(r >> 1) * SP + j];
					gb_store_real<T>(gdat, realOff(r >> 1, r & 1u, j), 0, (r & 1u) ? y.y : y.x);
				} else gb_store<T>(gdat, (r < here && !padded(j)) ? e * ES : kGbInvalid, 0, rows[r * SP + j]);
			}
		}
	} else {
		mc_stage<T, SCH, 0, TPF, 1, true, false, true>(line, glut, tau, waveOnly,
		                                  [&](uint32_t t, uint32_t c) -> cx<T> {
			                                  const bool rd = !padded(t + c); // lanes of the padded range load nothing: zero
			                                  if constexpr (REAL) {
				                                  cx<T> v;
				                                  v.x = gb_load_real<T>(gdat, rd ? laneA + t * RS : kGbInvalid, c * RS);
				                                  v.y = gb_load_real<T>(gdat, rd ? laneB + t * RS : kGbInvalid, c * RS);
				                                  return v;
			                                  } else return gb_load<T>(gdat, rd ? laneA + t * ES : kGbInvalid, c * ES);
		                                  },
		                                  product);
		fsync();
		mc_stage<T, SCH, 0, TPF, 1, true, true, false>(line, glut, tau, waveOnly, fromLine, [&](uint32_t t, uint32_t c, cx<T> v) {
			const bool wr = !padded(t + c); // ... and store nothing
			const cx<T> y = fin(v);
			if constexpr (REAL) {
				gb_store_real<T>(gdat, wr ? laneA + t * RS : kGbInvalid, c * RS, y.x);
				gb_store_real<T>(gdat, wr ? laneB + t * RS : kGbInvalid, c * RS, y.y);
			} else gb_store<T>(gdat, wr ? laneA + t * ES : kGbInvalid, c * ES, y);
		});
	}
}

// ---- registry ---------------------------------------------------------------------------------------------------
struct MixConvRowVariant {
	int n; bool dp; bool real; int rad[5]; int tpf; int fpw;
	void (*launch)(const PassParams&, dim3, hipStream_t);
};
template <typename T, typename SCH, int TPF, int FPW, bool REAL> void mix_conv_row_launch(const PassParams& prm, dim3 grid, hipStream_t s) {
	hipLaunchKernelGGL((mix_conv_row_kernel<T, SCH, TPF, FPW, REAL>), grid, dim3(TPF * FPW), 0, s, prm);
}
#define VKFFT_MCR(T, dp, real, r0, r1, r2, r3, r4, tpf, fpw) \
	{ (r0) * (r1) * (r2) * (r3) * (r4), dp, real, {r0, r1, r2, r3, r4}, tpf, fpw, &mix_conv_row_launch<T, MixSched<r0, r1, r2, r3, r4>, tpf, fpw, real> },

} // namespace vkfft_mi355x
