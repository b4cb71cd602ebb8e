// One-launch convolution of unit-stride power-of-two rows (a ONE-dimensional performConvolution plan): forward FFT -> product with the row's kernel
// spectrum -> inverse FFT (swap identity) -> scale, store.  The row form of pow2_col_blue_kernel MODE 6 and the single-kernel form of the reference's
// convolution-merged axis (vkFFT_Convolution.h:125); choreography of pow2_blue_kernel (kernel_pow2.h) without the chirp products, with all E points
// of a thread loaded and the caller's kernel spectrum in the place of FFT(chirp).  One read and one write of the data instead of three each.
//
// Row slot r = b * cf + v (batch b, coordinate v of cf = coordinateFeatures) is multiplied with kernel system v, the layout conv_pointwise_kernel reads
// (kernels_aux.hip).  Register m of a thread holds point tau + m*TPF on the way in, at the spectrum and on the way out, so the kernel values a thread
// needs depend only on its row's coordinate: the workgroup is persistent and keeps them in registers when the coordinate of slot f is the same in
// every tile (cf divides FPW); otherwise they are read again per tile (N points shared by every batch: cache traffic).
//
// REAL (performR2C, in-place layout of N + 2 reals per row): the spectrum of a real kernel is Hermitian and the product is linear, so two real rows
// a, b of the same coordinate travel as z = a + i b through ONE complex transform: FFT(z) H = FFT(a) H + i FFT(b) H, and the inverse separates them
// again into real and imaginary part — no split maps.  A slot is the pair of rows (2 q cf + v, (2 q + 1) cf + v); H[k] is read from the half
// spectrum for k <= N/2 and is conj(H[N - k]) above (the imaginary parts of H[0] and H[N/2], which a C2R transform ignores, are ignored here as well).
// The last batch of an odd count runs with a zero imaginary part and nothing is stored for the missing partner; the two padding reals of a row are
// neither read nor written.
#pragma once
#include "kernel_pow2_core.h"

namespace vkfft_mi355x {

// PassParams: dim[0].count = slots, dim[0].inStride = row pitch (complex elements; REAL: reals), convCf, convConj (0, 1: conj of the data spectrum,
// 2: conj of the kernel; REAL: 0), convKerSysStride = complex elements between kernel systems, opN = real rows in the buffer (REAL), scale,
// padInL / padInN = padOutL / padOutN: the zero-padded range of the axis (not read, not written), aux2 = kernel spectra
template <typename T, typename SCH, int FPW, bool REAL>
__global__ void __launch_bounds__(((1 << SCH::LOGN) >> SCH::LOGE) * FPW) pow2_conv_row_kernel(const PassParams p) {
	constexpr int LOGN = SCH::LOGN, N = 1 << LOGN, LOGE = SCH::LOGE, E = 1 << LOGE, TPF = N / E;
	constexpr int LDSPF = SCH::NS > 1 ? N + (N >> LOGE) : 1;
	constexpr bool waveOnly = TPF <= 64;
	constexpr uint32_t ES = (uint32_t)sizeof(cx<T>), RS = (uint32_t)sizeof(T);
	__shared__ cx<T> lds[FPW * LDSPF];
	const uint32_t tid = threadIdx.x;
	const uint32_t f = tid / TPF, tau = tid % TPF;
	const GBuf glut = make_gbuf(p.lut), gker = make_gbuf(p.aux2);
	const uint32_t cf = p.convCf, pitch = (uint32_t)p.dim[0].inStride, kerSys = (uint32_t)p.convKerSysStride;
	const bool kconj = p.convConj == 2, xconj = p.convConj == 1;
	// kernel spectrum of coordinate v at this thread's points
	cx<T> h[E];
	auto load_kernel = [&](uint32_t v) {
#pragma unroll
		for (int m = 0; m < E; m++) {
			const uint32_t pos = tau + (uint32_t)(m * TPF);
			if constexpr (REAL) {
				const bool upper = pos > (uint32_t)(N / 2);
				cx<T> k = gb_load<T>(gker, (v * kerSys + (upper ? (uint32_t)N - pos : pos)) * ES, 0);
				if (upper) k = cconj(k);
				if (pos == 0u || pos == (uint32_t)(N / 2)) k.y = (T)0;
				h[m] = k;
			} else {
				const cx<T> k = gb_load<T>(gker, (v * kerSys + pos) * ES, 0);
				h[m] = kconj ? cconj(k) : k;
			}
		}
	};
	const bool keep = (uint32_t)FPW % cf == 0u; // slot f of every tile has coordinate f % cf
	if (keep) load_kernel(f % cf);
	// which of this thread's points are read and written: outside the caller's zero-padded range (vkFFT_Zeropad.h:28).  The points do not depend on the
	// tile: the range is tested once, one bit per point (as rdMask / wrMask of pow2_blue_kernel)
	uint32_t ioMask = 0;
#pragma unroll
	for (int m = 0; m < E; m++) if (!(tau + (uint32_t)(m * TPF) - p.padInL < p.padInN)) ioMask |= 1u << m;
	const uint32_t slots = p.dim[0].count, tiles = p.tilesPerG0;
	const T sc = (T)p.scale;
	for (uint32_t wgi = blockIdx.x; wgi < tiles; wgi += gridDim.x) {
		const uint32_t tile = p.reverseTiles ? tiles - 1u - wgi : wgi;
		const uint32_t s0 = tile * FPW, slot = s0 + f;
		const bool valid = slot < slots;
		cx<T> v[E];
		// (REAL: rows of the tile's first slot and of this thread's slot, 2 q cf + v; lane offsets from the former)
		const uint32_t row0 = REAL ? (s0 / cf) * cf + s0 : s0, row = REAL ? (slot / cf) * cf + slot : slot;
		const GBuf gdat = make_gbuf((char*)p.out + (int64_t)row0 * pitch * (REAL ? RS : ES));
		uint32_t laneA, laneB = kGbInvalid;
		if constexpr (REAL) {
			laneA = valid ? ((row - row0) * pitch + tau) * RS : kGbInvalid;
			laneB = valid && row + cf < p.opN ? laneA + cf * pitch * RS : kGbInvalid;
#pragma unroll
			for (int m = 0; m < E; m++) {
				const bool rd = (ioMask >> m) & 1u;
				v[m].x = gb_load_real<T>(gdat, rd ? laneA : kGbInvalid, (uint32_t)(m * TPF) * RS);
				v[m].y = gb_load_real<T>(gdat, rd ? laneB : kGbInvalid, (uint32_t)(m * TPF) * RS);
			}
		} else {
			laneA = valid ? (f * pitch + tau) * ES : kGbInvalid;
#pragma unroll
			for (int m = 0; m < E; m++) v[m] = gb_load<T>(gdat, ((ioMask >> m) & 1u) ? laneA : kGbInvalid, (uint32_t)(m * TPF) * ES);
		}
		if (!keep) load_kernel(valid ? slot % cf : 0u); // (behind the row's loads: needed only after the first transform)
		pow2_stages<T, SCH, 0, TPF, 0, TwGlobal<T>>(v, lds + f * LDSPF, TwGlobal<T>{glut}, tau, waveOnly);
#pragma unroll
		for (int m = 0; m < E; m++) v[m] = cswap(cmul(h[m], xconj ? cconj(v[m]) : v[m]));
		if constexpr (SCH::NS > 1) { if (waveOnly) VKFFT_WAVE_SYNC(); else VKFFT_SYNC(); } // the exchange buffer is reused
		pow2_stages<T, SCH, 0, TPF, 0, TwGlobal<T>>(v, lds + f * LDSPF, TwGlobal<T>{glut}, tau, waveOnly);
#pragma unroll
		for (int m = 0; m < E; m++) {
			cx<T> y = cswap(v[m]);
			if (sc != (T)1) y = cscale(y, sc);
			const bool wr = (ioMask >> m) & 1u;
			if constexpr (REAL) {
				gb_store_real<T>(gdat, wr ? laneA : kGbInvalid, (uint32_t)(m * TPF) * RS, y.x);
				gb_store_real<T>(gdat, wr ? laneB : kGbInvalid, (uint32_t)(m * TPF) * RS, y.y);
			} else gb_store<T>(gdat, wr ? laneA : kGbInvalid, (uint32_t)(m * TPF) * ES, y);
		}
		if constexpr (SCH::NS > 1) { if (waveOnly) VKFFT_WAVE_SYNC(); else VKFFT_SYNC(); }
	}
}

} // namespace vkfft_mi355x
