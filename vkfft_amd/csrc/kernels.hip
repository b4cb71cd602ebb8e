// Kernel instantiations and the launch layer (the counterpart of the reference's hipModuleLaunchKernel
// glue, vkFFT_DispatchPlan.h:226-295 — but on ahead-of-time compiled gfx950 kernels).
#include "engine.h"
#include "kernel_generic.h"
#include "kernel_opfft.h"
#include "kernel_mixed.h"
#include "kernel_mixconv.h"
#include "kernel_mix_conv.h"
#include "kernel_mix_conv_col.h"
#include <cstdio>
#include <cstdlib>
#include <algorithm>

namespace vkfft_mi355x {

int launch_pass(const PassPlan& pp, const PassParams& prm, hipStream_t stream) {
	const uint64_t grid64 = (uint64_t)prm.tilesPerG0 * (prm.colMerge ? 1u : prm.dim[1].count) * prm.dim[2].count;
	if (grid64 == 0) return 0;
	if (grid64 > 0x7fffffffull) return 4039;
	const dim3 grid((uint32_t)grid64), block(pp.threads);
	switch (pp.kernel) {
	case KERNEL_GENERIC:
		if (pp.dp) hipLaunchKernelGGL(generic_pass_kernel<double>, grid, block, pp.ldsBytes, stream, prm);
		else hipLaunchKernelGGL(generic_pass_kernel<float>, grid, block, pp.ldsBytes, stream, prm);
		break;
	case KERNEL_POW2_ROW:
	case KERNEL_POW2_COL:
		return launch_pow2(pp, prm, stream);
	case KERNEL_POW2_BLUE:
		return launch_pow2_blue(pp, prm, stream);
	case KERNEL_POW2_COL_BLUE:
		return launch_pow2_col_blue(pp, prm, stream);
	case KERNEL_POW2_CONV_ROW:
		return launch_pow2_conv_row(pp, prm, stream);
	case KERNEL_MIX_CONV_ROW:
		return launch_mix_conv_row(pp, prm, stream);
	case KERNEL_MIX_CONV_COL:
		return launch_mix_conv_col(pp, prm, stream);
	case KERNEL_MIX_CONV_COL_BANK:
		return launch_mix_conv_col_bank(pp, prm, stream);
	case KERNEL_TRANSPOSE:
		return launch_transpose(pp, prm, stream);
	case KERNEL_REAL_MAP:
		return launch_real_map(pp, prm, stream);
	case KERNEL_POW2_BLUE_R2R:
		return launch_pow2_blue_r2r(pp, prm, stream);
	case KERNEL_MIXED_ROW:
		return launch_mixed(pp, prm, stream);
	case KERNEL_MIXCONV:
		return launch_mixconv(pp, prm, stream);
	case KERNEL_OPFFT:
		return launch_opfft(pp, prm, stream);
	case KERNEL_R2C_PAIR: {
		const uint32_t npair = (prm.opN >> 2) + 1;
		const uint64_t rows = (uint64_t)prm.dim[0].count * prm.dim[1].count * prm.dim[2].count;
		if (rows > 65535) { // grid.y limit: split over dim[2]/dim[1] on the host
			PassParams q = prm;
			if (prm.dim[2].count > 1) {
				for (uint32_t i = 0; i < prm.dim[2].count; i++) { q.dim[2].count = 1; q.out = (char*)prm.out + (int64_t)i * prm.dim[2].outStride * pp.outElemBytes; int r = launch_pass(pp, q, stream); if (r) return r; }
			} else if (prm.dim[1].count > 1) {
				for (uint32_t i = 0; i < prm.dim[1].count; i++) { q.dim[1].count = 1; q.out = (char*)prm.out + (int64_t)i * prm.dim[1].outStride * pp.outElemBytes; int r = launch_pass(pp, q, stream); if (r) return r; }
			} else {
				for (uint32_t i = 0; i < prm.dim[0].count; i += 32768) { q.dim[0].count = std::min<uint32_t>(32768, prm.dim[0].count - i); q.out = (char*)prm.out + (int64_t)i * prm.dim[0].outStride * pp.outElemBytes; int r = launch_pass(pp, q, stream); if (r) return r; }
			}
			return 0;
		}
		const dim3 g2((npair + 255) / 256, (uint32_t)rows);
		if (pp.dp) hipLaunchKernelGGL(r2c_even_pair_kernel<double>, g2, dim3(256), 0, stream, prm);
		else hipLaunchKernelGGL(r2c_even_pair_kernel<float>, g2, dim3(256), 0, stream, prm);
		break;
	}
	default:
		return 4039;
	}
	return hipGetLastError() == hipSuccess ? 0 : 4039;
}

int launch_on_grid(uint64_t grid64, PassLaunchFn fn, const PassParams& prm, hipStream_t stream) {
	if (grid64 == 0) return 0;
	if (grid64 > 0x7fffffffull || !fn) return 4039;
	fn(prm, dim3((uint32_t)grid64), stream);
	return hipGetLastError() == hipSuccess ? 0 : 4039;
}

// A registry in parts, one translation unit each: PARTS(X) lists the suffixes of `<family>_table_<suffix>(int* count)`; this declares them and defines
// <family>_part(part, &count) and the part count
#define VKFFT_PART_DECL(Variant, family, t) const Variant* family##_table_##t(int*);
#define VKFFT_PART_REF(Variant, family, t) &family##_table_##t,
#define VKFFT_REGISTRY_PARTS(Variant, family, kParts, PARTS) \
	PARTS(VKFFT_PART_DECL, Variant, family) \
	typedef const Variant* (*family##_part_fn)(int*); \
	static const family##_part_fn family##_part_fns[] = { PARTS(VKFFT_PART_REF, Variant, family) }; \
	constexpr int kParts = (int)(sizeof(family##_part_fns) / sizeof(family##_part_fns[0]));

// ---- mixed-radix registry: twenty table parts (kernels_mixed_*.hip).  Parts 6-19: tools/gen_long_rows_table.py — the long rows; the 7-smooth lengths of 4097 ... 8192 points outside the first six tables
#define VKFFT_MIXED_PARTS(X, V, f) X(V, f, 0) X(V, f, 1) X(V, f, 2) X(V, f, 3) X(V, f, 4) X(V, f, 5) X(V, f, 6) X(V, f, 7) X(V, f, 8) X(V, f, 9) \
	X(V, f, 10) X(V, f, 11) X(V, f, 12) X(V, f, 13) X(V, f, 14) X(V, f, 15) X(V, f, 16) X(V, f, 17) X(V, f, 18) X(V, f, 19)
VKFFT_REGISTRY_PARTS(MixedVariant, mixed, kMixedParts, VKFFT_MIXED_PARTS)
static const MixedVariant* mixed_part(int part, int* count) { // (a negative part — of a variant of -1, no instance — has no entries)
	return part < 0 ? nullptr : mixed_part_fns[part % kMixedParts](count);
}
KernelShape mixed_row_lookup(uint64_t n, bool dp) {
	for (int part = 0; part < kMixedParts; part++) {
		int cnt = 0;
		const MixedVariant* tab = mixed_part(part, &cnt);
		for (int i = 0; i < cnt; i++) {
			if ((uint64_t)tab[i].n != n || tab[i].dp != dp) continue;
			KernelShape k;
			k.variant = (part << 16) | i; k.perWg = tab[i].fpw; k.threads = tab[i].tpf * tab[i].fpw;
			for (int r = 0; r < 5; r++) k.sched[r] = tab[i].rad[r];
			return k;
		}
	}
	return {};
}
// rows per workgroup of the variant's form between the maps (kernel_mixed.h mixed_ops_fpw)
int mixed_row_ops_fpw(int variant) {
	int cnt = 0;
	const MixedVariant* tab = mixed_part((variant >> 16) % kMixedParts, &cnt);
	const int idx = variant & 0xffff;
	return (variant < 0 || idx >= cnt) ? 0 : tab[idx].fpwOps;
}
int launch_mixed(const PassPlan& pp, const PassParams& prm, hipStream_t stream) {
	int cnt = 0;
	const MixedVariant* tab = mixed_part((pp.variant >> 16) % kMixedParts, &cnt);
	const int idx = pp.variant & 0xffff;
	const bool known = pp.variant >= 0 && idx < cnt, ops = prm.preOp != OP_NONE || prm.postOp != OP_NONE;
	return launch_on_grid((uint64_t)prm.tilesPerG0 * prm.dim[1].count * prm.dim[2].count, !known ? nullptr : ops ? tab[idx].launchOps : tab[idx].launch, prm, stream);
}

// ---- one-kernel cyclic convolution registry: six table parts (kernels_mixconv_*.hip) ---------------------------------
#define VKFFT_MIXCONV_PARTS(X, V, f) X(V, f, 0) X(V, f, 1) X(V, f, 2) X(V, f, 3) X(V, f, 4) X(V, f, 5)
VKFFT_REGISTRY_PARTS(MixConvVariant, mixconv, kMixConvParts, VKFFT_MIXCONV_PARTS)
static const MixConvVariant* mixconv_part(int part, int* count) {
	return part < 0 ? nullptr : mixconv_part_fns[part % kMixConvParts](count);
}
KernelShape mixconv_lookup(bool rader, bool col, uint64_t pOrMinLen, bool dp) {
	const MixConvVariant* best = nullptr;
	KernelShape k;
	for (int part = 0; part < kMixConvParts; part++) {
		int cnt = 0;
		const MixConvVariant* tab = mixconv_part(part, &cnt);
		for (int i = 0; i < cnt; i++) {
			const MixConvVariant& v = tab[i];
			if (v.dp != dp || (v.rader != 0) != rader || (v.col != 0) != col) continue;
			if (rader ? (uint64_t)v.l + 1 != pOrMinLen : (uint64_t)v.l < pOrMinLen) continue;
			if (best && best->l <= v.l) continue;
			best = &v; k.variant = (part << 16) | i;
		}
	}
	if (!best) return k;
	k.len = (uint64_t)best->l; k.perWg = best->fpw; k.threads = best->tpf * best->fpw;
	for (int i = 0; i < 5; i++) k.sched[i] = best->rad[i];
	return k;
}
bool mixrad_available(int variant) {
	int cnt = 0;
	const MixConvVariant* tab = mixconv_part((variant >> 16) % kMixConvParts, &cnt);
	const int idx = variant & 0xffff;
	return variant >= 0 && idx < cnt && tab[idx].launchRad != nullptr;
}
MixradShape mixrad_geom(int variant) {
	MixradShape g;
	if (!mixrad_available(variant)) return g;
	int cnt = 0;
	const MixConvVariant& v = mixconv_part((variant >> 16) % kMixConvParts, &cnt)[variant & 0xffff];
	g.ok = true; g.sp = v.radSP; g.lutn = v.radLutN; g.groups = v.radGroups; g.groupsDense = v.radGroupsDense;
	return g;
}
int launch_mixconv(const PassPlan& pp, const PassParams& prm, hipStream_t stream) {
	int cnt = 0;
	const MixConvVariant* tab = mixconv_part((pp.variant >> 16) % kMixConvParts, &cnt);
	const int idx = pp.variant & 0xffff;
	const bool known = pp.variant >= 0 && idx < cnt;
	const bool rad = prm.raderM >= 1; // the prime as a stage of the composite length raderM * P (kernel_mixrad.h; 1: the prime's own rows)
	const bool ops = (prm.preOp != OP_NONE || prm.postOp != OP_NONE) && prm.preOp != OP_BLUESTEIN_PRE; // (the Bluestein form handles its chirp itself: not the interpreter's maps)
	const PassLaunchFn fn = !known ? nullptr : rad ? tab[idx].launchRad : ops ? tab[idx].launchOps : tab[idx].launch; // (nullptr where the instance has no such form)
	return launch_on_grid((uint64_t)prm.tilesPerG0 * (prm.colMerge ? 1u : prm.dim[1].count) * prm.dim[2].count, fn, prm, stream);
}

// ---- one-launch convolution on 7-smooth rows: eight table parts (kernels_mixconv_rows_*.hip) ------------------------
#define VKFFT_MIX_CONV_ROWS_PARTS(X, V, f) X(V, f, 0) X(V, f, 1) X(V, f, 2) X(V, f, 3) X(V, f, 4) X(V, f, 5) X(V, f, 6) X(V, f, 7)
VKFFT_REGISTRY_PARTS(MixConvRowVariant, mix_conv_rows, kMixConvRowsParts, VKFFT_MIX_CONV_ROWS_PARTS)
static const MixConvRowVariant* mix_conv_rows_part(int part, int* count) {
	return part < 0 ? nullptr : mix_conv_rows_part_fns[part % kMixConvRowsParts](count);
}
KernelShape mix_conv_row_lookup(uint64_t n, bool dp, bool real) {
	for (int part = 0; part < kMixConvRowsParts; part++) {
		int cnt = 0;
		const MixConvRowVariant* tab = mix_conv_rows_part(part, &cnt);
		for (int i = 0; i < cnt; i++) {
			if ((uint64_t)tab[i].n != n || tab[i].dp != dp || tab[i].real != real) continue;
			KernelShape k;
			k.variant = (part << 16) | i; k.perWg = tab[i].fpw; k.threads = tab[i].tpf * tab[i].fpw;
			for (int r = 0; r < 5; r++) k.sched[r] = tab[i].rad[r];
			return k;
		}
	}
	return {};
}
int launch_mix_conv_row(const PassPlan& pp, const PassParams& prm, hipStream_t stream) {
	int cnt = 0;
	const MixConvRowVariant* tab = mix_conv_rows_part((pp.variant >> 16) % kMixConvRowsParts, &cnt);
	const int idx = pp.variant & 0xffff;
	return launch_on_grid((uint64_t)prm.tilesPerG0, pp.variant >= 0 && idx < cnt ? tab[idx].launch : nullptr, prm, stream);
}

// ---- merged convolution along a strided 7-smooth last axis: four table parts (kernels_mixconv_cols_*.hip) -----------
#define VKFFT_MIX_CONV_COLS_PARTS(X, V, f) X(V, f, 0) X(V, f, 1) X(V, f, 2) X(V, f, 3)
VKFFT_REGISTRY_PARTS(MixConvColVariant, mix_conv_cols, kMixConvColsParts, VKFFT_MIX_CONV_COLS_PARTS)
static const MixConvColVariant* mix_conv_cols_part(int part, int* count) {
	return part < 0 ? nullptr : mix_conv_cols_part_fns[part % kMixConvColsParts](count);
}
KernelShape mix_conv_col_lookup(uint64_t n, bool dp) {
	for (int part = 0; part < kMixConvColsParts; part++) {
		int cnt = 0;
		const MixConvColVariant* tab = mix_conv_cols_part(part, &cnt);
		for (int i = 0; i < cnt; i++) {
			if ((uint64_t)tab[i].n != n || tab[i].dp != dp) continue;
			KernelShape k;
			k.variant = (part << 16) | i; k.perWg = tab[i].tc; k.threads = tab[i].tpf * tab[i].tc;
			for (int r = 0; r < 5; r++) k.sched[r] = tab[i].rad[r];
			return k;
		}
	}
	return {};
}
int launch_mix_conv_col(const PassPlan& pp, const PassParams& prm, hipStream_t stream) {
	int cnt = 0;
	const MixConvColVariant* tab = mix_conv_cols_part((pp.variant >> 16) % kMixConvColsParts, &cnt);
	const int idx = pp.variant & 0xffff;
	return launch_on_grid((uint64_t)prm.tilesPerG0 * prm.dim[1].count * prm.dim[2].count, pp.variant >= 0 && idx < cnt ? tab[idx].launch : nullptr, prm, stream);
}

// ---- ... and its bank form (numberKernels > 1): four table parts (kernels_mixconv_cols_bank_*.hip), the entries of the same record -----
#define VKFFT_MIX_CONV_COLS_BANK_PARTS(X, V, f) X(V, f, 0) X(V, f, 1) X(V, f, 2) X(V, f, 3)
VKFFT_REGISTRY_PARTS(MixConvColVariant, mix_conv_cols_bank, kMixConvColsBankParts, VKFFT_MIX_CONV_COLS_BANK_PARTS)
static const MixConvColVariant* mix_conv_cols_bank_part(int part, int* count) {
	return part < 0 ? nullptr : mix_conv_cols_bank_part_fns[part % kMixConvColsBankParts](count);
}
KernelShape mix_conv_col_bank_lookup(uint64_t n, bool dp) {
	for (int part = 0; part < kMixConvColsBankParts; part++) {
		int cnt = 0;
		const MixConvColVariant* tab = mix_conv_cols_bank_part(part, &cnt);
		for (int i = 0; i < cnt; i++) {
			if ((uint64_t)tab[i].n != n || tab[i].dp != dp) continue;
			KernelShape k;
			k.variant = (part << 16) | i; k.perWg = tab[i].tc; k.threads = tab[i].tpf * tab[i].tc;
			for (int r = 0; r < 5; r++) k.sched[r] = tab[i].rad[r];
			return k;
		}
	}
	return {};
}
int launch_mix_conv_col_bank(const PassPlan& pp, const PassParams& prm, hipStream_t stream) {
	int cnt = 0;
	const MixConvColVariant* tab = mix_conv_cols_bank_part((pp.variant >> 16) % kMixConvColsBankParts, &cnt);
	const int idx = pp.variant & 0xffff;
	return launch_on_grid((uint64_t)prm.tilesPerG0 * prm.dim[1].count * prm.dim[2].count, pp.variant >= 0 && idx < cnt ? tab[idx].launch : nullptr, prm, stream);
}

// ---- op-FFT registry: nine table parts, one translation unit each (kernels_opfft_*.hip) ---------------------------
#define VKFFT_OPFFT_PARTS(X, V, f) X(V, f, f32_row_0) X(V, f, f32_row_1) X(V, f, f32_col_0) X(V, f, f32_col_1) X(V, f, f64_row_0) X(V, f, f64_row_1) X(V, f, f64_col_0) X(V, f, f64_col_1) \
	X(V, f, f32_col_2) /* part 8: tools/gen_opfft_col_extra.py */
VKFFT_REGISTRY_PARTS(OpfftVariant, opfft, kOpfftParts, VKFFT_OPFFT_PARTS)
static const OpfftVariant* opfft_part(int part, int* count) { // part = 2 * ((dp ? 2 : 0) + (col ? 1 : 0)) + half
	return opfft_part_fns[part >= 0 && part < kOpfftParts ? part : 0](count);
}
#undef VKFFT_REGISTRY_PARTS
#undef VKFFT_PART_REF
#undef VKFFT_PART_DECL
#undef VKFFT_OPFFT_PARTS
#undef VKFFT_MIX_CONV_COLS_BANK_PARTS
#undef VKFFT_MIX_CONV_COLS_PARTS
#undef VKFFT_MIX_CONV_ROWS_PARTS
#undef VKFFT_MIXCONV_PARTS
#undef VKFFT_MIXED_PARTS
static uint32_t opfft_family(uint32_t op) { // DST members run on the DCT instance of their family
	switch (op) {
	case OP_DST2_PRE: return OP_DCT2_PRE; case OP_DST2_POST: return OP_DCT2_POST;
	case OP_DST3_PRE: return OP_DCT3_PRE; case OP_DST3_POST: return OP_DCT3_POST;
	case OP_DST4_PRE: return OP_DCT4_PRE; case OP_DST4_POST: return OP_DCT4_POST;
	case OP_DST2H_PRE: return OP_DCT2H_PRE; case OP_DST2H_POST: return OP_DCT2H_POST;
	case OP_DST3H_PRE: return OP_DCT3H_PRE; case OP_DST3H_POST: return OP_DCT3H_POST;
	default: return op;
	}
}
KernelShape opfft_lookup(uint64_t n, bool dp, bool col, bool trans, uint32_t pre, uint32_t post) {
	pre = opfft_family(pre); post = opfft_family(post);
	for (int half = 0; half < ((!dp && col) ? 3 : 2); half++) {
		const int part = half == 2 ? 8 : 2 * ((dp ? 2 : 0) + (col ? 1 : 0)) + half; // (fp32 column tiles have a third part)
		int cnt = 0;
		const OpfftVariant* tab = opfft_part(part, &cnt);
		for (int i = 0; i < cnt; i++) {
			if ((uint64_t)tab[i].n != n || (uint32_t)tab[i].pre != pre || (uint32_t)tab[i].post != post || tab[i].trans != trans) continue;
			KernelShape k;
			k.variant = (part << 16) | i; k.perWg = tab[i].fpw; k.threads = tab[i].tpf * tab[i].fpw;
			for (int r = 0; r < 5; r++) k.sched[r] = tab[i].rad[r];
			return k;
		}
	}
	return {};
}
int launch_opfft(const PassPlan& pp, const PassParams& prm, hipStream_t stream) {
	int cnt = 0;
	const OpfftVariant* tab = opfft_part(pp.variant >> 16, &cnt);
	const int idx = pp.variant & 0xffff;
	return launch_on_grid((uint64_t)prm.tilesPerG0 * (prm.colMerge ? 1u : prm.dim[1].count) * prm.dim[2].count, pp.variant >= 0 && idx < cnt ? tab[idx].launch : nullptr, prm, stream);
}

static int launch_with_hostloop(const PassPlan& pp, PassParams prm, const StreamSet& ss, uint32_t& rr, size_t level) {
	if (level == pp.hostLoop.size()) return launch_pass(pp, prm, ss.s[pp.hostLoop.empty() ? 0 : (rr++ % ss.n)]);
	const HostDim& h = pp.hostLoop[level];
	for (uint64_t i = 0; i < h.count; i++) {
		PassParams q = prm;
		q.in = (const char*)prm.in + (int64_t)i * h.inStride * pp.inElemBytes;
		q.out = (char*)prm.out + (int64_t)i * h.outStride * pp.outElemBytes;
		int r = launch_with_hostloop(pp, q, ss, rr, level + 1);
		if (r) return r;
	}
	return 0;
}

static void bind(const DirectionPlan& plan, const PassPlan& pp, const LaunchBuffers& bufs, PassParams& prm) {
	prm.in = (const char*)bufs.base[pp.inRole] + pp.inOffset * pp.inElemBytes;
	prm.out = (char*)bufs.base[pp.outRole] + pp.outOffset * pp.outElemBytes;
	const char* ar = (const char*)plan.dArena;
	prm.lut = pp.lutOff != (size_t)-1 ? ar + pp.lutOff : nullptr;
	prm.aux = pp.auxOff != (size_t)-1 ? ar + pp.auxOff : nullptr;
	prm.aux2 = pp.auxIsKernel ? bufs.kernel : pp.aux2Off != (size_t)-1 ? ar + pp.aux2Off : nullptr;
	prm.aux3 = pp.aux3Off != (size_t)-1 ? ar + pp.aux3Off : nullptr;
	prm.rader = pp.raderOff != (size_t)-1 ? ar + pp.raderOff : nullptr;
	prm.tmPre = pp.tmPreOff != (size_t)-1 ? ar + pp.tmPreOff : nullptr;
	prm.tmPost = pp.tmPostOff != (size_t)-1 ? ar + pp.tmPostOff : nullptr;
}

int execute_direction(const DirectionPlan& plan, const LaunchBuffers& bufs, const StreamSet& ss, uint32_t* sweep) {
	hipStream_t stream = ss.s[0];
	const int np = (int)plan.passes.size();
	for (int i = 0; i < np; i++) {
		const PassPlan& pp = plan.passes[i];
		if (pp.kernel == KERNEL_POW2_FUSED || pp.kernel == KERNEL_MIX_FUSED) {
			FusedParams f = pp.fused;
			const char* ar = (const char*)plan.dArena;
			f.in = (const char*)bufs.base[pp.inRole] + pp.inOffset * pp.inElemBytes;
			f.out = (char*)bufs.base[pp.outRole] + pp.outOffset * pp.outElemBytes;
			f.scratch = bufs.base[ROLE_TEMP];
			f.lutA = ar + pp.lutOff; f.lutB = ar + pp.fusedLutBOff; f.tw4 = ar + pp.auxOff;
			f.rowTab = pp.fusedRowTabOff != (size_t)-1 ? ar + pp.fusedRowTabOff : nullptr;
			f.ctr = (uint32_t*)((char*)plan.dArena + pp.fusedCtrOff);
			if (sweep) { f.reverse = *sweep & 1u; *sweep ^= 1u; }
			int r = pp.kernel == KERNEL_MIX_FUSED ? launch_mix_fused(pp, f, stream) : launch_pow2_fused(pp, f, stream);
			if (r) return r;
			continue;
		}
		PassParams prm = pp.prm;
		bind(plan, pp, bufs, prm);
		if (sweep) { prm.reverseTiles = *sweep & 1u; *sweep ^= 1u; } // zig-zag: opposite to the previous launch of this application
		const bool fan = ss.n > 1 && !pp.hostLoop.empty(); // independent sub-launches: fan out over the caller's streams, join into s[0]
		if (fan) {
			if (hipEventRecord(ss.ev[0], ss.s[0]) != hipSuccess) return 4040;
			for (uint32_t k = 1; k < ss.n; k++) if (hipStreamWaitEvent(ss.s[k], ss.ev[0], 0) != hipSuccess) return 4040;
		}
		uint32_t rr = 0;
		int r = launch_with_hostloop(pp, prm, ss, rr, 0);
		if (r) return r;
		if (fan) {
			for (uint32_t k = 1; k < ss.n; k++) {
				if (hipEventRecord(ss.ev[k], ss.s[k]) != hipSuccess) return 4040;
				if (hipStreamWaitEvent(ss.s[0], ss.ev[k], 0) != hipSuccess) return 4040;
			}
		}
	}
	return 0;
}

} // namespace vkfft_mi355x
