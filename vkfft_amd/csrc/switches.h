// Every environment switch of the library, declared once.  read_switches() below is the only place that reads the environment: initializeVkFFT takes one
// snapshot per call, the snapshot travels in TransformDesc, and what a launch needs of it is stored in the plan — a plan never changes with the environment
// after it is built.  INTEGRATION.md's switch table documents the same names (tests/test_abi.py::test_environment_switches_are_documented keeps the two in step).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>

namespace vkfft_mi355x {

// X(name, field, type, parse, default, description).  parse, applied only when the variable is set (the field keeps its default otherwise):
//   FLAG  set at all, whatever the value (`NAME=0` still means set)     INT  (type)atoi     LONG  (type)atoll     KIB  (type)atoll << 10     REAL  atof
// XI(name, field, description): an indexed family NAME<k>, k = log2 of the length, INT, default 0: the k-th registered shape of that length (0 = what ships).
// Defaults are in the field's own unit (bytes for KIB).
#define VKFFT_SWITCHES(X, XI) \
	X(VKFFT_MI355X_PRINT_PLAN,           printPlan,        bool,     FLAG, false,      "one line per pass on stderr; fallbacks of zero-padded axes; disableReorderFourStep notice") \
	X(VKFFT_MI355X_GENERIC_ONLY,         genericOnly,      bool,     INT,  false,      "every pass on the interpreter kernel (coverage baseline)") \
	X(VKFFT_MI355X_CONV_SEPARATE,        convSeparate,     bool,     FLAG, false,      "convolution plans as separate forward / product / inverse passes") \
	X(VKFFT_MI355X_NO_REVERSE,           noReverse,        bool,     FLAG, false,      "every launch sweeps front to back (no zig-zag reuse of the Infinity Cache)") \
	X(VKFFT_MI355X_FORCE_BIGSPAN,        forceBigSpan,     bool,     FLAG, false,      "tests: the 64-bit form of the column kernel on small problems") \
	/* fused Four-Step (kernel_pow2_fused.h, kernel_mix_fused.h); the numeric ones are tuning knobs, 0 = planner default */ \
	X(VKFFT_MI355X_FUSED,                fused,            bool,     INT,  true,       "0: separate passes") \
	X(VKFFT_MI355X_FUSED_MODE,           fusedMode,        int,      INT,  2,          "kernel mode (2 = what ships; 6 = the same with per-phase cycle sums, development build)") \
	X(VKFFT_MI355X_FUSED_CHUNK_KIB,      fusedChunkBytes,  uint64_t, KIB,  0,          "chunk size") \
	X(VKFFT_MI355X_FUSED_LAG,            fusedLag,         uint32_t, INT,  0,          "lag of the ring (chunks)") \
	X(VKFFT_MI355X_FUSED_RING,           fusedRing,        uint32_t, INT,  0,          "ring slots") \
	X(VKFFT_MI355X_FUSED_WGS,            fusedWgPerCu,     uint32_t, INT,  0,          "workgroups per CU (0: what the occupancy query reports)") \
	X(VKFFT_MI355X_FUSED_QUEUES,         fusedQueues,      uint32_t, INT,  0,          "work queues") \
	X(VKFFT_MI355X_FUSED_MARGIN,         fusedMarginPct,   uint32_t, INT,  0,          "ring margin in per cent") \
	X(VKFFT_MI355X_FUSED_PROFILE,        fusedProfile,     bool,     FLAG, false,      "development build: per-phase cycle sums of every launch (blocking)") \
	X(VKFFT_MI355X_MIXFUSED,             mixFused,         int,      INT,  1,          "0: non-power-of-two two-factor lengths as separate passes") \
	X(VKFFT_MI355X_MIXFUSED_BLUE,        mixFusedBlue,     int,      INT,  0,          "non-zero: long chirp-z rows as two launches of that kernel (correct, measured slower: off)") \
	X(VKFFT_MI355X_MXFV,                 mixFusedShape,    int,      INT,  0,          "k-th registered shape of a non-power-of-two fused length (one value for every length)") \
	X(VKFFT_MI355X_ROW15,                row15,            int,      INT,  1,          "0: 2^15 fp32 as the fused two-pass plan instead of one pass") \
	X(VKFFT_MI355X_LONGROWS,             longRows,         int,      INT,  1,          "0: 11^4, 5^6, 7^5 as fused Four-Step launches instead of one pass of the long mixed-radix rows") \
	/* one-kernel Rader / smooth Bluestein family (kernel_mixconv.h) and the Rader-stage kernel (kernel_mixrad.h) */ \
	X(VKFFT_MI355X_MIXCONV,              mixconv,          int,      INT,  1,          "0: family off; 2: always preferred") \
	X(VKFFT_MI355X_MIXCONV_COST_RADER,   mixconvCostRader, double,   REAL, 1.9,        "time per point of its Rader form relative to the power-of-two kernels") \
	X(VKFFT_MI355X_MIXCONV_COST_BLUE,    mixconvCostBlue,  double,   REAL, 1.6,        "... of its Bluestein form") \
	X(VKFFT_MI355X_MIXRAD,               mixrad,           int,      INT,  1,          "0: Rader-stage kernel off; 2: always where it serves the length") \
	X(VKFFT_MI355X_MIXRAD_PRIMES,        mixradPrimes,     int,      INT,  0,          "1 (exactly): a prime's own rows on it too (measured slower than kernel_mixconv.h)") \
	X(VKFFT_MI355X_MIXRAD_COST,          mixradCost,       double,   REAL, kSwitchUnset, "cost per point against the fused Bluestein kernel; unset (or a value that parses as NaN): the planner's model (mixrad_choose)") \
	X(VKFFT_MI355X_MIXRAD_LDS_KIB,       mixradLdsBytes,   uint64_t, KIB,  40ull << 10, "LDS budget of a tile") \
	X(VKFFT_MI355X_MIXRAD_DENSE,         mixradDense,      bool,     FLAG, false,      "thread groups always in the dense layout") \
	/* real rows */ \
	X(VKFFT_MI355X_NO_MIXED_OPS,         noMixedOps,       bool,     FLAG, false,      "never an instance transform between the interpreter's maps") \
	X(VKFFT_MI355X_MIXED_OPS_MAX,        mixedOpsMax,      uint64_t, LONG, 16,         "longest complex length that prefers that form over its fused-map kernel") \
	X(VKFFT_MI355X_NO_ROW_PAIRS,         noRowPairs,       bool,     FLAG, false,      "one real row per complex transform") \
	X(VKFFT_MI355X_NO_BLUE_PAIRS,        noBluePairs,      bool,     FLAG, false,      "... inside the fused Bluestein kernel only") \
	X(VKFFT_MI355X_PAIR_PREFER,          pairPrefer,       int,      INT,  2,          "pairs over a fused-map instance: 0 never, 1 every pairable family, 2 DCT-II / -III and odd DCT-IV (pairable_family)") \
	X(VKFFT_MI355X_EVEN_FULL,            evenFull,         int,      INT,  1,          "even lengths: 0 half-length forms, 1 full-length pairs where they win, 2 also over a fused-map kernel") \
	X(VKFFT_MI355X_NO_TMAPS,             noTmaps,          bool,     FLAG, false,      "the generic maps instead of the table-driven ones (kernel_tmaps.h)") \
	X(VKFFT_MI355X_TMAPS_MIN_TPF,        tmapsMinTpf,      int,      INT,  1,          "threads per row from which the tables replace the generic maps (they win at every shape measured: A/B runs)") \
	X(VKFFT_MI355X_NO_REAL_BLUE_CHOICE,  noRealBlueChoice, bool,     FLAG, false,      "real rows whose complex length has a factor 47, 59 ... back on the interpreter") \
	/* registered shapes of the power-of-two kernels */ \
	XI(VKFFT_MI355X_P2V,                 pow2RowShape,     "row kernel of 2^k (kernels_pow2.hip)") \
	XI(VKFFT_MI355X_P2C,                 pow2ColShape,     "column kernel of 2^k") \
	XI(VKFFT_MI355X_P2B,                 pow2BlueShape,    "fused Bluestein kernel on 2^k padded points") \
	XI(VKFFT_MI355X_FUV,                 pow2FusedShape,   "fused Four-Step kernel of 2^k (kernels_fused.hip)")

constexpr double kSwitchUnset = std::numeric_limits<double>::quiet_NaN(); // a REAL switch that distinguishes "unset" from every value: test with x != x
constexpr uint32_t kSwitchIndexed = 32; // k of an indexed family: 0 ... 31

struct Switches {
#define VKFFT_SW_FIELD(name, field, type, parse, def, doc) type field = def;
#define VKFFT_SW_FIELDS(name, field, doc) int field[kSwitchIndexed] = {};
	VKFFT_SWITCHES(VKFFT_SW_FIELD, VKFFT_SW_FIELDS)
#undef VKFFT_SW_FIELD
#undef VKFFT_SW_FIELDS
	static int shape(const int (&family)[kSwitchIndexed], uint32_t k) { return k < kSwitchIndexed ? family[k] : 0; }
};

inline Switches read_switches() {
	Switches s;
#define VKFFT_SW_FLAG(type, e) true
#define VKFFT_SW_INT(type, e) (type)atoi(e)
#define VKFFT_SW_LONG(type, e) (type)atoll(e)
#define VKFFT_SW_KIB(type, e) (type)atoll(e) << 10
#define VKFFT_SW_REAL(type, e) atof(e)
#define VKFFT_SW_READ(name, field, type, parse, def, doc) if (const char* e = getenv(#name)) s.field = VKFFT_SW_##parse(type, e);
#define VKFFT_SW_READS(name, field, doc) \
	for (uint32_t k = 0; k < kSwitchIndexed; k++) { char n[48]; snprintf(n, sizeof(n), #name "%u", k); if (const char* e = getenv(n)) s.field[k] = atoi(e); }
	VKFFT_SWITCHES(VKFFT_SW_READ, VKFFT_SW_READS)
#undef VKFFT_SW_FLAG
#undef VKFFT_SW_INT
#undef VKFFT_SW_LONG
#undef VKFFT_SW_KIB
#undef VKFFT_SW_REAL
#undef VKFFT_SW_READ
#undef VKFFT_SW_READS
	return s;
}

} // namespace vkfft_mi355x
