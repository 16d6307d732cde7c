// Log-likelihood arithmetic in base 2, shared by the CTC lattices (ctc.hip, ctc_long.hip, pair_lattice.h): v_exp_f32 and v_log_f32 are
// base-2 instructions, so log-probs are scaled by log2(e) once and the lattices hold log2 values.  "Impossible" is the finite sentinel
// LOG2_NEG, not -inf: max + log2(sum of exp2) then needs no guard against inf - inf, the sentinel absorbs every finite score added to
// it and exp2(sentinel - anything real) is 0.
#pragma once

#define LOG2_NEG (-1e30f)
#define LOG2_DEAD (-1e29f)        // anything below is "impossible"
#define LOG2_E 1.4426950408889634f
#define LOG2_LN2 0.6931471805599453

// -inf (and anything below the sentinel) becomes the sentinel; a NaN stays a NaN (fmaxf would drop it)
__device__ __forceinline__ float log2_floor(float v) { return v < LOG2_NEG ? LOG2_NEG : v; }

// Base-2 log-sum-exp of three values >= the sentinel, in the max / med3 / min form: the largest term is exp2(0) = 1 exactly, so only the
// other two go through v_exp_f32 (max3 / med3 / min3 are single instructions).  The two-term forms stay with their files: they compile
// differently and differ in the sum's order (pair_lattice.h's lse2 .. lse5 take exp2 of every term).
__device__ __forceinline__ float lse3_med3(float a, float b, float c) {
	const float m = fmaxf(a, fmaxf(b, c));
	const float md = __builtin_amdgcn_fmed3f(a, b, c), lo = fminf(a, fminf(b, c));
	return m + __builtin_amdgcn_logf(1.f + __builtin_amdgcn_exp2f(md - m) + __builtin_amdgcn_exp2f(lo - m));
}
