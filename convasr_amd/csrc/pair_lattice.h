// The alpha-beta sweep that star_ctc.hip and mwer.hip share: one workgroup per lattice, two halves of cap / 2 threads.  The lower half
// runs the alpha sweep forward in time, the upper half the beta sweep backward, both in the same loop over k = 1 .. Tb - 1 with ONE
// workgroup barrier per frame.  Nothing is polled: every loop is bounded by Tb <= T or by the state count, so no input can make a launch
// spin.  A thread owns the (blank, unit) pair j of its sweep -- states 2j and 2j+1 -- in registers; the column of the previous frame lives
// in LDS as one 16-byte entry per pair {blank, unit, the pair's offset, -} (double-buffered, PL_PAD / 2 sentinel pairs on either side, so
// the neighbour pairs need no bounds test).  An arc that does not exist is an additive cost of the sentinel: the recursion is branch-free.
// STAR = false is the plain three-arc CTC recursion (s, s - 1, and s - 2 when the units differ); STAR = true adds the arcs around a star
// unit that is skipped (s - 3, s - 4) and the cost c1 of entering one.
// Arithmetic as log2_domain.h documents it, every new value floored at the sentinel, and every PL_RENORM frames a PAIR of states loses
// floor(its maximum) -- an integer in the log2 domain, so the subtraction, the running sum of the offsets and the conversion of a
// neighbour pair's values (true value = stored value + the pair's offset) are exact.  One offset per pair and block of frames, where
// ctc.hip keeps one per wave: a star is cheap, so the column's maximum sits at the states that have consumed the fewest labels, ~3 bits
// per frame above the states the posterior lives on -- with one offset per column (measured: 1,023 states, T = 355) those were ~1,100 in
// magnitude and the gradient missed its bar 4.8-fold; per pair every stored value is O(10) wherever it matters.
// LP_LDS: the (Tb, C) log-prob slab is staged into LDS when it fits beside the columns (753 x 38: 112 KiB).
#pragma once
#include "log2_domain.h"

#define PL_RENORM 2             // (per pair, no exchange between lanes: the only cost of a short block is its entry in the offsets)
#define PL_RENORM_LOG2 1
#define PL_WAVE_STATES 128       // states of one wave of a sweep (two per lane)
#define PL_MAX_STATES 1024
#define PL_MAX_T 8192
#define PL_MAX_C 8192
template <bool STAR> constexpr int PL_PAD = STAR ? 4 : 2;   // sentinel pairs of a column buffer: half of them below pair 0, half above the last

__device__ __forceinline__ float pl_exp2(float v) { return __builtin_amdgcn_exp2f(v); }
// base-2 log-sum-exp with every term through v_exp_f32; the order of the additions is part of the results' bit pattern
__device__ __forceinline__ float lse2(float a, float b) {
	const float m = fmaxf(a, b);
	return m + __builtin_amdgcn_logf(pl_exp2(a - m) + pl_exp2(b - m));
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
	const float m = fmaxf(a, fmaxf(b, c));
	return m + __builtin_amdgcn_logf(pl_exp2(a - m) + pl_exp2(b - m) + pl_exp2(c - m));
}
__device__ __forceinline__ float lse4(float a, float b, float c, float d) {
	const float m = fmaxf(fmaxf(a, b), fmaxf(c, d));
	return m + __builtin_amdgcn_logf((pl_exp2(a - m) + pl_exp2(b - m)) + (pl_exp2(c - m) + pl_exp2(d - m)));
}
__device__ __forceinline__ float lse5(float a, float b, float c, float d, float e) {
	const float m = fmaxf(fmaxf(fmaxf(a, b), fmaxf(c, d)), e);
	return m + __builtin_amdgcn_logf((pl_exp2(a - m) + pl_exp2(b - m)) + (pl_exp2(c - m) + pl_exp2(d - m)) + pl_exp2(e - m));
}

typedef float pl_f2 __attribute__((ext_vector_type(2)));

// Fills the four column buffers at `col` with the sentinel and, LP_LDS, stages the cnt = Tb C log-probs; the caller's barrier follows.
template <bool STAR, bool LP_LDS>
__device__ __forceinline__ void pair_lattice_stage(float4* col, int half, float* lpl, const float* lpg, int cnt) {
	const int tid = threadIdx.x, nthr = blockDim.x;
	for (int i = tid; i < 4 * (half + PL_PAD<STAR>); i += nthr) col[i] = make_float4(LOG2_NEG, LOG2_NEG, 0.f, 0.f);
	if (LP_LDS)
		for (int i = tid; i < cnt; i += nthr) lpl[i] = log2_floor(lpg[i] * LOG2_E);
}

struct PairLattice {
	// the lattice (uniform over the workgroup)
	const float* lpb;       // its log-probs [Tb][C]: the staged LDS copy (LP_LDS) or the raw global slab
	float4* col;            // LDS columns [2 sweeps][2 buffers][half + PL_PAD]
	float *alpha, *beta;    // its lattices [T][ls] in the workspace
	float *offa, *offb;     // the two sweeps' offsets [NB][lh]
	float *nll, *tot;       // its loss and tot[4] = {integer part, remainder of the log2 likelihood, states, -}
	int Tb, C, blank, half, ls, lh;
	int n;                  // units: 2 n + 1 states
	bool last_star;         // the last unit is a star: the lattice may also end before it
	// this thread's pair j of its sweep
	bool fwd, st;           // st: the pair lies inside the workspace's row and is stored
	int j, cidx;            // cidx: the unit's class, -1 for a star, a label outside [0, C) or no unit
	bool prev_star;         // unit j - 1 is a star: pair 1 of the alpha sweep also starts
	float oconst;           // what a unit without a class emits: a star's penalty, else the sentinel
	float c1, c2, c3, c4;   // arc costs: blank -> unit inside the pair, and the arcs from (alpha) or to (beta) the neighbour pairs
};

template <bool STAR, bool LP_LDS>
__device__ __forceinline__ void pair_lattice_sweep(const PairLattice& p) {
	const int colw = p.half + PL_PAD<STAR>, j = p.j, e = 2 * j, n = p.n, Tb = p.Tb, C = p.C, cidx = p.cidx, ls = p.ls, lh = p.lh;
	const bool fwd = p.fwd, st = p.st, has_e = j <= n;
	const float c1 = p.c1, c2 = p.c2, c3 = p.c3, c4 = p.c4;
	auto emis = [&](int t, float& ve, float& vo) {
		const float* row = p.lpb + (int64_t)t * C;
		float xe = row[p.blank], xo = row[cidx >= 0 ? cidx : p.blank];
		if (!LP_LDS) { xe = log2_floor(xe * LOG2_E); xo = log2_floor(xo * LOG2_E); }
		ve = has_e ? xe : LOG2_NEG;
		vo = cidx >= 0 ? xo : p.oconst;
	};
	float4* const mycol = p.col + (fwd ? 0 : 2) * colw + PL_PAD<STAR> / 2;   // buffer q: mycol + q * colw, pair j at [j]
	float* const lat = fwd ? p.alpha : p.beta;
	float* const off = (fwd ? p.offa : p.offb) + j;   // block q of frames: off[q * lh]
	const int t0 = fwd ? 0 : Tb - 1, dt = fwd ? 1 : -1;
	float ae, ao, ce = LOG2_NEG, co = LOG2_NEG, cum = 0.f;
	{
		float ee, eo;
		emis(t0, ee, eo);
		if (fwd) {
			ae = j == 0 ? ee : LOG2_NEG;
			if constexpr (STAR) ao = j == 0 ? eo + c1 : ((j == 1 && p.prev_star) ? eo : LOG2_NEG);
			else ao = j == 0 ? eo : LOG2_NEG;
		} else {
			ae = (j == n || (p.last_star && j == n - 1)) ? ee : LOG2_NEG;
			ao = (j == n - 1 || (p.last_star && j == n - 2)) ? eo : LOG2_NEG;
		}
		ae = log2_floor(ae); ao = log2_floor(ao);
		mycol[j] = make_float4(ae, ao, 0.f, 0.f);
		if (st) {
			*reinterpret_cast<pl_f2*>(lat + (int64_t)t0 * ls + e) = pl_f2{ae, ao};
			off[0] = 0.f;
		}
		if (Tb > 1) emis(t0 + dt, ce, co);
	}
	__syncthreads();
	for (int k = 1; k < Tb; ++k) {   // the k-th frame of the sweep
		const int t = t0 + k * dt;
		const float4* prev = mycol + ((k - 1) & 1) * colw;
		float4* cur = mycol + (k & 1) * colw;
		float nxe = LOG2_NEG, nxo = LOG2_NEG;
		if (k + 1 < Tb) emis(t + dt, nxe, nxo);
		float ne, no, nbz;   // nbz: the offset of the neighbour pair the sweep comes from
		if (fwd) {
			const float4 p1 = prev[j - 1];   // the neighbour pairs' values, converted to this pair's offset (exact)
			const float d1 = p1.z - cum, x2 = p1.y + d1;
			ne = lse2(ae, x2) + ce;
			if constexpr (STAR) {
				const float4 p2 = prev[j - 2];
				const float x3 = p1.x + d1, x4 = p2.y + (p2.z - cum);
				no = lse5(ao, ae + c1, x2 + c2, x3 + c3, x4 + c4) + co;
			} else no = lse3(ao, ae, x2 + c2) + co;
			nbz = p1.z;
		} else {
			const float4 n1 = prev[j + 1];
			const float d1 = n1.z - cum, y2 = n1.x + d1, y3 = n1.y + d1;
			if constexpr (STAR) {
				const float4 n2 = prev[j + 2];
				const float y5 = n2.y + (n2.z - cum);
				ne = lse3(ae, ao + c1, y3 + c3) + ce;
				no = lse4(ao, y2, y3 + c2, y5 + c4) + co;
			} else {
				ne = lse2(ae, ao) + ce;
				no = lse3(ao, y2, y3 + c2) + co;
			}
			nbz = n1.z;
		}
		ne = log2_floor(ne); no = log2_floor(no);
		// A pair no path has reached yet (both values the sentinel, which absorbs any offset) follows its neighbour's offset frame by frame,
		// so that the first values to arrive are O(10) against it: left at 0 they would be ~5 t in magnitude until the block ends, and in a
		// tight lattice (T close to the frames the labels need) every path runs through such freshly reached states.  A live pair changes
		// its offset at the first frame of a block only; the block's entry is rewritten every frame, and the last write is the offset of
		// every live value of the block.
		const float m = fmaxf(ne, no);
		if (!(m > LOG2_DEAD)) cum = nbz;
		else if ((k & (PL_RENORM - 1)) == 0 && m < INFINITY) {
			const float kk = floorf(m);
			ne -= kk; no -= kk;
			cum += kk;
		}
		ae = ne; ao = no;
		cur[j] = make_float4(ae, ao, cum, 0.f);
		if (st) {
			off[(int64_t)(k >> PL_RENORM_LOG2) * lh] = cum;
			*reinterpret_cast<pl_f2*>(lat + (int64_t)t * ls + e) = pl_f2{ae, ao};
		}
		ce = nxe; co = nxo;
		__syncthreads();
	}
	if (threadIdx.x == 0) {   // (mycol: the alpha sweep's)
		// the end states 2n (pair n), 2n - 1 (pair n - 1) and, behind a last star, 2n - 2 (pair n - 1) and 2n - 3 (pair n - 2), each at its
		// pair's offset; the pairs below pair 0 hold the sentinel.  The total is split into the offset of the largest and a remainder.
		constexpr int NE = STAR ? 4 : 2;
		const float4* fin = mycol + ((Tb - 1) & 1) * colw;
		const float4 pn = fin[n], pm1 = fin[n - 1], pm2 = STAR ? fin[n - 2] : pm1;
		const float v[4] = {pn.x, pm1.y, p.last_star ? pm1.x : LOG2_NEG, p.last_star ? pm2.y : LOG2_NEG}, c[4] = {pn.z, pm1.z, pm1.z, pm2.z};
		int best = 0;
		for (int i = 1; i < NE; ++i) if (v[i] > LOG2_DEAD && (!(v[best] > LOG2_DEAD) || v[i] + c[i] > v[best] + c[best])) best = i;
		const float cbest = c[best];
		float m = LOG2_NEG, l[4];
		for (int i = 0; i < NE; ++i) { l[i] = v[i] + (c[i] - cbest); m = fmaxf(m, l[i]); }
		float sum = exp2f(l[0] - m) + exp2f(l[1] - m);
		if constexpr (STAR) sum += exp2f(l[2] - m) + exp2f(l[3] - m);
		const float rem = m + log2f(sum);
		*p.nll = rem != rem ? NAN : (m > LOG2_DEAD ? (float)(-LOG2_LN2 * ((double)cbest + (double)rem)) : INFINITY);
		p.tot[0] = cbest;
		p.tot[1] = rem;
		p.tot[2] = (float)(2 * n + 1);
	}
}

// the exponent's shift of a state's posterior exp2(alpha + beta + (shift - emission)): alpha + beta - total = (lattice values - remainder
// of total) + (the pair's offsets oa, ob - integer part ti of total), and the second group is exact
__device__ __forceinline__ float pl_posterior_shift(float oa, float ob, float ti, float tr) { return ((oa - ti) + ob) - tr; }

// states of a lattice row rounded up to whole waves = the workgroup's threads; -1 outside 1 .. PL_MAX_STATES - 1
static int pl_cap(int64_t states) {
	if (states < 1 || states >= PL_MAX_STATES) return -1;
	return ((int)states + PL_WAVE_STATES - 1) / PL_WAVE_STATES * PL_WAVE_STATES;
}

// Launches K_LDS when the (T, C) log-prob slab fits LDS beside the kernel's lds_fixed bytes, else K_GLOBAL, with the slab's bytes added.
template <auto K_LDS, auto K_GLOBAL, typename... Args>
static void pl_launch(int grid, int cap, size_t lds_fixed, int T, int C, hipStream_t s, Args... args) {
	static unsigned long long set[2] = {};
	const size_t lds_lp = (size_t)T * C * 4;
	const bool in_lds = lds_fixed + lds_lp <= 159 * 1024;
	const auto kern = in_lds ? K_LDS : K_GLOBAL;
	convasr_allow_160k_lds(reinterpret_cast<const void*>(kern), set[in_lds]);
	hipLaunchKernelGGL(kern, dim3(grid), dim3(cap), lds_fixed + (in_lds ? lds_lp : 0), s, args...);
}
