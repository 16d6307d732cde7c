// Star-token CTC loss and gradient (this project's own rule, include/convasr_hip.h: convasr_star_ctc_loss; the W-CTC / Star Temporal
// Classification family): the transcript may miss words, so an optional STAR unit -- "any stretch of frames, or nothing" -- stands in
// every allowed gap between the labels.  The lattice has up to five arcs into a state (s, s-1, s-2 and, around a star that is skipped,
// s-3, s-4), which csrc/ctc.hip's two-neighbour recursion cannot express.
//
// Kernel 1 -- one workgroup per utterance, two halves of cap / 2 threads: the lower half runs the alpha sweep forward in time, the upper
// half the beta sweep backward, both in the same loop over k = 1 .. olen - 1 with ONE workgroup barrier per frame.  Nothing is polled:
// every loop is bounded by olen <= T or by the state count, so no input can make a launch spin.  A thread owns the (blank, unit) pair j
// of its sweep -- states 2j and 2j+1 -- in registers; the column of the previous frame lives in LDS as one 16-byte entry per pair
// {blank, unit, the pair's offset, -} (double-buffered, two sentinel pairs on either side, so the neighbour pairs j-1, j-2 / j+1, j+2
// need no bounds test).
// An arc that does not exist is an additive cost of the sentinel, an arc into a star costs star_enter: the recursion is branch-free.
// The per-unit descriptor (class, star or nothing; the gap of a star) is built in LDS from targets, ylen and star_mask by a prefix count
// over the mask, and its per-state form goes to the workspace for kernel 2.
// Arithmetic as csrc/ctc.hip documents it: fp32 log-sum-exp in base 2, "impossible" = the finite sentinel -1e30 (a -inf log-prob is staged
// as the sentinel, every new value is floored at it), and every SC_RENORM frames a PAIR of states loses floor(its maximum) -- an integer
// in the log2 domain, so the subtraction, the running sum of the offsets and the conversion of a neighbour pair's values (true value =
// stored value + the pair's offset) are exact.  One offset per pair and block of frames, where ctc.hip keeps one per wave: a star is
// cheap, so the column's maximum sits at the states that have consumed the fewest labels, ~3 bits per frame above the states the
// posterior lives on -- with one offset per column (measured: 1,023 states, T = 355) those were ~1,100 in magnitude and the gradient
// missed its bar 4.8-fold; per pair every stored value is O(10) wherever it matters.
// LP_LDS: the utterance's (olen, C) log-prob slab is staged into LDS when it fits beside the columns (753 x 38: 112 KiB).
// Kernel 2 -- one wave per frame: posterior of every state = exp2(alpha + beta - total - emission); label and blank states go to LDS bins
// per class, their sum is occ, star states go to LDS bins per gap (added to star_frames once per workgroup: fp32 atomics on global
// memory, so star_frames is reproducible to rounding only; nll and grad are bit-reproducible).  grad = occ * exp(lp) - posterior.
#include "common.h"

#define SC_NEG (-1e30f)
#define SC_DEAD (-1e29f)         // anything below is "impossible"
#define SC_LOG2E 1.4426950408889634f
#define SC_LN2 0.6931471805599453
#define SC_RENORM 2             // (per pair, no exchange between lanes: the only cost of a short block is its entry in the offsets)
#define SC_RENORM_LOG2 1
#define SC_WAVE_STATES 128       // states of one wave of a sweep (two per lane)
#define SC_MAX_STATES 1024
#define SC_PAD 4
#define SC_MAX_T 8192
#define SC_MAX_C 8192
enum { SC_STAR = -1, SC_BAD = -2, SC_NONE = -3 };  // unit kinds below the classes: a star, a label outside [0, C) (never matches), no unit

// -inf (and anything below the sentinel) becomes the sentinel; a NaN stays a NaN
__device__ __forceinline__ float sc_floor(float v) { return v < SC_NEG ? SC_NEG : v; }
__device__ __forceinline__ float sc_exp2(float v) { return __builtin_amdgcn_exp2f(v); }
__device__ __forceinline__ float sc_lse2(float a, float b) {
	const float m = fmaxf(a, b);
	return m + __builtin_amdgcn_logf(sc_exp2(a - m) + sc_exp2(b - m));
}
__device__ __forceinline__ float sc_lse3(float a, float b, float c) {
	const float m = fmaxf(a, fmaxf(b, c));
	return m + __builtin_amdgcn_logf(sc_exp2(a - m) + sc_exp2(b - m) + sc_exp2(c - m));
}
__device__ __forceinline__ float sc_lse4(float a, float b, float c, float d) {
	const float m = fmaxf(fmaxf(a, b), fmaxf(c, d));
	return m + __builtin_amdgcn_logf((sc_exp2(a - m) + sc_exp2(b - m)) + (sc_exp2(c - m) + sc_exp2(d - m)));
}
__device__ __forceinline__ float sc_lse5(float a, float b, float c, float d, float e) {
	const float m = fmaxf(fmaxf(fmaxf(a, b), fmaxf(c, d)), e);
	return m + __builtin_amdgcn_logf((sc_exp2(a - m) + sc_exp2(b - m)) + (sc_exp2(c - m) + sc_exp2(d - m)) + sc_exp2(e - m));
}

typedef float sc_f2 __attribute__((ext_vector_type(2)));

// 32-bit words of LDS ahead of the log-prob slab: columns [2 sweeps][2 buffers][cap / 2 + SC_PAD pairs][4] | unit kinds
// [cap / 2 + 4] | unit gaps [cap / 2] | mask [S_max + 2] | unit count [4], rounded up to 16 bytes
__host__ __device__ static inline int sc_lds_words(int cap, int S_max) {
	return (16 * (cap / 2 + SC_PAD) + (cap / 2 + 4) + cap / 2 + (S_max + 2) + 4 + 3) & ~3;
}

// Workspace: alpha, beta [B][T][cap] fp32 | offs [2][B][NB][cap / 2] | tot [B][4] = {integer part, remainder of the log2 likelihood, states, -} |
// desc [B][cap] int32: the class of a label or blank state, -(gap + 2) for a star, -1 for a label outside [0, C)
template <bool LP_LDS>
__global__ __launch_bounds__(1024) void star_ctc_alpha_beta_kernel(const float* __restrict__ lp, const int64_t* __restrict__ targets, const int64_t* __restrict__ olen,
                                                                   const int64_t* __restrict__ ylen, const uint8_t* __restrict__ star_mask, float* __restrict__ nll,
                                                                   float* __restrict__ alpha, float* __restrict__ beta, float* __restrict__ offs, float* __restrict__ tot,
                                                                   int* __restrict__ desc, float* __restrict__ star_frames,
                                                                   int B, int T, int C, int S_max, int blank, int cap, float pen2, float ent2) {
	extern __shared__ __attribute__((aligned(16))) float sc_smem[];
	const int half = cap >> 1, tid = threadIdx.x, nthr = blockDim.x, b = blockIdx.x;
	const int colw = half + SC_PAD;   // pairs per column buffer: two sentinel pairs below pair 0, two above the last
	float4* const col = reinterpret_cast<float4*>(sc_smem);
	int* const ucls = reinterpret_cast<int*>(sc_smem + 16 * colw);   // unit i at ucls[2 + i]
	int* const ugap = ucls + half + 4;
	int* const msk = ugap + half;
	int* const nsh = msk + S_max + 2;
	float* const lpl = sc_smem + sc_lds_words(cap, S_max);
	const int NB = T / SC_RENORM + 1;
	const int64_t Tb64 = olen[b], S64 = ylen[b];
	for (int g = tid; g <= S_max; g += nthr) star_frames[(int64_t)b * (S_max + 1) + g] = 0.f;
	if (Tb64 <= 0 || Tb64 > T || S64 < 0 || S64 > S_max) {  // uniform over the workgroup
		if (tid == 0) nll[b] = (Tb64 == 0 && S64 == 0) ? 0.f : INFINITY;
		return;
	}
	const int Tb = (int)Tb64, S = (int)S64;
	const float* lpg = lp + (int64_t)b * T * C;
	const int64_t* tg = targets + (int64_t)b * S_max;

	// ---- the units: a star in every allowed gap g <= S, ahead of label g
	for (int i = tid; i < half + 4; i += nthr) ucls[i] = SC_NONE;
	for (int g = tid; g <= S; g += nthr) msk[g] = star_mask[(int64_t)b * (S_max + 1) + g] ? 1 : 0;
	for (int i = tid; i < 4 * colw; i += nthr) col[i] = make_float4(SC_NEG, SC_NEG, 0.f, 0.f);
	if (LP_LDS) {
		const int cnt = Tb * C;
		for (int i = tid; i < cnt; i += nthr) lpl[i] = sc_floor(lpg[i] * SC_LOG2E);
	}
	__syncthreads();
	for (int g = tid; g <= S; g += nthr) {
		int pre = 0;
		for (int h = 0; h < g; ++h) pre += msk[h];
		const int m = msk[g], u = g + pre;   // u + m <= 2 S + 1 < half
		if (m) { ucls[2 + u] = SC_STAR; ugap[u] = g; }
		if (g < S) {
			const int64_t y = tg[g];
			ucls[2 + u + m] = (y >= 0 && y < C) ? (int)y : SC_BAD;
			ugap[u + m] = -1;
		} else nsh[0] = u + m;
	}
	__syncthreads();
	const int n = nsh[0], L = 2 * n + 1;
	for (int s = tid; s < L; s += nthr) {
		int d = blank;
		if (s & 1) {
			const int u = ucls[2 + (s >> 1)];
			d = u >= 0 ? u : (u == SC_STAR ? -(ugap[s >> 1] + 2) : -1);
		}
		desc[(int64_t)b * cap + s] = d;
	}

	// ---- this thread's pair of states and the arcs around it
	const bool fwd = tid < half;
	const int j = fwd ? tid : tid - half, e = 2 * j, o = e + 1;
	const int u0 = ucls[2 + j], um1 = ucls[1 + j], um2 = ucls[j], up1 = ucls[3 + j], up2 = ucls[4 + j];
	const bool has_e = j <= n, has_o = j < n, star0 = u0 == SC_STAR;
	const bool last_star = n >= 1 && ucls[2 + n - 1] == SC_STAR;
	const int cidx = u0 >= 0 ? u0 : -1;
	const float oconst = star0 ? pen2 : SC_NEG;
	const float c1 = star0 ? ent2 : 0.f;   // e -> o: into a star
	float c2, c3, c4;
	if (fwd) {
		c2 = (has_o && j >= 1 && u0 != um1) ? c1 : SC_NEG;              // o - 2 -> o: the unit before differs
		c3 = (has_o && j >= 1 && um1 == SC_STAR) ? 0.f : SC_NEG;         // o - 3 -> o: the blank before the star that is skipped
		c4 = (c3 == 0.f && j >= 2 && um2 != u0) ? 0.f : SC_NEG;          // o - 4 -> o: the unit before that star, when it differs
	} else {
		c2 = (has_o && j + 1 < n && up1 != u0) ? (up1 == SC_STAR ? ent2 : 0.f) : SC_NEG;   // o -> o + 2
		c3 = (star0 && j + 1 < n) ? 0.f : SC_NEG;                                         // e -> e + 3: past this star
		c4 = (has_o && j + 2 < n && up1 == SC_STAR && up2 != u0) ? 0.f : SC_NEG;           // o -> o + 4: past the next star
	}
	const float* lpb = LP_LDS ? lpl : lpg;
	auto emis = [&](int t, float& ve, float& vo) {
		const float* row = lpb + (int64_t)t * C;
		float xe = row[blank], xo = row[cidx >= 0 ? cidx : blank];
		if (!LP_LDS) { xe = sc_floor(xe * SC_LOG2E); xo = sc_floor(xo * SC_LOG2E); }
		ve = has_e ? xe : SC_NEG;
		vo = cidx >= 0 ? xo : oconst;
	};
	float4* const mycol = col + (fwd ? 0 : 2) * colw + SC_PAD / 2;   // buffer p: mycol + p * colw, pair j at [j]
	float* const lat = (fwd ? alpha : beta) + (int64_t)b * T * cap;
	float* const off = offs + ((int64_t)(fwd ? 0 : 1) * B + b) * NB * half + j;   // block q of frames: off[q * half]
	const int t0 = fwd ? 0 : Tb - 1, dt = fwd ? 1 : -1;
	float ae, ao, ce = SC_NEG, co = SC_NEG, cum = 0.f;
	{
		float ee, eo;
		emis(t0, ee, eo);
		if (fwd) {
			ae = j == 0 ? ee : SC_NEG;
			ao = j == 0 ? eo + c1 : ((j == 1 && um1 == SC_STAR) ? eo : SC_NEG);
		} else {
			ae = (j == n || (last_star && j == n - 1)) ? ee : SC_NEG;
			ao = (j == n - 1 || (last_star && j == n - 2)) ? eo : SC_NEG;
		}
		ae = sc_floor(ae); ao = sc_floor(ao);
		mycol[j] = make_float4(ae, ao, 0.f, 0.f);
		*reinterpret_cast<sc_f2*>(lat + (int64_t)t0 * cap + e) = sc_f2{ae, ao};
		off[0] = 0.f;
		if (Tb > 1) emis(t0 + dt, ce, co);
	}
	__syncthreads();
	for (int k = 1; k < Tb; ++k) {   // the k-th frame of the sweep
		const int t = t0 + k * dt;
		const float4* prev = mycol + ((k - 1) & 1) * colw;
		float4* cur = mycol + (k & 1) * colw;
		float nxe = SC_NEG, nxo = SC_NEG;
		if (k + 1 < Tb) emis(t + dt, nxe, nxo);
		float ne, no, nbz;   // nbz: the offset of the neighbour pair the sweep comes from
		if (fwd) {
			const float4 p1 = prev[j - 1], p2 = prev[j - 2];   // the neighbour pairs' values, converted to this pair's offset (exact)
			const float d1 = p1.z - cum, x2 = p1.y + d1, x3 = p1.x + d1, x4 = p2.y + (p2.z - cum);
			ne = sc_lse2(ae, x2) + ce;
			no = sc_lse5(ao, ae + c1, x2 + c2, x3 + c3, x4 + c4) + co;
			nbz = p1.z;
		} else {
			const float4 n1 = prev[j + 1], n2 = prev[j + 2];
			const float d1 = n1.z - cum, y2 = n1.x + d1, y3 = n1.y + d1, y5 = n2.y + (n2.z - cum);
			ne = sc_lse3(ae, ao + c1, y3 + c3) + ce;
			no = sc_lse4(ao, y2, y3 + c2, y5 + c4) + co;
			nbz = n1.z;
		}
		ne = sc_floor(ne); no = sc_floor(no);
		// A pair no path has reached yet (both values the sentinel, which absorbs any offset) follows its neighbour's offset frame by frame,
		// so that the first values to arrive are O(10) against it: left at 0 they would be ~5 t in magnitude until the block ends, and in a
		// tight lattice (T close to the frames the labels need) every path runs through such freshly reached states.  A live pair changes
		// its offset at the first frame of a block only; the block's entry is rewritten every frame, and the last write is the offset of
		// every live value of the block.
		const float m = fmaxf(ne, no);
		if (!(m > SC_DEAD)) cum = nbz;
		else if ((k & (SC_RENORM - 1)) == 0 && m < INFINITY) {
			const float kk = floorf(m);
			ne -= kk; no -= kk;
			cum += kk;
		}
		off[(int64_t)(k >> SC_RENORM_LOG2) * half] = cum;
		ae = ne; ao = no;
		cur[j] = make_float4(ae, ao, cum, 0.f);
		*reinterpret_cast<sc_f2*>(lat + (int64_t)t * cap + e) = sc_f2{ae, ao};
		ce = nxe; co = nxo;
		__syncthreads();
	}
	if (tid == 0) {   // (mycol: the alpha sweep's)
		// the end states 2n (pair n), 2n - 1 (pair n - 1) and, behind a last star, 2n - 2 (pair n - 1) and 2n - 3 (pair n - 2), each at its
		// pair's offset; the pairs below pair 0 hold the sentinel.  The total is split into the offset of the largest and a remainder.
		const float4* fin = mycol + ((Tb - 1) & 1) * colw;
		const float4 pn = fin[n], pm1 = fin[n - 1], pm2 = fin[n - 2];
		const float v[4] = {pn.x, pm1.y, last_star ? pm1.x : SC_NEG, last_star ? pm2.y : SC_NEG}, c[4] = {pn.z, pm1.z, pm1.z, pm2.z};
		int best = 0;
		for (int i = 1; i < 4; ++i) if (v[i] > SC_DEAD && (!(v[best] > SC_DEAD) || v[i] + c[i] > v[best] + c[best])) best = i;
		const float cbest = c[best];
		float m = SC_NEG, l[4];
		for (int i = 0; i < 4; ++i) { l[i] = v[i] + (c[i] - cbest); m = fmaxf(m, l[i]); }
		const float rem = m + log2f((exp2f(l[0] - m) + exp2f(l[1] - m)) + (exp2f(l[2] - m) + exp2f(l[3] - m)));
		nll[b] = rem != rem ? NAN : (m > SC_DEAD ? (float)(-SC_LN2 * ((double)cbest + (double)rem)) : INFINITY);
		tot[4 * b] = cbest;
		tot[4 * b + 1] = rem;
		tot[4 * b + 2] = (float)L;
	}
}

__global__ __launch_bounds__(256) void star_ctc_grad_kernel(const float* __restrict__ lp, const int64_t* __restrict__ olen, const float* __restrict__ nll,
                                                            const float* __restrict__ alpha, const float* __restrict__ beta, const float* __restrict__ offs,
                                                            const float* __restrict__ tot, const int* __restrict__ desc, float* __restrict__ grad,
                                                            float* __restrict__ star_frames, int B, int T, int C, int S_max, int t_per_block, int cap, float pen2) {
	extern __shared__ float sc_bins[];  // [4][C] | [S_max + 1]
	float* const sf = sc_bins + 4 * C;
	const int NB = T / SC_RENORM + 1;
	const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int64_t Tb64 = olen[b];
	const int Tb = (Tb64 < 0 || Tb64 > T) ? 0 : (int)Tb64;
	const float loss = nll[b];
	const bool feasible = loss < INFINITY;   // (a NaN loss: not feasible, a zero gradient)
	float* mybins = sc_bins + wave * C;
	for (int g = threadIdx.x; g <= S_max; g += blockDim.x) sf[g] = 0.f;
	__syncthreads();
	const int t_begin = blockIdx.x * t_per_block, t_end = min(T, t_begin + t_per_block);
	const int* dr = desc + (int64_t)b * cap;
	for (int t = t_begin + wave; t < t_end; t += 4) {
		const float* row = lp + ((int64_t)b * T + t) * C;
		float* grow = grad ? grad + ((int64_t)b * T + t) * C : nullptr;
		if (t >= Tb || !feasible) {
			if (grow) for (int c = lane; c < C; c += 64) grow[c] = 0.f;
			continue;
		}
		for (int c = lane; c < C; c += 64) mybins[c] = 0.f;
		__builtin_amdgcn_s_waitcnt(0xc07f);
		__builtin_amdgcn_wave_barrier();
		const int L = min((int)tot[4 * b + 2], cap);
		const float* ar = alpha + ((int64_t)b * T + t) * cap;
		const float* br = beta + ((int64_t)b * T + t) * cap;
		// alpha + beta - total = (lattice values - remainder of total) + (offsets - integer part of total): the second group is exact
		const int half = cap >> 1;
		const float* oa = offs + ((int64_t)b * NB + (t >> SC_RENORM_LOG2)) * half;
		const float* ob = offs + (((int64_t)B + b) * NB + ((Tb - 1 - t) >> SC_RENORM_LOG2)) * half;
		const float ti = tot[4 * b], tr = tot[4 * b + 1];
		float occ = 0.f;
		for (int s = lane; s < L; s += 64) {
			const int d = dr[s];
			const float shift = ((oa[s >> 1] - ti) + ob[s >> 1]) - tr;   // the pair's offsets - integer part of total: exact
			const float ab = ar[s] + br[s];
			if (d >= 0) {
				const float p = sc_exp2(ab + (shift - sc_floor(row[d] * SC_LOG2E)));
				occ += p;
				atomicAdd(mybins + d, p);
			} else if (d <= -2 && -(d + 2) <= S_max) atomicAdd(sf - (d + 2), sc_exp2(ab + (shift - pen2)));
		}
		occ = wave_sum(occ);
		__builtin_amdgcn_s_waitcnt(0xc07f);
		__builtin_amdgcn_wave_barrier();
		if (grow) for (int c = lane; c < C; c += 64) grow[c] = occ * __expf(row[c]) - mybins[c];
		__builtin_amdgcn_wave_barrier();
	}
	__syncthreads();
	for (int g = threadIdx.x; g <= S_max; g += blockDim.x) {
		const float v = sf[g];
		if (v != 0.f) atomicAdd(star_frames + (int64_t)b * (S_max + 1) + g, v);
	}
}

// states per lattice row: every gap starred gives 2 (2 S_max + 1) + 1 states, rounded up to whole waves; -1 beyond SC_MAX_STATES
static int sc_cap(int S_max) {
	if (S_max < 0 || S_max > (SC_MAX_STATES - 4) / 4) return -1;
	return (4 * S_max + 3 + SC_WAVE_STATES - 1) / SC_WAVE_STATES * SC_WAVE_STATES;
}

extern "C" int convasr_star_ctc_states_per_wave(void) { return SC_WAVE_STATES; }
extern "C" int convasr_star_ctc_renorm_frames(void) { return SC_RENORM; }
extern "C" int convasr_star_ctc_max_states(void) { return SC_MAX_STATES - 1; }

extern "C" int convasr_star_ctc_supported(int B, int T, int C, int S_max) {
	return (B > 0 && B <= 65535 && T > 0 && T <= SC_MAX_T && C > 1 && C <= SC_MAX_C && sc_cap(S_max) > 0) ? 1 : 0;
}

extern "C" int64_t convasr_star_ctc_workspace_bytes(int B, int T, int C, int S_max) {
	if (!convasr_star_ctc_supported(B, T, C, S_max)) return convasr_fail(CONVASR_EUNSUPPORTED, "star_ctc_workspace_bytes: B %d, T %d, C %d, S_max %d outside the envelope (B <= 65535, T <= %d, C <= %d, S_max <= %d)", B, T, C, S_max, SC_MAX_T, SC_MAX_C, (SC_MAX_STATES - 4) / 4);
	const int64_t cap = sc_cap(S_max), NB = T / SC_RENORM + 1;
	return (2 * (int64_t)B * T * cap + (int64_t)B * NB * cap + 4 * (int64_t)B + (int64_t)B * cap) * 4;
}

extern "C" int convasr_star_ctc_loss(const float* log_probs, const int64_t* targets, const int64_t* olen, const int64_t* ylen, const uint8_t* star_mask,
                                     float star_penalty, float star_enter, float* nll, float* grad, float* star_frames, void* workspace,
                                     int B, int T, int C, int S_max, int blank, void* stream) {
	CONVASR_CHECK_ARG(log_probs && olen && ylen && star_mask && nll && star_frames && workspace && (targets || S_max == 0) && B > 0 && T > 0 && C > 1 && S_max >= 0 && blank >= 0 && blank < C, "star_ctc_loss: bad arguments");
	CONVASR_CHECK_ARG(star_penalty <= 0.f && star_enter <= 0.f, "star_ctc_loss: star_penalty %g and star_enter %g must be <= 0 (natural-log costs)", (double)star_penalty, (double)star_enter);
	if (!convasr_star_ctc_supported(B, T, C, S_max)) return convasr_fail(CONVASR_EUNSUPPORTED, "star_ctc_loss: B %d, T %d, C %d, S_max %d outside the envelope (B <= 65535, T <= %d, C <= %d, S_max <= %d: %d states with every gap starred)", B, T, C, S_max, SC_MAX_T, SC_MAX_C, (SC_MAX_STATES - 4) / 4, SC_MAX_STATES - 1);
	hipStream_t s = (hipStream_t)stream;
	const int cap = sc_cap(S_max), NB = T / SC_RENORM + 1;
	float* alpha = (float*)workspace;
	float* beta = alpha + (int64_t)B * T * cap;
	float* offs = beta + (int64_t)B * T * cap;
	float* tot = offs + (int64_t)B * NB * cap;
	int* desc = (int*)(tot + 4 * (int64_t)B);
	const float pen2 = fmaxf(star_penalty * SC_LOG2E, SC_NEG), ent2 = fmaxf(star_enter * SC_LOG2E, SC_NEG);
	const size_t lds_fixed = (size_t)sc_lds_words(cap, S_max) * 4, lds_lp = (size_t)T * C * 4;
	const bool in_lds = lds_fixed + lds_lp <= 159 * 1024;
#define SC_LAUNCH(LDS) do { \
		auto kern = star_ctc_alpha_beta_kernel<LDS>; \
		static unsigned long long set = 0; \
		convasr_allow_160k_lds(reinterpret_cast<const void*>(kern), set); \
		hipLaunchKernelGGL(kern, dim3(B), dim3(cap), lds_fixed + (LDS ? lds_lp : 0), s, log_probs, targets, olen, ylen, star_mask, nll, alpha, beta, offs, tot, desc, star_frames, B, T, C, S_max, blank, cap, pen2, ent2); \
	} while (0)
	if (in_lds) SC_LAUNCH(true); else SC_LAUNCH(false);
#undef SC_LAUNCH
	const int t_per_block = 32;
	static unsigned long long gset = 0;   // (4 C + S_max + 1 floats of bins: past 64 KiB from C = 4,033 on)
	convasr_allow_160k_lds(reinterpret_cast<const void*>(star_ctc_grad_kernel), gset);
	hipLaunchKernelGGL(star_ctc_grad_kernel, dim3((T + t_per_block - 1) / t_per_block, B), dim3(256), (4 * (size_t)C + S_max + 1) * sizeof(float), s,
	                   log_probs, olen, nll, alpha, beta, offs, tot, desc, grad, star_frames, B, T, C, S_max, t_per_block, cap, pen2);
	CONVASR_CHECK_LAUNCH("star_ctc_loss");
	return 0;
}
