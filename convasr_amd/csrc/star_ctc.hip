// Star-token CTC loss and gradient (this project's own rule, include/convasr_hip.h: convasr_star_ctc_loss; the W-CTC / Star Temporal
// Classification family): the transcript may miss words, so an optional STAR unit -- "any stretch of frames, or nothing" -- stands in
// every allowed gap between the labels.  The lattice has up to five arcs into a state (s, s-1, s-2 and, around a star that is skipped,
// s-3, s-4), which csrc/ctc.hip's two-neighbour recursion cannot express.
//
// Kernel 1 -- one workgroup per utterance runs pair_lattice.h's alpha-beta sweep (scheme, arithmetic and per-pair offsets: there) with
// STAR = true: two sentinel pairs on either side of a column, the neighbour pairs j-1, j-2 / j+1, j+2, and an arc into a star costs
// star_enter.  The per-unit descriptor (class, star or nothing; the gap of a star) is built in LDS from targets, ylen and star_mask by a
// prefix count over the mask, and its per-state form goes to the workspace for kernel 2.
// Kernel 2 -- one wave per frame: posterior of every state = exp2(alpha + beta - total - emission); label and blank states go to LDS bins
// per class, their sum is occ, star states go to LDS bins per gap (added to star_frames once per workgroup: fp32 atomics on global
// memory, so star_frames is reproducible to rounding only; nll and grad are bit-reproducible).  grad = occ * exp(lp) - posterior.
#include "common.h"
#include "pair_lattice.h"

enum { SC_STAR = -1, SC_BAD = -2, SC_NONE = -3 };  // unit kinds below the classes: a star, a label outside [0, C) (never matches), no unit

// 32-bit words of LDS ahead of the log-prob slab: columns [2 sweeps][2 buffers][cap / 2 + PL_PAD pairs][4] | unit kinds
// [cap / 2 + 4] | unit gaps [cap / 2] | mask [S_max + 2] | unit count [4], rounded up to 16 bytes
__host__ __device__ static inline int sc_lds_words(int cap, int S_max) {
	return (16 * (cap / 2 + PL_PAD<true>) + (cap / 2 + 4) + cap / 2 + (S_max + 2) + 4 + 3) & ~3;
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
	float4* const col = reinterpret_cast<float4*>(sc_smem);
	int* const ucls = reinterpret_cast<int*>(sc_smem + 16 * (half + PL_PAD<true>));   // unit i at ucls[2 + i]
	int* const ugap = ucls + half + 4;
	int* const msk = ugap + half;
	int* const nsh = msk + S_max + 2;
	float* const lpl = sc_smem + sc_lds_words(cap, S_max);
	const int NB = T / PL_RENORM + 1;
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
	pair_lattice_stage<true, LP_LDS>(col, half, lpl, lpg, Tb * C);
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
	const int j = fwd ? tid : tid - half;
	const int u0 = ucls[2 + j], um1 = ucls[1 + j], um2 = ucls[j], up1 = ucls[3 + j], up2 = ucls[4 + j];
	const bool has_o = j < n, star0 = u0 == SC_STAR;
	const float c1 = star0 ? ent2 : 0.f;   // e -> o: into a star
	float c2, c3, c4;
	if (fwd) {
		c2 = (has_o && j >= 1 && u0 != um1) ? c1 : LOG2_NEG;              // o - 2 -> o: the unit before differs
		c3 = (has_o && j >= 1 && um1 == SC_STAR) ? 0.f : LOG2_NEG;         // o - 3 -> o: the blank before the star that is skipped
		c4 = (c3 == 0.f && j >= 2 && um2 != u0) ? 0.f : LOG2_NEG;          // o - 4 -> o: the unit before that star, when it differs
	} else {
		c2 = (has_o && j + 1 < n && up1 != u0) ? (up1 == SC_STAR ? ent2 : 0.f) : LOG2_NEG;   // o -> o + 2
		c3 = (star0 && j + 1 < n) ? 0.f : LOG2_NEG;                                         // e -> e + 3: past this star
		c4 = (has_o && j + 2 < n && up1 == SC_STAR && up2 != u0) ? 0.f : LOG2_NEG;           // o -> o + 4: past the next star
	}
	PairLattice p;
	p.lpb = LP_LDS ? lpl : lpg; p.col = col;
	p.alpha = alpha + (int64_t)b * T * cap; p.beta = beta + (int64_t)b * T * cap;
	p.offa = offs + (int64_t)b * NB * half; p.offb = offs + ((int64_t)B + b) * NB * half;
	p.nll = nll + b; p.tot = tot + 4 * b;
	p.Tb = Tb; p.C = C; p.blank = blank; p.half = half; p.ls = cap; p.lh = half;   // every thread's pair lies inside the row
	p.n = n; p.last_star = n >= 1 && ucls[2 + n - 1] == SC_STAR;
	p.fwd = fwd; p.st = true; p.j = j; p.cidx = u0 >= 0 ? u0 : -1; p.prev_star = um1 == SC_STAR;
	p.oconst = star0 ? pen2 : LOG2_NEG;
	p.c1 = c1; p.c2 = c2; p.c3 = c3; p.c4 = c4;
	pair_lattice_sweep<true, LP_LDS>(p);
}

__global__ __launch_bounds__(256) void star_ctc_grad_kernel(const float* __restrict__ lp, const int64_t* __restrict__ olen, const float* __restrict__ nll,
                                                            const float* __restrict__ alpha, const float* __restrict__ beta, const float* __restrict__ offs,
                                                            const float* __restrict__ tot, const int* __restrict__ desc, float* __restrict__ grad,
                                                            float* __restrict__ star_frames, int B, int T, int C, int S_max, int t_per_block, int cap, float pen2) {
	extern __shared__ float sc_bins[];  // [4][C] | [S_max + 1]
	float* const sf = sc_bins + 4 * C;
	const int NB = T / PL_RENORM + 1;
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
		const int half = cap >> 1;
		const float* oa = offs + ((int64_t)b * NB + (t >> PL_RENORM_LOG2)) * half;
		const float* ob = offs + (((int64_t)B + b) * NB + ((Tb - 1 - t) >> PL_RENORM_LOG2)) * half;
		const float ti = tot[4 * b], tr = tot[4 * b + 1];
		float occ = 0.f;
		for (int s = lane; s < L; s += 64) {
			const int d = dr[s];
			const float shift = pl_posterior_shift(oa[s >> 1], ob[s >> 1], ti, tr);
			const float ab = ar[s] + br[s];
			if (d >= 0) {
				const float p = pl_exp2(ab + (shift - log2_floor(row[d] * LOG2_E)));
				occ += p;
				atomicAdd(mybins + d, p);
			} else if (d <= -2 && -(d + 2) <= S_max) atomicAdd(sf - (d + 2), pl_exp2(ab + (shift - pen2)));
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

// threads of a lattice: every gap starred gives 2 (2 S_max + 1) + 1 states; -1 beyond S_max = (PL_MAX_STATES - 4) / 4
static int sc_cap(int S_max) { return pl_cap(4 * (int64_t)S_max + 3); }

extern "C" int convasr_star_ctc_states_per_wave(void) { return PL_WAVE_STATES; }
extern "C" int convasr_star_ctc_renorm_frames(void) { return PL_RENORM; }
extern "C" int convasr_star_ctc_max_states(void) { return PL_MAX_STATES - 1; }

extern "C" int convasr_star_ctc_supported(int B, int T, int C, int S_max) {
	return (B > 0 && B <= 65535 && T > 0 && T <= PL_MAX_T && C > 1 && C <= PL_MAX_C && sc_cap(S_max) > 0) ? 1 : 0;
}

extern "C" int64_t convasr_star_ctc_workspace_bytes(int B, int T, int C, int S_max) {
	if (!convasr_star_ctc_supported(B, T, C, S_max)) return convasr_fail(CONVASR_EUNSUPPORTED, "star_ctc_workspace_bytes: B %d, T %d, C %d, S_max %d outside the envelope (B <= 65535, T <= %d, C <= %d, S_max <= %d)", B, T, C, S_max, PL_MAX_T, PL_MAX_C, (PL_MAX_STATES - 4) / 4);
	const int64_t cap = sc_cap(S_max), NB = T / PL_RENORM + 1;
	return (2 * (int64_t)B * T * cap + (int64_t)B * NB * cap + 4 * (int64_t)B + (int64_t)B * cap) * 4;
}

extern "C" int convasr_star_ctc_loss(const float* log_probs, const int64_t* targets, const int64_t* olen, const int64_t* ylen, const uint8_t* star_mask,
                                     float star_penalty, float star_enter, float* nll, float* grad, float* star_frames, void* workspace,
                                     int B, int T, int C, int S_max, int blank, void* stream) {
	CONVASR_CHECK_ARG(log_probs && olen && ylen && star_mask && nll && star_frames && workspace && (targets || S_max == 0) && B > 0 && T > 0 && C > 1 && S_max >= 0 && blank >= 0 && blank < C, "star_ctc_loss: bad arguments");
	CONVASR_CHECK_ARG(star_penalty <= 0.f && star_enter <= 0.f, "star_ctc_loss: star_penalty %g and star_enter %g must be <= 0 (natural-log costs)", (double)star_penalty, (double)star_enter);
	if (!convasr_star_ctc_supported(B, T, C, S_max)) return convasr_fail(CONVASR_EUNSUPPORTED, "star_ctc_loss: B %d, T %d, C %d, S_max %d outside the envelope (B <= 65535, T <= %d, C <= %d, S_max <= %d: %d states with every gap starred)", B, T, C, S_max, PL_MAX_T, PL_MAX_C, (PL_MAX_STATES - 4) / 4, PL_MAX_STATES - 1);
	hipStream_t s = (hipStream_t)stream;
	const int cap = sc_cap(S_max), NB = T / PL_RENORM + 1;
	float* alpha = (float*)workspace;
	float* beta = alpha + (int64_t)B * T * cap;
	float* offs = beta + (int64_t)B * T * cap;
	float* tot = offs + (int64_t)B * NB * cap;
	int* desc = (int*)(tot + 4 * (int64_t)B);
	const float pen2 = fmaxf(star_penalty * LOG2_E, LOG2_NEG), ent2 = fmaxf(star_enter * LOG2_E, LOG2_NEG);
	pl_launch<star_ctc_alpha_beta_kernel<true>, star_ctc_alpha_beta_kernel<false>>(B, cap, (size_t)sc_lds_words(cap, S_max) * 4, T, C, s,
		log_probs, targets, olen, ylen, star_mask, nll, alpha, beta, offs, tot, desc, star_frames, B, T, C, S_max, blank, cap, pen2, ent2);
	const int t_per_block = 32;
	static unsigned long long gset = 0;   // (4 C + S_max + 1 floats of bins: past 64 KiB from C = 4,033 on)
	convasr_allow_160k_lds(reinterpret_cast<const void*>(star_ctc_grad_kernel), gset);
	hipLaunchKernelGGL(star_ctc_grad_kernel, dim3((T + t_per_block - 1) / t_per_block, B), dim3(256), (4 * (size_t)C + S_max + 1) * sizeof(float), s,
	                   log_probs, olen, nll, alpha, beta, offs, tot, desc, grad, star_frames, B, T, C, S_max, t_per_block, cap, pen2);
	CONVASR_CHECK_LAUNCH("star_ctc_loss");
	return 0;
}
