// N-best minimum-word-error-rate (MWER) loss and gradient (this project's own rule, include/convasr_hip.h: convasr_mwer_loss; the
// sequence-level family of Prabhavalkar et al. 2018): the expected number of errors over an N-best list whose weights are the softmax of
// the hypotheses' CTC log-likelihoods, minus the list's mean risk.  All N lattices of an utterance read the SAME (T, C) log-prob slab and
// ONE gradient tensor per utterance is written; no copy per hypothesis exists anywhere.
//
// Kernel 1 (lattices) -- one workgroup per (b, n), csrc/star_ctc.hip's scheme without the star arcs: two halves of cap / 2 threads, the
// lower half runs the alpha sweep forward in time, the upper half the beta sweep backward, both in the same loop over k = 1 .. olen - 1
// with ONE workgroup barrier per frame.  Nothing is polled: every loop is bounded by olen <= T or by the state count.  A thread owns the
// (blank, label) pair j of its sweep -- states 2j and 2j+1 -- in registers; the column of the previous frame lives in LDS as one 16-byte
// entry per pair {blank, label, the pair's offset, -} (double-buffered, one sentinel pair on either side, so the neighbour pair needs no
// bounds test).  The plain three-arc recursion (s, s - 1, and s - 2 when the labels differ); an arc that does not exist is an additive
// cost of the sentinel, so the recursion is branch-free.  Arithmetic as star_ctc.hip documents it: fp32 log-sum-exp in base 2,
// "impossible" = the finite sentinel -1e30, and every MW_RENORM frames a PAIR of states loses floor(its maximum) -- an integer in the log2
// domain, so the subtraction, the running sum of the offsets and the conversion of the neighbour pair's values are exact.
// LP_LDS: the utterance's (olen, C) slab is staged into LDS when it fits beside the columns (753 x 38: 112 KiB).
// Kernel 2 (weights) -- one wave per utterance, one lane per hypothesis: the masked softmax of scale * ll with the wave maximum subtracted,
// E, rbar, loss, p and w, every reduction a butterfly of fixed order.
// Kernel 3 (gradient) -- one wave per (b, t): for n ascending with w != 0 the state posteriors exp2(alpha + beta - total - emission) times
// w[b, n] go into per-class LDS bins, then grad[b, :, t] is stored.  No atomics on global memory: everything is bit-reproducible.
#include "common.h"

#define MW_NEG (-1e30f)
#define MW_DEAD (-1e29f)         // anything below is "impossible"
#define MW_LOG2E 1.4426950408889634f
#define MW_LN2 0.6931471805599453
#define MW_RENORM 2
#define MW_RENORM_LOG2 1
#define MW_WAVE_STATES 128       // states of one wave of a sweep (two per lane)
#define MW_MAX_STATES 1024
#define MW_MAX_LABELS ((MW_MAX_STATES - 2) / 2)   // 511 labels: 1,023 states
#define MW_MAX_HYPS 64
#define MW_PAD 2
#define MW_MAX_T 8192
#define MW_MAX_C 8192

// -inf (and anything below the sentinel) becomes the sentinel; a NaN stays a NaN
__device__ __forceinline__ float mw_floor(float v) { return v < MW_NEG ? MW_NEG : v; }
__device__ __forceinline__ float mw_exp2(float v) { return __builtin_amdgcn_exp2f(v); }
__device__ __forceinline__ float mw_lse2(float a, float b) {
	const float m = fmaxf(a, b);
	return m + __builtin_amdgcn_logf(mw_exp2(a - m) + mw_exp2(b - m));
}
__device__ __forceinline__ float mw_lse3(float a, float b, float c) {
	const float m = fmaxf(a, fmaxf(b, c));
	return m + __builtin_amdgcn_logf(mw_exp2(a - m) + mw_exp2(b - m) + mw_exp2(c - m));
}

typedef float mw_f2 __attribute__((ext_vector_type(2)));

// 32-bit words of LDS ahead of the log-prob slab: columns [2 sweeps][2 buffers][cap / 2 + MW_PAD pairs][4] | label classes [cap / 2 + 2],
// rounded up to 16 bytes
__host__ __device__ static inline int mw_lds_words(int cap) {
	return (16 * (cap / 2 + MW_PAD) + (cap / 2 + 2) + 3) & ~3;
}

// Workspace, ls = 2 L_max + 2: alpha, beta [B N][T][ls] fp32 | offs [2][B N][NB][ls / 2] | tot [B N][4] = {integer part, remainder of the log2 likelihood,
// states, -} | w [B N]
template <bool LP_LDS>
__global__ __launch_bounds__(1024) void mwer_alpha_beta_kernel(const float* __restrict__ lp, const int64_t* __restrict__ hyps, const int64_t* __restrict__ hyp_lengths,
                                                               const int64_t* __restrict__ olen, float* __restrict__ nll, float* __restrict__ alpha,
                                                               float* __restrict__ beta, float* __restrict__ offs, float* __restrict__ tot,
                                                               int BN, int N, int T, int C, int L_max, int blank, int cap) {
	extern __shared__ __attribute__((aligned(16))) float mw_smem[];
	const int ls = 2 * L_max + 2, lh = L_max + 1;   // the workspace's row of states and of pairs: the threads beyond it own no state of any hypothesis and store nothing
	const int half = cap >> 1, tid = threadIdx.x, nthr = blockDim.x, bn = blockIdx.x, b = bn / N;
	const int colw = half + MW_PAD;   // pairs per column buffer: one sentinel pair below pair 0, one above the last
	float4* const col = reinterpret_cast<float4*>(mw_smem);
	int* const ucls = reinterpret_cast<int*>(mw_smem + 16 * colw);   // label i at ucls[1 + i]; -1: no label, or one outside [0, C) (nothing matches it)
	float* const lpl = mw_smem + mw_lds_words(cap);
	const int NB = T / MW_RENORM + 1;
	const int64_t Tb64 = olen[b], L64 = hyp_lengths[bn];
	if (Tb64 <= 0 || Tb64 > T || L64 < 0 || L64 > L_max) {  // uniform over the workgroup: an absent hypothesis, a bad length
		if (tid == 0) { nll[bn] = INFINITY; tot[4 * bn + 2] = 0.f; }
		return;
	}
	const int Tb = (int)Tb64, n = (int)L64, L = 2 * n + 1;
	const float* lpg = lp + (int64_t)b * T * C;   // the utterance's slab, shared by its N workgroups
	const int64_t* hy = hyps + (int64_t)bn * L_max;

	for (int i = tid; i < half + 2; i += nthr) {
		int u = -1;
		if (i >= 1 && i - 1 < n) {
			const int64_t y = hy[i - 1];
			u = (y >= 0 && y < C) ? (int)y : -1;
		}
		ucls[i] = u;
	}
	for (int i = tid; i < 4 * colw; i += nthr) col[i] = make_float4(MW_NEG, MW_NEG, 0.f, 0.f);
	if (LP_LDS) {
		const int cnt = Tb * C;
		for (int i = tid; i < cnt; i += nthr) lpl[i] = mw_floor(lpg[i] * MW_LOG2E);
	}
	__syncthreads();

	// ---- this thread's pair of states and the arc that skips a blank
	const bool fwd = tid < half;
	const int j = fwd ? tid : tid - half, e = 2 * j;
	const bool has_e = j <= n, has_o = j < n;
	const int cidx = ucls[1 + j];   // (-1 for j >= n)
	// the labels' raw values decide whether two neighbours differ: a repeated label outside [0, C) is still a repeat
	const int64_t y0 = has_o ? hy[j] : -1, ym1 = (has_o && j >= 1) ? hy[j - 1] : -1, yp1 = (j + 1 < n) ? hy[j + 1] : -1;
	float c2;
	if (fwd) c2 = (has_o && j >= 1 && y0 != ym1) ? 0.f : MW_NEG;   // o - 2 -> o: the label before differs
	else c2 = (j + 1 < n && yp1 != y0) ? 0.f : MW_NEG;             // o -> o + 2
	const float* lpb = LP_LDS ? lpl : lpg;
	auto emis = [&](int t, float& ve, float& vo) {
		const float* row = lpb + (int64_t)t * C;
		float xe = row[blank], xo = row[cidx >= 0 ? cidx : blank];
		if (!LP_LDS) { xe = mw_floor(xe * MW_LOG2E); xo = mw_floor(xo * MW_LOG2E); }
		ve = has_e ? xe : MW_NEG;
		vo = cidx >= 0 ? xo : MW_NEG;
	};
	float4* const mycol = col + (fwd ? 0 : 2) * colw + MW_PAD / 2;   // buffer p: mycol + p * colw, pair j at [j]
	float* const lat = (fwd ? alpha : beta) + (int64_t)bn * T * ls;
	const bool st = j < lh;
	float* const off = offs + ((int64_t)(fwd ? 0 : 1) * BN + bn) * NB * lh + j;   // block q of frames: off[q * lh]
	const int t0 = fwd ? 0 : Tb - 1, dt = fwd ? 1 : -1;
	float ae, ao, ce = MW_NEG, co = MW_NEG, cum = 0.f;
	{
		float ee, eo;
		emis(t0, ee, eo);
		if (fwd) {
			ae = j == 0 ? ee : MW_NEG;
			ao = j == 0 ? eo : MW_NEG;
		} else {
			ae = j == n ? ee : MW_NEG;
			ao = j == n - 1 ? eo : MW_NEG;
		}
		ae = mw_floor(ae); ao = mw_floor(ao);
		mycol[j] = make_float4(ae, ao, 0.f, 0.f);
		if (st) {
			*reinterpret_cast<mw_f2*>(lat + (int64_t)t0 * ls + e) = mw_f2{ae, ao};
			off[0] = 0.f;
		}
		if (Tb > 1) emis(t0 + dt, ce, co);
	}
	__syncthreads();
	for (int k = 1; k < Tb; ++k) {   // the k-th frame of the sweep
		const int t = t0 + k * dt;
		const float4* prev = mycol + ((k - 1) & 1) * colw;
		float4* cur = mycol + (k & 1) * colw;
		float nxe = MW_NEG, nxo = MW_NEG;
		if (k + 1 < Tb) emis(t + dt, nxe, nxo);
		float ne, no, nbz;   // nbz: the offset of the neighbour pair the sweep comes from
		if (fwd) {
			const float4 p1 = prev[j - 1];   // the neighbour pair's label, converted to this pair's offset (exact)
			const float x2 = p1.y + (p1.z - cum);
			ne = mw_lse2(ae, x2) + ce;
			no = mw_lse3(ao, ae, x2 + c2) + co;
			nbz = p1.z;
		} else {
			const float4 n1 = prev[j + 1];
			const float d1 = n1.z - cum, y2 = n1.x + d1, y3 = n1.y + d1;
			ne = mw_lse2(ae, ao) + ce;
			no = mw_lse3(ao, y2, y3 + c2) + co;
			nbz = n1.z;
		}
		ne = mw_floor(ne); no = mw_floor(no);
		// A pair no path has reached yet (both values the sentinel, which absorbs any offset) follows its neighbour's offset frame by frame,
		// so that the first values to arrive are O(10) against it.  A live pair changes its offset at the first frame of a block only; the
		// block's entry is rewritten every frame, and the last write is the offset of every live value of the block.
		const float m = fmaxf(ne, no);
		if (!(m > MW_DEAD)) cum = nbz;
		else if ((k & (MW_RENORM - 1)) == 0 && m < INFINITY) {
			const float kk = floorf(m);
			ne -= kk; no -= kk;
			cum += kk;
		}
		ae = ne; ao = no;
		cur[j] = make_float4(ae, ao, cum, 0.f);
		if (st) {
			off[(int64_t)(k >> MW_RENORM_LOG2) * lh] = cum;
			*reinterpret_cast<mw_f2*>(lat + (int64_t)t * ls + e) = mw_f2{ae, ao};
		}
		ce = nxe; co = nxo;
		__syncthreads();
	}
	if (tid == 0) {   // (mycol: the alpha sweep's)
		// the end states 2n (pair n) and 2n - 1 (pair n - 1), each at its pair's offset; the pair below pair 0 holds the sentinel.  The total
		// is split into the offset of the larger and a remainder.
		const float4* fin = mycol + ((Tb - 1) & 1) * colw;
		const float4 pn = fin[n], pm1 = fin[n - 1];
		const bool second = pm1.y > MW_DEAD && (!(pn.x > MW_DEAD) || pm1.y + pm1.z > pn.x + pn.z);
		const float cbest = second ? pm1.z : pn.z;
		const float l0 = pn.x + (pn.z - cbest), l1 = pm1.y + (pm1.z - cbest), m = fmaxf(l0, l1);
		const float rem = m + log2f(exp2f(l0 - m) + exp2f(l1 - m));
		nll[bn] = rem != rem ? NAN : (m > MW_DEAD ? (float)(-MW_LN2 * ((double)cbest + (double)rem)) : INFINITY);
		tot[4 * bn] = cbest;
		tot[4 * bn + 1] = rem;
		tot[4 * bn + 2] = (float)L;
	}
}

// One wave per utterance, lane n = hypothesis n.  A hypothesis takes part iff its nll is finite (absent ones were given +inf).
__global__ __launch_bounds__(64) void mwer_weights_kernel(const float* __restrict__ nll, const float* __restrict__ risk, float scale, float* __restrict__ loss,
                                                          float* __restrict__ post, float* __restrict__ w, int N) {
	const int b = blockIdx.x, lane = threadIdx.x;
	const bool in = lane < N;
	const float v = in ? nll[(int64_t)b * N + lane] : INFINITY;
	const bool part = in && fabsf(v) < INFINITY;   // (false for a NaN)
	const float ll = part ? -v : -INFINITY;
	const float cnt = wave_sum(part ? 1.f : 0.f);
	const float llmax = wave_max(ll);
	float p = 0.f, wv = 0.f, l = 0.f;
	if (cnt > 0.5f) {   // uniform
		const float r = part ? risk[(int64_t)b * N + lane] : 0.f;
		const float ex = part ? expf(scale * (ll - llmax)) : 0.f;
		const float Z = wave_sum(ex);   // >= 1: the maximum's own term
		p = ex / Z;
		const float E = wave_sum(p * r), rbar = wave_sum(r) / cnt;
		if (cnt > 1.5f) {
			l = E - rbar;
			wv = part ? scale * p * (r - E) : 0.f;
		}
	}
	if (in) {
		post[(int64_t)b * N + lane] = p;
		w[(int64_t)b * N + lane] = wv;
	}
	if (lane == 0) loss[b] = l;
}

__global__ __launch_bounds__(256) void mwer_grad_kernel(const float* __restrict__ lp, const int64_t* __restrict__ hyps, const int64_t* __restrict__ olen,
                                                        const float* __restrict__ alpha, const float* __restrict__ beta, const float* __restrict__ offs,
                                                        const float* __restrict__ tot, const float* __restrict__ w, float* __restrict__ grad,
                                                        int B, int N, int T, int C, int L_max, int blank, int t_per_block) {
	extern __shared__ float mw_bins[];  // [4][C]
	const int NB = T / MW_RENORM + 1, BN = B * N, ls = 2 * L_max + 2, lh = L_max + 1;
	const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int64_t Tb64 = olen[b];
	const int Tb = (Tb64 < 0 || Tb64 > T) ? 0 : (int)Tb64;
	float* mybins = mw_bins + wave * C;
	const int t_begin = blockIdx.x * t_per_block, t_end = min(T, t_begin + t_per_block);
	for (int t = t_begin + wave; t < t_end; t += 4) {
		const float* row = lp + ((int64_t)b * T + t) * C;
		float* grow = grad + ((int64_t)b * T + t) * C;
		if (t >= Tb) {
			for (int c = lane; c < C; c += 64) grow[c] = 0.f;
			continue;
		}
		for (int c = lane; c < C; c += 64) mybins[c] = 0.f;
		__builtin_amdgcn_s_waitcnt(0xc07f);
		__builtin_amdgcn_wave_barrier();
		for (int n = 0; n < N; ++n) {   // ascending: a fixed order of the additions into a bin
			const int bn = b * N + n;
			const float wn = w[bn];
			if (wn == 0.f) continue;   // uniform over the wave
			const int L = min((int)tot[4 * bn + 2], ls - 1);
			const float* ar = alpha + ((int64_t)bn * T + t) * ls;
			const float* br = beta + ((int64_t)bn * T + t) * ls;
			// alpha + beta - total = (lattice values - remainder of total) + (offsets - integer part of total): the second group is exact
			const float* oa = offs + ((int64_t)bn * NB + (t >> MW_RENORM_LOG2)) * lh;
			const float* ob = offs + (((int64_t)BN + bn) * NB + ((Tb - 1 - t) >> MW_RENORM_LOG2)) * lh;
			const float ti = tot[4 * bn], tr = tot[4 * bn + 1];
			const int64_t* hy = hyps + (int64_t)bn * L_max;
			for (int s = lane; s < L; s += 64) {
				int d = blank;
				if (s & 1) {
					const int64_t y = hy[s >> 1];
					d = (y >= 0 && y < C) ? (int)y : -1;
				}
				if (d < 0) continue;
				const float shift = ((oa[s >> 1] - ti) + ob[s >> 1]) - tr;
				const float ab = ar[s] + br[s];
				atomicAdd(mybins + d, wn * mw_exp2(ab + (shift - mw_floor(row[d] * MW_LOG2E))));
			}
			__builtin_amdgcn_s_waitcnt(0xc07f);
			__builtin_amdgcn_wave_barrier();
		}
		for (int c = lane; c < C; c += 64) grow[c] = mybins[c];
		__builtin_amdgcn_wave_barrier();
	}
}

// states per lattice row: 2 L_max + 1, rounded up to whole waves; -1 beyond MW_MAX_STATES
static int mw_cap(int L_max) {
	if (L_max < 0 || L_max > MW_MAX_LABELS) return -1;
	return (2 * L_max + 1 + MW_WAVE_STATES - 1) / MW_WAVE_STATES * MW_WAVE_STATES;
}

extern "C" int convasr_mwer_states_per_wave(void) { return MW_WAVE_STATES; }
extern "C" int convasr_mwer_renorm_frames(void) { return MW_RENORM; }
extern "C" int convasr_mwer_max_labels(void) { return MW_MAX_LABELS; }
extern "C" int convasr_mwer_max_hyps(void) { return MW_MAX_HYPS; }

extern "C" int convasr_mwer_supported(int B, int N, int T, int C, int L_max) {
	return (B > 0 && B <= 65535 && N > 0 && N <= MW_MAX_HYPS && T > 0 && T <= MW_MAX_T && C > 1 && C <= MW_MAX_C && mw_cap(L_max) > 0) ? 1 : 0;
}

#define MW_ENVELOPE "outside the envelope (B <= 65535, N <= %d hypotheses, T <= %d, C <= %d, L_max <= %d labels: %d states)"

extern "C" int64_t convasr_mwer_workspace_bytes(int B, int N, int T, int C, int L_max) {
	if (!convasr_mwer_supported(B, N, T, C, L_max)) return convasr_fail(CONVASR_EUNSUPPORTED, "mwer_workspace_bytes: B %d, N %d, T %d, C %d, L_max %d " MW_ENVELOPE, B, N, T, C, L_max, MW_MAX_HYPS, MW_MAX_T, MW_MAX_C, MW_MAX_LABELS, MW_MAX_STATES - 1);
	const int64_t BN = (int64_t)B * N, ls = 2 * (int64_t)L_max + 2, NB = T / MW_RENORM + 1;
	return (2 * BN * T * ls + BN * NB * ls + 4 * BN + BN) * 4;
}

extern "C" int convasr_mwer_loss(const float* log_probs, const int64_t* hyps, const int64_t* hyp_lengths, const int64_t* olen, const float* risk, float scale,
                                 float* loss, float* grad, float* hyp_nll, float* hyp_posterior, void* workspace,
                                 int B, int N, int T, int C, int L_max, int blank, void* stream) {
	CONVASR_CHECK_ARG(log_probs && hyp_lengths && olen && risk && loss && hyp_nll && hyp_posterior && workspace && (hyps || L_max == 0) && B > 0 && N > 0 && T > 0 && C > 1 && L_max >= 0 && blank >= 0 && blank < C, "mwer_loss: bad arguments");
	CONVASR_CHECK_ARG(scale > 0.f && scale < INFINITY, "mwer_loss: scale %g must be a finite number > 0", (double)scale);
	if (!convasr_mwer_supported(B, N, T, C, L_max)) return convasr_fail(CONVASR_EUNSUPPORTED, "mwer_loss: B %d, N %d, T %d, C %d, L_max %d " MW_ENVELOPE, B, N, T, C, L_max, MW_MAX_HYPS, MW_MAX_T, MW_MAX_C, MW_MAX_LABELS, MW_MAX_STATES - 1);
	hipStream_t s = (hipStream_t)stream;
	const int cap = mw_cap(L_max), NB = T / MW_RENORM + 1, BN = B * N;
	float* alpha = (float*)workspace;
	const int64_t ls = 2 * (int64_t)L_max + 2;   // a lattice row: the 2 L_max + 1 states, made even
	float* beta = alpha + (int64_t)BN * T * ls;
	float* offs = beta + (int64_t)BN * T * ls;
	float* tot = offs + (int64_t)BN * NB * ls;
	float* w = tot + 4 * (int64_t)BN;
	const size_t lds_fixed = (size_t)mw_lds_words(cap) * 4, lds_lp = (size_t)T * C * 4;
	const bool in_lds = lds_fixed + lds_lp <= 159 * 1024;
#define MW_LAUNCH(LDS) do { \
		auto kern = mwer_alpha_beta_kernel<LDS>; \
		static unsigned long long set = 0; \
		convasr_allow_160k_lds(reinterpret_cast<const void*>(kern), set); \
		hipLaunchKernelGGL(kern, dim3(BN), dim3(cap), lds_fixed + (LDS ? lds_lp : 0), s, log_probs, hyps, hyp_lengths, olen, hyp_nll, alpha, beta, offs, tot, BN, N, T, C, L_max, blank, cap); \
	} while (0)
	if (in_lds) MW_LAUNCH(true); else MW_LAUNCH(false);
#undef MW_LAUNCH
	hipLaunchKernelGGL(mwer_weights_kernel, dim3(B), dim3(64), 0, s, hyp_nll, risk, scale, loss, hyp_posterior, w, N);
	if (grad) {
		const int t_per_block = 32;
		static unsigned long long gset = 0;   // (4 C floats of bins: past 64 KiB from C = 4,097 on)
		convasr_allow_160k_lds(reinterpret_cast<const void*>(mwer_grad_kernel), gset);
		hipLaunchKernelGGL(mwer_grad_kernel, dim3((T + t_per_block - 1) / t_per_block, B), dim3(256), 4 * (size_t)C * sizeof(float), s,
		                   log_probs, hyps, olen, alpha, beta, offs, tot, w, grad, B, N, T, C, L_max, blank, t_per_block);
	}
	CONVASR_CHECK_LAUNCH("mwer_loss");
	return 0;
}
