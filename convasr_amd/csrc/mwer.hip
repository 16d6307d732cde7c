// N-best minimum-word-error-rate (MWER) loss and gradient (this project's own rule, include/convasr_hip.h: convasr_mwer_loss; the
// sequence-level family of Prabhavalkar et al. 2018): the expected number of errors over an N-best list whose weights are the softmax of
// the hypotheses' CTC log-likelihoods, minus the list's mean risk.  All N lattices of an utterance read the SAME (T, C) log-prob slab and
// ONE gradient tensor per utterance is written; no copy per hypothesis exists anywhere.
//
// Kernel 1 (lattices) -- one workgroup per (b, n) runs pair_lattice.h's alpha-beta sweep (scheme, arithmetic and per-pair offsets: there)
// with STAR = false: the plain three-arc recursion, one sentinel pair on either side of a column.
// Kernel 2 (weights) -- one wave per utterance, one lane per hypothesis: the masked softmax of scale * ll with the wave maximum subtracted,
// E, rbar, loss, p and w, every reduction a butterfly of fixed order.
// Kernel 3 (gradient) -- one wave per (b, t): for n ascending with w != 0 the state posteriors exp2(alpha + beta - total - emission) times
// w[b, n] go into per-class LDS bins, then grad[b, :, t] is stored.  No atomics on global memory: everything is bit-reproducible.
#include "common.h"
#include "pair_lattice.h"

#define MW_MAX_LABELS ((PL_MAX_STATES - 2) / 2)   // 511 labels: 1,023 states
#define MW_MAX_HYPS 64

// 32-bit words of LDS ahead of the log-prob slab: columns [2 sweeps][2 buffers][cap / 2 + PL_PAD pairs][4] | label classes [cap / 2 + 2],
// rounded up to 16 bytes
__host__ __device__ static inline int mw_lds_words(int cap) {
	return (16 * (cap / 2 + PL_PAD<false>) + (cap / 2 + 2) + 3) & ~3;
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
	float4* const col = reinterpret_cast<float4*>(mw_smem);
	int* const ucls = reinterpret_cast<int*>(mw_smem + 16 * (half + PL_PAD<false>));   // label i at ucls[1 + i]; -1: no label, or one outside [0, C) (nothing matches it)
	float* const lpl = mw_smem + mw_lds_words(cap);
	const int NB = T / PL_RENORM + 1;
	const int64_t Tb64 = olen[b], L64 = hyp_lengths[bn];
	if (Tb64 <= 0 || Tb64 > T || L64 < 0 || L64 > L_max) {  // uniform over the workgroup: an absent hypothesis, a bad length
		if (tid == 0) { nll[bn] = INFINITY; tot[4 * bn + 2] = 0.f; }
		return;
	}
	const int Tb = (int)Tb64, n = (int)L64;
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
	pair_lattice_stage<false, LP_LDS>(col, half, lpl, lpg, Tb * C);
	__syncthreads();

	// ---- this thread's pair of states and the arc that skips a blank
	const bool fwd = tid < half;
	const int j = fwd ? tid : tid - half;
	const bool has_o = j < n;
	// the labels' raw values decide whether two neighbours differ: a repeated label outside [0, C) is still a repeat
	const int64_t y0 = has_o ? hy[j] : -1, ym1 = (has_o && j >= 1) ? hy[j - 1] : -1, yp1 = (j + 1 < n) ? hy[j + 1] : -1;
	float c2;
	if (fwd) c2 = (has_o && j >= 1 && y0 != ym1) ? 0.f : LOG2_NEG;   // o - 2 -> o: the label before differs
	else c2 = (j + 1 < n && yp1 != y0) ? 0.f : LOG2_NEG;             // o -> o + 2
	PairLattice p;
	p.lpb = LP_LDS ? lpl : lpg; p.col = col;
	p.alpha = alpha + (int64_t)bn * T * ls; p.beta = beta + (int64_t)bn * T * ls;
	p.offa = offs + (int64_t)bn * NB * lh; p.offb = offs + ((int64_t)BN + bn) * NB * lh;
	p.nll = nll + bn; p.tot = tot + 4 * bn;
	p.Tb = Tb; p.C = C; p.blank = blank; p.half = half; p.ls = ls; p.lh = lh;
	p.n = n; p.last_star = false;
	p.fwd = fwd; p.st = j < lh; p.j = j; p.cidx = ucls[1 + j]; p.prev_star = false;   // (cidx: -1 for j >= n)
	p.oconst = LOG2_NEG;
	p.c1 = 0.f; p.c2 = c2; p.c3 = p.c4 = LOG2_NEG;
	pair_lattice_sweep<false, LP_LDS>(p);
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
	const int NB = T / PL_RENORM + 1, BN = B * N, ls = 2 * L_max + 2, lh = L_max + 1;
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
			const float* oa = offs + ((int64_t)bn * NB + (t >> PL_RENORM_LOG2)) * lh;
			const float* ob = offs + (((int64_t)BN + bn) * NB + ((Tb - 1 - t) >> PL_RENORM_LOG2)) * lh;
			const float ti = tot[4 * bn], tr = tot[4 * bn + 1];
			const int64_t* hy = hyps + (int64_t)bn * L_max;
			for (int s = lane; s < L; s += 64) {
				int d = blank;
				if (s & 1) {
					const int64_t y = hy[s >> 1];
					d = (y >= 0 && y < C) ? (int)y : -1;
				}
				if (d < 0) continue;
				const float shift = pl_posterior_shift(oa[s >> 1], ob[s >> 1], ti, tr);
				const float ab = ar[s] + br[s];
				atomicAdd(mybins + d, wn * pl_exp2(ab + (shift - log2_floor(row[d] * LOG2_E))));
			}
			__builtin_amdgcn_s_waitcnt(0xc07f);
			__builtin_amdgcn_wave_barrier();
		}
		for (int c = lane; c < C; c += 64) grow[c] = mybins[c];
		__builtin_amdgcn_wave_barrier();
	}
}

// threads of a lattice: 2 L_max + 1 states; -1 beyond MW_MAX_LABELS
static int mw_cap(int L_max) { return pl_cap(2 * (int64_t)L_max + 1); }

extern "C" int convasr_mwer_states_per_wave(void) { return PL_WAVE_STATES; }
extern "C" int convasr_mwer_renorm_frames(void) { return PL_RENORM; }
extern "C" int convasr_mwer_max_labels(void) { return MW_MAX_LABELS; }
extern "C" int convasr_mwer_max_hyps(void) { return MW_MAX_HYPS; }

extern "C" int convasr_mwer_supported(int B, int N, int T, int C, int L_max) {
	return (B > 0 && B <= 65535 && N > 0 && N <= MW_MAX_HYPS && T > 0 && T <= PL_MAX_T && C > 1 && C <= PL_MAX_C && mw_cap(L_max) > 0) ? 1 : 0;
}

#define MW_ENVELOPE "outside the envelope (B <= 65535, N <= %d hypotheses, T <= %d, C <= %d, L_max <= %d labels: %d states)"

extern "C" int64_t convasr_mwer_workspace_bytes(int B, int N, int T, int C, int L_max) {
	if (!convasr_mwer_supported(B, N, T, C, L_max)) return convasr_fail(CONVASR_EUNSUPPORTED, "mwer_workspace_bytes: B %d, N %d, T %d, C %d, L_max %d " MW_ENVELOPE, B, N, T, C, L_max, MW_MAX_HYPS, PL_MAX_T, PL_MAX_C, MW_MAX_LABELS, PL_MAX_STATES - 1);
	const int64_t BN = (int64_t)B * N, ls = 2 * (int64_t)L_max + 2, NB = T / PL_RENORM + 1;
	return (2 * BN * T * ls + BN * NB * ls + 4 * BN + BN) * 4;
}

extern "C" int convasr_mwer_loss(const float* log_probs, const int64_t* hyps, const int64_t* hyp_lengths, const int64_t* olen, const float* risk, float scale,
                                 float* loss, float* grad, float* hyp_nll, float* hyp_posterior, void* workspace,
                                 int B, int N, int T, int C, int L_max, int blank, void* stream) {
	CONVASR_CHECK_ARG(log_probs && hyp_lengths && olen && risk && loss && hyp_nll && hyp_posterior && workspace && (hyps || L_max == 0) && B > 0 && N > 0 && T > 0 && C > 1 && L_max >= 0 && blank >= 0 && blank < C, "mwer_loss: bad arguments");
	CONVASR_CHECK_ARG(scale > 0.f && scale < INFINITY, "mwer_loss: scale %g must be a finite number > 0", (double)scale);
	if (!convasr_mwer_supported(B, N, T, C, L_max)) return convasr_fail(CONVASR_EUNSUPPORTED, "mwer_loss: B %d, N %d, T %d, C %d, L_max %d " MW_ENVELOPE, B, N, T, C, L_max, MW_MAX_HYPS, PL_MAX_T, PL_MAX_C, MW_MAX_LABELS, PL_MAX_STATES - 1);
	hipStream_t s = (hipStream_t)stream;
	const int cap = mw_cap(L_max), NB = T / PL_RENORM + 1, BN = B * N;
	float* alpha = (float*)workspace;
	const int64_t ls = 2 * (int64_t)L_max + 2;   // a lattice row: the 2 L_max + 1 states, made even
	float* beta = alpha + (int64_t)BN * T * ls;
	float* offs = beta + (int64_t)BN * T * ls;
	float* tot = offs + (int64_t)BN * NB * ls;
	float* w = tot + 4 * (int64_t)BN;
	pl_launch<mwer_alpha_beta_kernel<true>, mwer_alpha_beta_kernel<false>>(BN, cap, (size_t)mw_lds_words(cap) * 4, T, C, s,
		log_probs, hyps, hyp_lengths, olen, hyp_nll, alpha, beta, offs, tot, BN, N, T, C, L_max, blank, cap);
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
