// CTC loss and gradient (F.ctc_loss at models.py:323) for whole recordings, on many CUs: convasr_ctc_loss_long.  The kernel of csrc/ctc.hip
// runs one workgroup per utterance and stops at 1,023 labels (16 label pairs per lane) and ~12,000 frames (its per-frame hand-over
// slots live in LDS); ten minutes of speech are ~30,000 frames against ~9,000 labels = ~18,000 states.
//
// The alpha-beta recursion is that of ctc.hip -- fp32 log-sum-exp in base 2, the finite sentinel LOG2_NEG for "impossible", a -inf
// log-prob staged as the sentinel -- cut like csrc/align_long.hip cuts the alignment: tiles of CL_SB consecutive states (a "block") x
// `chunk` consecutive frames, one wave per tile, lane l owning states s0 + 4 l .. s0 + 4 l + 3.  An alpha tile depends on the tile before
// it in time (the carried column), on the tile of the block to its left and on the one diagonally before-left (the last state of the left
// block at the frame before: a block starts on a blank, which never takes the s-2 move); a beta tile is the mirror image (the first two
// states of the right block at the frame after).  Tiles on one anti-diagonal are independent: launch k of a plain sequence of launches
// runs the k-th anti-diagonal of BOTH sweeps (alpha tiles first in the grid, then beta tiles).  Every value a tile reads from another
// tile was written by an earlier launch; nothing waits, spins or polls inside a launch.
//
// Both lattices are stored whole, [B][T][blocks * CL_SB] fp32 each: the carried column and the neighbour's edge states are rows of the
// lattice itself.  A long lattice cannot be carried unnormalised (values grow like 3 T and fp32 loses the gradient): at every frame
// whose ABSOLUTE index is a multiple of CL_RENORM a block subtracts floor(max over its states), an integer in the log2 domain, so that the
// subtraction, the running sum of the offsets and the conversion of a neighbour's edge states are exact in fp32.  The running sum is
// published per block and FRAME beside the lattice ([B][blocks][T], 1/256 of a lattice), true log2 alpha(t, s) = lattice + offset: since
// the period is keyed on the frame index and the offsets on the block, no value depends on the chunk length.
//
// Unreachable states: alpha(t, s) with s > 2t + 1 and beta(t, s) with L - 1 - s > 2 (olen - 1 - t) + 1 are exactly the sentinel (it
// absorbs every finite score and offset).  Alpha tiles wholly inside that region are not launched; beta's region depends on the
// utterance's own olen and ylen, which live on the device, so a beta tile wholly inside it ends at its first instruction.  Every read
// of a lattice value or an offset that such a tile would have written substitutes the sentinel / 0 under the same per-state test, so a
// result never depends on how the lattice was cut.
//
// Gradient: one wave per frame reduces exp2(alpha + beta - total - lp) over the states that both sweeps reach into LDS bins per class
// (ctc_grad_kernel's arithmetic with per-block offsets), grad = exp(lp) - posterior for t < olen, 0 beyond.  No atomics on global memory.
#include "common.h"
#include "log2_domain.h"

#define CL_RENORM 8                   // frames between renormalisations (a power of two), as in ctc.hip
#define CL_NS 4                       // states per lane (even: a lane starts on a blank)
#define CL_SB (64 * CL_NS)            // states per block
#define CL_CHUNK_DEFAULT 256
#define CL_CHUNK_MIN 16
#define CL_CHUNK_MAX 4096
#define CL_MAX_LABELS 131071
#define CL_MAX_FRAMES (1 << 20)
#define CL_MAX_CLASSES 8192
#define CL_MAX_BATCH 65535            // grid.y

// base-2 log-sum-exp of two values >= the sentinel (lse3_med3's companion: the largest term is exp2(0) = 1 exactly)
__device__ __forceinline__ float cl_lse2(float a, float b) {
	const float m = fmaxf(a, b);
	return m + __builtin_amdgcn_logf(1.f + __builtin_amdgcn_exp2f(fminf(a, b) - m));
}

struct ClSweep {
	const float* lp;
	const int64_t *targets, *olen, *ylen;
	float *alpha, *beta, *off_a, *off_b, *nan_flag;
	int T, C, S_max, blank, chunk, nblocks, nchunks, LP;
};

// beta(t, s) of an utterance with L states and Tb frames is impossible (or s is no state at all)
__device__ __forceinline__ bool cl_dead_b(int64_t s, int64_t t, int L, int Tb) { return s >= L || (int64_t)L - 1 - s > 2 * ((int64_t)Tb - 1 - t) + 1; }

template <bool FWD>
__device__ __forceinline__ void cl_tile(const ClSweep& q, int j, int c, int b) {
	constexpr int NS = CL_NS;
	const int lane = threadIdx.x, T = q.T, C = q.C, LP = q.LP;
	const int Tb = (int)q.olen[b], S = (int)q.ylen[b], L = 2 * S + 1;
	if (Tb <= 0 || Tb > T || S < 0 || S > q.S_max) return;
	const int s0 = j * CL_SB;
	if (s0 >= L) return;  // no state of the utterance in this block, and no block that is read reads from it
	const int t_begin = c * q.chunk, t_end = min(Tb, t_begin + q.chunk);
	if (t_begin >= Tb) return;
	const int s_hi = min(s0 + CL_SB, L) - 1;
	if (FWD ? (int64_t)s0 > 2 * ((int64_t)t_end - 1) + 1 : cl_dead_b(s_hi, t_begin, L, Tb)) return;  // every state impossible at every frame of the tile
	const int64_t* tg = q.targets + (int64_t)b * q.S_max;
	const float* lpb = q.lp + (int64_t)b * T * C;
	float* lat = (FWD ? q.alpha : q.beta) + (int64_t)b * T * LP;
	float* off = (FWD ? q.off_a : q.off_b) + ((int64_t)b * q.nblocks + j) * T;
	const float* offn = off + (FWD ? -(int64_t)T : (int64_t)T);  // the neighbouring block's (dereferenced only where that block has reachable states)
	const int sl = s0 + lane * NS;

	int cls[NS];
	bool skip[NS], valid[NS];
#pragma unroll
	for (int i = 0; i < NS; ++i) {
		const int s = sl + i;
		valid[i] = s < L;
		bool lab = (i & 1) && valid[i];
		int k = lab ? (int)tg[s >> 1] : q.blank;
		if ((unsigned)k >= (unsigned)C) { k = q.blank; valid[i] = false; lab = false; }  // a label that is no class: the state is impossible
		cls[i] = k;
		// a label state may take the s-2 (alpha) / s+2 (beta) move when its neighbour label differs
		skip[i] = lab && (FWD ? (s >= 3 && tg[s >> 1] != tg[(s >> 1) - 1]) : (s + 2 < L && tg[s >> 1] != tg[(s >> 1) + 1]));
	}
	bool saw_nan = false;
	auto score = [&](float v, int i) {
		if (!valid[i]) return LOG2_NEG;
		saw_nan |= v != v;
		v *= LOG2_E;
		return log2_floor(v);
	};
	float a[NS], r[NS], cum;
	// renormalise at the frames the absolute index names, then store the frame's states and the block's running offset
	auto finish = [&](int t) {
		if ((t & (CL_RENORM - 1)) == 0) {
			float m = fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3]));
			m = wave_max(m);
			if (m > LOG2_DEAD && m < INFINITY) {
				const float kk = floorf(m);
#pragma unroll
				for (int i = 0; i < NS; ++i) a[i] -= kk;
				cum += kk;
			}
		}
		*reinterpret_cast<float4*>(lat + (int64_t)t * LP + sl) = make_float4(a[0], a[1], a[2], a[3]);
		if (lane == 0) off[t] = cum;
	};
	int t;
	const int t_first = FWD ? 0 : Tb - 1;
	if (FWD ? c == 0 : t_end == Tb) {
		const float* row = lpb + (int64_t)t_first * C;
#pragma unroll
		for (int i = 0; i < NS; ++i) a[i] = (FWD ? sl + i < 2 : sl + i >= L - 2) ? score(row[cls[i]], i) : LOG2_NEG;
		cum = 0.f;
		finish(t_first);
		t = FWD ? 1 : Tb - 2;
	} else {
		const int64_t tc = FWD ? t_begin - 1 : t_end;  // the carried column's frame
		const float4 v = *reinterpret_cast<const float4*>(lat + tc * LP + sl);  // (inside the workspace whether or not it was written)
		const float vv[NS] = {v.x, v.y, v.z, v.w};
#pragma unroll
		for (int i = 0; i < NS; ++i) a[i] = (FWD ? (int64_t)(sl + i) > 2 * tc + 1 : cl_dead_b(sl + i, tc, L, Tb)) ? LOG2_NEG : vv[i];
		cum = (FWD ? (int64_t)s0 > 2 * tc + 1 : cl_dead_b(s_hi, tc, L, Tb)) ? 0.f : off[tc];  // (the tile that would have written it did not run)
		t = FWD ? t_begin : t_end - 1;
	}
	const int dt = FWD ? 1 : -1;
	const int n_left = FWD ? t_end - t : t - t_begin + 1;  // frames still to do
	if (n_left > 0) {
		const float* row = lpb + (int64_t)t * C;
#pragma unroll
		for (int i = 0; i < NS; ++i) r[i] = score(row[cls[i]], i);
	}
	for (int done = 0; done < n_left; done += 64) {
		// lane l fetches what the edge lane needs at this batch's l-th frame: the neighbouring block's edge state(s) at the frame before it in the sweep
		float q0 = LOG2_NEG, q1 = LOG2_NEG, qo = 0.f;
		const int n_here = min(64, n_left - done);
		if (lane < n_here) {
			const int64_t tp = (int64_t)t + dt * lane - dt;
			if (FWD) {
				if (j > 0 && (int64_t)s0 - 1 <= 2 * tp + 1) { q0 = lat[tp * LP + s0 - 1]; qo = offn[tp]; }
			} else {
				const bool d0 = cl_dead_b(s0 + CL_SB, tp, L, Tb), d1 = cl_dead_b(s0 + CL_SB + 1, tp, L, Tb);
				if (!d0 || !d1) qo = offn[tp];  // (the higher state is reached first, unless it is past the utterance's last)
				if (!d0) q0 = lat[tp * LP + s0 + CL_SB];
				if (!d1) q1 = lat[tp * LP + s0 + CL_SB + 1];
			}
		}
		for (int ii = 0; ii < n_here; ++ii, t += dt) {
			float rn[NS];  // the next frame's log-probs, in flight while this frame is computed
			const float* row = lpb + (int64_t)min(max(t + dt, 0), Tb - 1) * C;
#pragma unroll
			for (int i = 0; i < NS; ++i) rn[i] = row[cls[i]];
			const float d = __shfl(qo, ii, 64) - cum;  // integer-valued: exact
			float n[NS];
			if (FWD) {
				float p1 = __shfl_up(a[NS - 1], 1, 64);  // state sl - 1
				const float e0 = __shfl(q0, ii, 64) + d;
				if (lane == 0) p1 = e0;
				n[0] = cl_lse2(a[0], p1) + r[0];
				n[1] = lse3_med3(a[1], a[0], skip[1] ? p1 : LOG2_NEG) + r[1];
				n[2] = cl_lse2(a[2], a[1]) + r[2];
				n[3] = lse3_med3(a[3], a[2], skip[3] ? a[1] : LOG2_NEG) + r[3];
			} else {
				float p0 = __shfl_down(a[0], 1, 64), p1 = __shfl_down(a[1], 1, 64);  // states sl + NS, sl + NS + 1
				const float e0 = __shfl(q0, ii, 64) + d, e1 = __shfl(q1, ii, 64) + d;
				if (lane == 63) { p0 = e0; p1 = e1; }
				n[0] = cl_lse2(a[0], a[1]) + r[0];
				n[1] = lse3_med3(a[1], a[2], skip[1] ? a[3] : LOG2_NEG) + r[1];
				n[2] = cl_lse2(a[2], a[3]) + r[2];
				n[3] = lse3_med3(a[3], p0, skip[3] ? p1 : LOG2_NEG) + r[3];
			}
#pragma unroll
			for (int i = 0; i < NS; ++i) a[i] = n[i];
			finish(t);
#pragma unroll
			for (int i = 0; i < NS; ++i) r[i] = score(rn[i], i);
		}
	}
	if (saw_nan) q.nan_flag[b] = 1.f;  // (every writer stores the same word)
}

// grid.x: the alpha tiles of anti-diagonal `diag` (blocks ja_lo .. ja_lo + na - 1), then the beta tiles of the mirrored one (nb of them)
__global__ __launch_bounds__(64) void ctc_long_sweep_kernel(ClSweep q, int diag, int ja_lo, int na, int jb_lo) {
	const int x = blockIdx.x, b = blockIdx.y;
	if (x < na) {
		const int j = ja_lo + x;
		cl_tile<true>(q, j, diag - j, b);
	} else {
		const int jm = jb_lo + (x - na);  // counted from the last block; chunks from the last chunk
		cl_tile<false>(q, q.nblocks - 1 - jm, q.nchunks - 1 - (diag - jm), b);
	}
}

// one thread per utterance: nll and the {integer part, remainder} of the log2 likelihood from the alpha row at olen - 1
__global__ void ctc_long_total_kernel(ClSweep q, float* __restrict__ nll, float* __restrict__ tot, int B) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= B) return;
	const int Tb = (int)q.olen[b], S = (int)q.ylen[b], L = 2 * S + 1, T = q.T;
	tot[2 * b] = 0.f; tot[2 * b + 1] = 0.f;
	if (Tb <= 0 || Tb > T || S < 0 || S > q.S_max) { nll[b] = (Tb == 0 && S == 0) ? 0.f : INFINITY; return; }
	const float* row = q.alpha + ((int64_t)b * T + (Tb - 1)) * q.LP;
	const float* off = q.off_a + (int64_t)b * q.nblocks * T + (Tb - 1);
	const int64_t reach = 2 * ((int64_t)Tb - 1) + 1;
	float l1 = LOG2_NEG, l2 = LOG2_NEG, c1 = 0.f;
	if (L - 1 <= reach) { l1 = row[L - 1]; c1 = off[(int64_t)((L - 1) / CL_SB) * T]; }
	if (L >= 2 && L - 2 <= reach) l2 = row[L - 2] + (off[(int64_t)((L - 2) / CL_SB) * T] - c1);
	const float m = fmaxf(l1, l2);
	const float rem = m + log2f(exp2f(l1 - m) + exp2f(l2 - m));
	nll[b] = q.nan_flag[b] != 0.f ? NAN : (m > LOG2_DEAD ? (float)(-LOG2_LN2 * ((double)c1 + (double)rem)) : INFINITY);  // NaN log-probs: NaN (as the reference)
	tot[2 * b] = c1;
	tot[2 * b + 1] = rem;
}

__global__ __launch_bounds__(256) void ctc_long_grad_kernel(ClSweep q, const float* __restrict__ nll, const float* __restrict__ tot, float* __restrict__ grad, int t_per_block) {
	extern __shared__ float cl_bins[];  // [4][C]
	const int T = q.T, C = q.C, LP = q.LP, blank = q.blank;
	const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int Tb = (int)q.olen[b], S = (int)q.ylen[b], L = 2 * S + 1;
	const bool feasible = nll[b] < INFINITY && Tb > 0 && Tb <= T && S >= 0 && S <= q.S_max;
	const int64_t* tg = q.targets + (int64_t)b * q.S_max;
	float* mybins = cl_bins + wave * C;
	const int t_begin = blockIdx.x * t_per_block, t_end = min(T, t_begin + t_per_block);
	for (int t = t_begin + wave; t < t_end; t += 4) {
		const float* row = q.lp + ((int64_t)b * T + t) * C;
		float* grow = grad + ((int64_t)b * T + t) * C;
		if (t >= Tb || !feasible) {
			for (int c = lane; c < C; c += 64) grow[c] = 0.f;
			continue;
		}
		for (int c = lane; c < C; c += 64) mybins[c] = 0.f;
		__builtin_amdgcn_s_waitcnt(0xc07f);
		__builtin_amdgcn_wave_barrier();
		const float* ar = q.alpha + ((int64_t)b * T + t) * LP;
		const float* br = q.beta + ((int64_t)b * T + t) * LP;
		const float* oa = q.off_a + (int64_t)b * q.nblocks * T + t;
		const float* ob = q.off_b + (int64_t)b * q.nblocks * T + t;
		// alpha + beta - total = (lattice values - remainder of total) + (offsets - integer part of total): the second group is exact
		const float ti = tot[2 * b], tr = tot[2 * b + 1];
		const float lpb = row[blank] * LOG2_E;
		// the states both sweeps reach at this frame (the others hold the sentinel, or nothing at all): posterior 0
		const int64_t lo64 = (int64_t)L - 2 - 2 * ((int64_t)Tb - 1 - t), hi64 = 2 * (int64_t)t + 1;
		const int s_lo = lo64 > 0 ? (int)lo64 : 0, s_hi = hi64 < L - 1 ? (int)hi64 : L - 1;
		float blank_sum = 0.f;
		for (int s = s_lo + lane; s <= s_hi; s += 64) {
			const int64_t jb = (int64_t)(s / CL_SB) * T;
			const float shift = ((oa[jb] - ti) + ob[jb]) - tr;
			const float ab = ar[s] + br[s];
			if (s & 1) {
				const int c = (int)tg[s >> 1];
				if ((unsigned)c < (unsigned)C) atomicAdd(mybins + c, __builtin_amdgcn_exp2f(ab + (shift - row[c] * LOG2_E)));
			} else blank_sum += __builtin_amdgcn_exp2f(ab + (shift - lpb));
		}
		blank_sum = wave_sum(blank_sum);
		if (lane == 0) atomicAdd(mybins + blank, blank_sum);
		__builtin_amdgcn_s_waitcnt(0xc07f);
		__builtin_amdgcn_wave_barrier();
		for (int c = lane; c < C; c += 64) grow[c] = __expf(row[c]) - mybins[c];
		__builtin_amdgcn_wave_barrier();
	}
}

static int cl_chunk(int chunk_frames) { return chunk_frames == 0 ? CL_CHUNK_DEFAULT : chunk_frames; }

struct ClLayout { int nblocks, LP; int64_t alpha_off, beta_off, offa_off, offb_off, tot_off, flag_off, bytes; };
// (the envelope's far corner, 65,535 x 2^20 frames x 131,071 labels, is 2^57 bytes: no sum here leaves int64)
static void cl_layout(int B, int T, int S_max, ClLayout* y) {
	const int64_t Lmax = 2 * (int64_t)S_max + 1;
	y->nblocks = (int)ceil_div64(Lmax, CL_SB);
	y->LP = y->nblocks * CL_SB;
	const auto up = [](int64_t n) { return (n + 255) & ~(int64_t)255; };
	const int64_t lat_b = up((int64_t)B * T * y->LP * 4), off_b = up((int64_t)B * y->nblocks * T * 4);
	y->alpha_off = 0;
	y->beta_off = lat_b;
	y->offa_off = 2 * lat_b;
	y->offb_off = y->offa_off + off_b;
	y->tot_off = y->offb_off + off_b;
	y->flag_off = y->tot_off + up((int64_t)B * 8);
	y->bytes = y->flag_off + up((int64_t)B * 4);
}

static int cl_check(int B, int T, int C, int S_max) {
	if (B <= 0 || T <= 0 || C <= 1 || S_max < 0) return convasr_fail(CONVASR_EINVAL, "ctc_loss_long: bad arguments (B %d T %d C %d S_max %d)", B, T, C, S_max);
	if (S_max > CL_MAX_LABELS) return convasr_fail(CONVASR_EUNSUPPORTED, "ctc_loss_long: target length %d > %d", S_max, CL_MAX_LABELS);
	if (T > CL_MAX_FRAMES) return convasr_fail(CONVASR_EUNSUPPORTED, "ctc_loss_long: %d frames > %d", T, CL_MAX_FRAMES);
	if (C > CL_MAX_CLASSES) return convasr_fail(CONVASR_EUNSUPPORTED, "ctc_loss_long: C %d > %d", C, CL_MAX_CLASSES);
	if (B > CL_MAX_BATCH) return convasr_fail(CONVASR_EUNSUPPORTED, "ctc_loss_long: batch %d > %d", B, CL_MAX_BATCH);
	return 0;
}

extern "C" int convasr_ctc_loss_long_states_per_block(void) { return CL_SB; }
extern "C" int convasr_ctc_loss_long_chunk_frames(void) { return CL_CHUNK_DEFAULT; }

extern "C" int64_t convasr_ctc_loss_long_workspace_bytes(int B, int T, int C, int S_max) {
	if (const int e = cl_check(B, T, C, S_max)) return e;
	ClLayout y;
	cl_layout(B, T, S_max, &y);
	return y.bytes;
}

extern "C" int convasr_ctc_loss_long(const float* log_probs, const int64_t* targets, const int64_t* olen, const int64_t* ylen, float* nll, float* grad,
                                     void* workspace, int64_t workspace_bytes, int B, int T, int C, int S_max, int blank, int chunk_frames, void* stream) {
	CONVASR_CHECK_ARG(log_probs && targets && olen && ylen && nll && workspace && blank >= 0 && blank < C, "ctc_loss_long: bad arguments");
	if (const int e = cl_check(B, T, C, S_max)) return e;
	CONVASR_CHECK_ARG(chunk_frames == 0 || (chunk_frames >= CL_CHUNK_MIN && chunk_frames <= CL_CHUNK_MAX), "ctc_loss_long: chunk_frames %d is neither 0 nor in [%d, %d]", chunk_frames, CL_CHUNK_MIN, CL_CHUNK_MAX);
	ClLayout y;
	cl_layout(B, T, S_max, &y);
	CONVASR_CHECK_ARG(workspace_bytes >= y.bytes, "ctc_loss_long: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)y.bytes);
	CONVASR_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "ctc_loss_long: the workspace must be 16-byte aligned");
	hipStream_t s = (hipStream_t)stream;
	char* ws = (char*)workspace;
	float* tot = (float*)(ws + y.tot_off);
	const int64_t chunk = cl_chunk(chunk_frames), nchunks = ceil_div64(T, chunk), nblocks = y.nblocks;
	ClSweep q;
	q.lp = log_probs; q.targets = targets; q.olen = olen; q.ylen = ylen;
	q.alpha = (float*)(ws + y.alpha_off); q.beta = (float*)(ws + y.beta_off);
	q.off_a = (float*)(ws + y.offa_off); q.off_b = (float*)(ws + y.offb_off);
	q.nan_flag = (float*)(ws + y.flag_off);
	q.T = T; q.C = C; q.S_max = S_max; q.blank = blank; q.chunk = (int)chunk; q.nblocks = y.nblocks; q.nchunks = (int)nchunks; q.LP = y.LP;
	if (hipMemsetAsync(q.nan_flag, 0, (size_t)B * sizeof(float), s) != hipSuccess) return convasr_fail(CONVASR_ELAUNCH, "ctc_loss_long: clearing the NaN flags failed");
	for (int64_t k = 0; k < nchunks + nblocks - 1; ++k) {
		const int64_t j_lo = k - nchunks + 1 > 0 ? k - nchunks + 1 : 0;  // the same range of blocks for alpha and, counted from the far corner, for beta
		const int64_t j_hi = k < nblocks - 1 ? k : nblocks - 1;
		// alpha tile (chunk k - j, block j) lies wholly in s > 2t + 1 when j * CL_SB > 2 * ((k - j + 1) * chunk - 1) + 1: true from some j on
		const int64_t j_reach = (2 * (k + 1) * chunk - 1) / (CL_SB + 2 * chunk);
		const int64_t ja_hi = j_reach < j_hi ? j_reach : j_hi;
		const int64_t na = ja_hi >= j_lo ? ja_hi - j_lo + 1 : 0, nb = j_hi - j_lo + 1;
		hipLaunchKernelGGL(ctc_long_sweep_kernel, dim3((unsigned)(na + nb), (unsigned)B), dim3(64), 0, s, q, (int)k, (int)j_lo, (int)na, (int)j_lo);
	}
	CONVASR_CHECK_LAUNCH("ctc_loss_long (sweeps)");
	hipLaunchKernelGGL(ctc_long_total_kernel, dim3((unsigned)ceil_div64(B, 64)), dim3(64), 0, s, q, nll, tot, B);
	CONVASR_CHECK_LAUNCH("ctc_loss_long (total)");
	if (grad) {
		const int t_per_block = 32;
		const size_t smem = 4 * (size_t)C * sizeof(float);  // 128 KiB at C = 8192
		static unsigned long long set = 0;
		convasr_allow_160k_lds(reinterpret_cast<const void*>(ctc_long_grad_kernel), set);
		hipLaunchKernelGGL(ctc_long_grad_kernel, dim3((unsigned)ceil_div64(T, t_per_block), (unsigned)B), dim3(256), smem, s, q, nll, tot, grad, t_per_block);
		CONVASR_CHECK_LAUNCH("ctc_loss_long (gradient)");
	}
	return 0;
}
