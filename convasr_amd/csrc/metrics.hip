// Validation metrics on the device: the edit distances behind the reference's metrics.cer / metrics.wer (metrics.py:409-421) and the
// greedy CTC collapse of GreedyCTCGenerator.generate (transcript_generators.py).  The semantics are normative in include/convasr_hip.h
// and restated in Python by tests/_metrics_ref.py.
//
// convasr_edit_distance: one wave (one 64-thread workgroup) per (utterance, hypothesis) pair; no workspace, the staging is in LDS.
//   1. Units: the positions of the units of the hypothesis and of the reference are compacted by ballot + mbcnt (CHARS: the tokens that
//      are not the space; WORDS: the first token and the length of every maximal run of non-space tokens).
//   2. Ids: every reference unit gets the index of the first reference unit equal to it, every hypothesis unit the index of the first
//      reference unit equal to it or 0xFFFF.  The search compares a 16-bit hash first and confirms a hash hit token by token against the
//      tokens in global memory, so equal ids mean equal units, exactly.
//   3. Distance: the Levenshtein row DP over the ids, the reference on the outer (row) axis.  With E[j] = min(D[i-1][j] + 1,
//      D[i-1][j-1] + (r_i != h_j)) and E[0] = i, the row is D[i][j] = j + min_{k <= j} (E[k] - k): the left-to-right dependency is a
//      prefix minimum, taken 64 columns at a time across the wave (a DPP scan: four row shifts, two row broadcasts) with the running
//      minimum carried between chunks.  Up to ED_REG_CHUNKS x 64 = 1,024 hypothesis units the row and the hypothesis ids stay in
//      registers (ed_dp_regs<R>, R chunks of 64 columns per lane, the smallest R of 1, 2, 4, 8, 12, 16 that holds the row): the R scans
//      of a row do not depend on each other, only the carried minimum does, so they overlap.  Longer hypotheses keep the row in LDS as
//      uint16 (a distance is at most 16,383), one chunk after the other; a lane only reads and writes its own column of it, the diagonal
//      neighbour arrives by a DPP shift.
//   LDS (uint16 entries): hypothesis units Lh + 2, reference units Lr + 2, reference hashes then the DP row max(Lr, Lh + 1) + 2,
//   reference ids Lr + 2 -- at most 131,104 bytes at Lh = Lr = 16,383, 4 KB at 750 x 250.
//
// convasr_ctc_greedy_collapse: one workgroup per utterance.  The path is staged through LDS in chunks of GC_CHUNK frames by all threads;
// thread 0 walks the chunk through the collapse rules and leaves the tokens it emits in LDS; all threads write them out.
#include "common.h"

namespace {

constexpr int ED_THREADS = 64;
constexpr int ED_BIG = 1 << 20;
constexpr uint16_t ED_NO_MATCH = 0xFFFF;
constexpr int ED_REG_CHUNKS = 16;
constexpr int GC_THREADS = 256;
constexpr int GC_CHUNK = 1024;

__device__ __forceinline__ uint64_t ed_mix(uint64_t x) {
	x ^= x >> 33;
	x *= 0xff51afd7ed558ccdull;
	x ^= x >> 33;
	x *= 0xc4ceb9fe1a85ec53ull;
	x ^= x >> 33;
	return x;
}

// The row DP with the row in registers: lane l holds columns j = 1 + 64 c + l, c < R (column 0 is i).  hid: hypothesis ids (LDS),
// rid: reference ids (LDS); 1 <= nh <= 64 R, nr >= 1.  Columns past nh compute garbage that no valid column reads: a valid column's
// diagonal comes from the column before it, also valid.
template <int R>
__device__ int ed_dp_regs(const uint16_t* hid, const uint16_t* rid, int nh, int nr) {
	const int lane = threadIdx.x;
	int up[R], id[R];
#pragma unroll
	for (int c = 0; c < R; ++c) {
		const int j = 1 + ED_THREADS * c + lane;
		up[c] = j;
		id[c] = j <= nh ? hid[j - 1] : -1;
	}
	for (int i = 1; i <= nr; ++i) {
		const int r = rid[i - 1];
		int x[R];
#pragma unroll
		for (int c = 0; c < R; ++c) {  // independent scans: D[i-1] is all they read
			const int j = 1 + ED_THREADS * c + lane;
			const int diag = wave_dpp<0x138>(c == 0 ? i - 1 : __builtin_amdgcn_readlane(up[c - 1], ED_THREADS - 1), up[c]);
			x[c] = wave_prefix_min(j <= nh ? min(up[c] + 1, diag + (id[c] != r)) - j : ED_BIG, ED_BIG);
		}
		int run = i;
#pragma unroll
		for (int c = 0; c < R; ++c) {
			const int v = min(x[c], run);
			run = __builtin_amdgcn_readlane(v, ED_THREADS - 1);
			up[c] = v + 1 + ED_THREADS * c + lane;
		}
	}
	const int last = (nh - 1) / ED_THREADS;
	int d = 0;
#pragma unroll
	for (int c = 0; c < R; ++c)
		if (c == last) d = up[c];
	return __shfl(d, (nh - 1) % ED_THREADS);
}

// Compacts the units of tok[0, L).  CHARS: pos[u] = position of unit u.  WORDS: pos[w] = first token of word w, len[w] = its length.
// Returns the number of units (uniform across the wave).
__device__ int ed_units(const int64_t* __restrict__ tok, int L, int mode, int64_t space, uint16_t* pos, uint16_t* len) {
	const int lane = threadIdx.x;
	const bool all = space < 0;
	int n_start = 0, n_end = 0;
	for (int base = 0; base < L; base += ED_THREADS) {
		const int t = base + lane;
		const bool unit = t < L && (all || tok[t] != space);
		if (mode == CONVASR_METRIC_CHARS) {
			const uint64_t m = __ballot(unit);
			if (unit) pos[n_start + lane_rank(m)] = (uint16_t)t;
			n_start += __popcll(m);
			continue;
		}
		int prev = __shfl_up((int)unit, 1), next = __shfl_down((int)unit, 1);
		if (lane == 0) prev = t > 0 && t - 1 < L && tok[t - 1] != space;
		if (lane == ED_THREADS - 1) next = t + 1 < L && tok[t + 1] != space;
		const bool first = unit && !prev, last = unit && !next;
		const uint64_t ms = __ballot(first), me = __ballot(last);
		if (first) pos[n_start + lane_rank(ms)] = (uint16_t)t;
		if (last) len[n_end + lane_rank(me)] = (uint16_t)t;  // the last token for now; made a length below
		n_start += __popcll(ms);
		n_end += __popcll(me);
	}
	if (mode == CONVASR_METRIC_WORDS) {
		__syncthreads();
		for (int w = lane; w < n_start; w += ED_THREADS) len[w] = (uint16_t)(len[w] - pos[w] + 1);
	}
	return n_start;
}

__device__ __forceinline__ uint16_t ed_hash(const int64_t* __restrict__ tok, int p, int n) {
	uint64_t h = ed_mix((uint64_t)n + 0x9e3779b97f4a7c15ull);
	for (int k = 0; k < n; ++k) h = ed_mix(h ^ (uint64_t)tok[p + k]);
	return (uint16_t)(h ^ (h >> 16) ^ (h >> 32) ^ (h >> 48));
}

__device__ __forceinline__ bool ed_same(const int64_t* __restrict__ a, int pa, const int64_t* __restrict__ b, int pb, int n) {
	for (int k = 0; k < n; ++k)
		if (a[pa + k] != b[pb + k]) return false;
	return true;
}

__global__ __launch_bounds__(ED_THREADS) void edit_distance_kernel(const int64_t* __restrict__ hyp, const int64_t* __restrict__ hyp_lengths,
                                                                   const int64_t* __restrict__ ref, int64_t ref_stride,
                                                                   const int64_t* __restrict__ ref_lengths, int64_t ref_lengths_stride,
                                                                   int32_t* __restrict__ distance, int32_t* __restrict__ ref_units, int K,
                                                                   int Lh, int Lr, int mode, int64_t space, int nA, int nB, int nC) {
	extern __shared__ __align__(16) uint16_t ed_smem[];
	const int lane = threadIdx.x;
	const int pair = blockIdx.x, b = pair / K, k = pair - b * K;
	const int64_t* h = hyp + (int64_t)pair * Lh;
	const int64_t* r = ref + (int64_t)b * ref_stride;
	const int lh = clamp_len(hyp_lengths[pair], Lh);
	const int lr = clamp_len(ref_lengths[(int64_t)b * ref_lengths_stride], Lr);
	const bool words = mode == CONVASR_METRIC_WORDS;
	uint16_t* A = ed_smem;   // hypothesis unit positions (WORDS: lengths in the upper half), then hypothesis ids
	uint16_t* Bp = A + nA;   // reference unit positions (WORDS: lengths in the upper half)
	uint16_t* C = Bp + nB;   // reference hashes, then the DP row
	uint16_t* D = C + nC;    // reference ids
	uint16_t* hlen = A + nA / 2;
	uint16_t* rlen = Bp + nB / 2;

	const int nh = ed_units(h, lh, mode, space, A, hlen);
	const int nr = ed_units(r, lr, mode, space, Bp, rlen);
	__syncthreads();
	for (int u = lane; u < nr; u += ED_THREADS) C[u] = ed_hash(r, Bp[u], words ? rlen[u] : 1);
	__syncthreads();
	for (int u = lane; u < nr; u += ED_THREADS) {
		const uint16_t hu = C[u];
		const int pu = Bp[u], lu = words ? rlen[u] : 1;
		int id = u;
		for (int q = 0; q < u; ++q)
			if (C[q] == hu && (!words || rlen[q] == lu) && ed_same(r, Bp[q], r, pu, lu)) { id = q; break; }
		D[u] = (uint16_t)id;
	}
	for (int u = lane; u < nh; u += ED_THREADS) {
		const int pu = A[u], lu = words ? hlen[u] : 1;
		const uint16_t hu = ed_hash(h, pu, lu);
		uint16_t id = ED_NO_MATCH;
		for (int q = 0; q < nr; ++q)
			if (C[q] == hu && (!words || rlen[q] == lu) && ed_same(r, Bp[q], h, pu, lu)) { id = (uint16_t)q; break; }
		A[u] = id;  // (only this lane reads A[u] / hlen[u])
	}
	__syncthreads();

	int dist;
	const int chunks = (nh + ED_THREADS - 1) / ED_THREADS;
	if (nh == 0 || nr == 0) {
		dist = nh + nr;
	} else if (chunks <= ED_REG_CHUNKS) {
		dist = chunks <= 1 ? ed_dp_regs<1>(A, D, nh, nr) : chunks <= 2 ? ed_dp_regs<2>(A, D, nh, nr) : chunks <= 4 ? ed_dp_regs<4>(A, D, nh, nr)
		     : chunks <= 8 ? ed_dp_regs<8>(A, D, nh, nr) : chunks <= 12 ? ed_dp_regs<12>(A, D, nh, nr) : ed_dp_regs<ED_REG_CHUNKS>(A, D, nh, nr);
	} else {
		uint16_t* row = C;
		for (int j = lane; j <= nh; j += ED_THREADS) row[j] = (uint16_t)j;
		__syncthreads();
		for (int i = 1; i <= nr; ++i) {
			const int rid = D[i - 1];
			int diag_carry = i - 1;  // D[i-1][base - 1]
			int run = i;             // min_{k < base} (E[k] - k), E[0] = i
			for (int base = 1; base <= nh; base += ED_THREADS) {
				const int j = base + lane;
				const bool v = j <= nh;
				const int up = v ? row[j] : ED_BIG;
				const int diag = wave_dpp<0x138>(diag_carry, up);  // wave_shr:1, lane 0 <- D[i-1][base - 1]
				diag_carry = __builtin_amdgcn_readlane(up, ED_THREADS - 1);
				const int x = min(wave_prefix_min(v ? min(up + 1, diag + (A[j - 1] != rid)) - j : ED_BIG, ED_BIG), run);
				if (v) row[j] = (uint16_t)(x + j);
				run = __builtin_amdgcn_readlane(x, ED_THREADS - 1);
			}
		}
		__syncthreads();
		dist = row[nh];
	}
	if (lane == 0) {
		distance[pair] = dist;
		if (k == 0) ref_units[b] = nr;
	}
}

__global__ __launch_bounds__(GC_THREADS) void ctc_greedy_collapse_kernel(const int64_t* __restrict__ path, const int64_t* __restrict__ lengths,
                                                                         int64_t* __restrict__ tokens, int64_t* __restrict__ out_lengths, int T,
                                                                         int64_t eps, int64_t space, int blank_amount_to_space) {
	__shared__ int64_t s_in[GC_CHUNK];
	__shared__ int64_t s_out[GC_CHUNK];
	__shared__ int s_n;
	const int b = blockIdx.x;
	const int64_t* p = path + (int64_t)b * T;
	int64_t* out = tokens + (int64_t)b * T;
	const int n = clamp_len(lengths[b], T);
	// the walk's state, thread 0 only: the last token emitted (eps before the first), blanks seen since, whether a blank allows a repeat
	int64_t last = eps;
	int blanks = 0;
	bool repeat_ok = false, started = false;
	int total = 0;
	for (int base = 0; base < n; base += GC_CHUNK) {
		const int m = min(GC_CHUNK, n - base);
		for (int t = threadIdx.x; t < m; t += GC_THREADS) s_in[t] = p[base + t];
		__syncthreads();
		if (threadIdx.x == 0) {
			int e = 0;
			for (int t = 0; t < m; ++t) {
				const int64_t c = s_in[t];
				if (!started) {
					if (c == eps || c == space) continue;
					started = true;
				}
				if (c == eps) {
					if (last == space) continue;
					repeat_ok = true;
					if (++blanks >= blank_amount_to_space) s_out[e++] = last = space;
					continue;
				}
				if (c == last && !repeat_ok) continue;
				repeat_ok = false;
				s_out[e++] = last = c;
				blanks = 0;
			}
			s_n = e;
		}
		__syncthreads();
		const int e = s_n;
		for (int t = threadIdx.x; t < e; t += GC_THREADS) out[total + t] = s_out[t];
		total += e;
		__syncthreads();  // s_in, s_out and s_n are refilled by the next chunk
	}
	for (int t = total + threadIdx.x; t < T; t += GC_THREADS) out[t] = 0;
	if (threadIdx.x == 0) out_lengths[b] = total;
}

inline int ed_region(int n) { return (n + 3) & ~3; }  // uint16 entries, rounded to 8 bytes

}  // namespace

extern "C" int convasr_edit_distance(const int64_t* hyp, const int64_t* hyp_lengths, const int64_t* ref, int64_t ref_stride,
                                     const int64_t* ref_lengths, int64_t ref_lengths_stride, int32_t* distance, int32_t* ref_units, int B,
                                     int K, int Lh, int Lr, int mode, int64_t space, void* stream) {
	CONVASR_CHECK_ARG(hyp && hyp_lengths && ref && ref_lengths && distance && ref_units, "edit_distance: NULL pointer");
	CONVASR_CHECK_ARG(B >= 1 && K >= 1, "edit_distance: B %d and K %d must be >= 1", B, K);
	CONVASR_CHECK_ARG((int64_t)B * K < (1 << 20), "edit_distance: B * K = %lld pairs, at most 2^20 - 1", (long long)B * K);
	CONVASR_CHECK_ARG(Lh >= 0 && Lh <= CONVASR_METRIC_MAX_LEN && Lr >= 0 && Lr <= CONVASR_METRIC_MAX_LEN,
	                  "edit_distance: Lh %d and Lr %d must be in [0, %d]", Lh, Lr, CONVASR_METRIC_MAX_LEN);
	CONVASR_CHECK_ARG(ref_stride >= 0 && ref_lengths_stride >= 0, "edit_distance: negative stride (%lld, %lld)", (long long)ref_stride,
	                  (long long)ref_lengths_stride);
	CONVASR_CHECK_ARG(mode == CONVASR_METRIC_CHARS || mode == CONVASR_METRIC_WORDS, "edit_distance: mode %d is neither CHARS (0) nor WORDS (1)", mode);
	CONVASR_CHECK_ARG(mode != CONVASR_METRIC_WORDS || space >= 0, "edit_distance: WORDS mode needs a space token >= 0 (got %lld)", (long long)space);
	const int nA = ed_region(Lh + 2), nB = ed_region(Lr + 2), nC = ed_region(max(Lr, Lh + 1) + 2), nD = ed_region(Lr + 2);
	const size_t lds = 2 * (size_t)(nA + nB + nC + nD);
	static unsigned long long set = 0;
	convasr_allow_160k_lds(reinterpret_cast<const void*>(edit_distance_kernel), set);
	hipLaunchKernelGGL(edit_distance_kernel, dim3(B * K), dim3(ED_THREADS), lds, (hipStream_t)stream, hyp, hyp_lengths, ref, ref_stride,
	                   ref_lengths, ref_lengths_stride, distance, ref_units, K, Lh, Lr, mode, space, nA, nB, nC);
	CONVASR_CHECK_LAUNCH("edit_distance");
	return 0;
}

extern "C" int convasr_ctc_greedy_collapse(const int64_t* path, const int64_t* lengths, int64_t* tokens, int64_t* out_lengths, int B, int T,
                                           int eps, int space, int blank_amount_to_space, void* stream) {
	CONVASR_CHECK_ARG(path && lengths && tokens && out_lengths, "ctc_greedy_collapse: NULL pointer");
	CONVASR_CHECK_ARG(B >= 1 && T >= 1, "ctc_greedy_collapse: B %d and T %d must be >= 1", B, T);
	CONVASR_CHECK_ARG((int64_t)B * T < (1ll << 31), "ctc_greedy_collapse: B * T = %lld, at most 2^31 - 1", (long long)B * T);
	CONVASR_CHECK_ARG(eps >= 0 && space >= 0 && eps != space, "ctc_greedy_collapse: eps %d and space %d must be distinct and >= 0", eps, space);
	CONVASR_CHECK_ARG(blank_amount_to_space >= 0, "ctc_greedy_collapse: blank_amount_to_space %d < 0", blank_amount_to_space);
	hipLaunchKernelGGL(ctc_greedy_collapse_kernel, dim3(B), dim3(GC_THREADS), 0, (hipStream_t)stream, path, lengths, tokens, out_lengths, T,
	                   (int64_t)eps, (int64_t)space, blank_amount_to_space);
	CONVASR_CHECK_LAUNCH("ctc_greedy_collapse");
	return 0;
}
