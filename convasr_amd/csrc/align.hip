// Sequence alignment on the device: the semi-global Needleman-Wunsch alignment with traceback behind the reference's align_strings
// (metrics.py:365-407, its Needleman class at 447-645).  The semantics are normative in include/convasr_hip.h and restated in Python by
// tests/_align_ref.py.
//
// convasr_nw_align: one wave (one 64-thread workgroup) per pair, hypothesis units a on the rows, reference units b on the columns.
//   1. Fill.  With E[j] = max(M[i-1][j-1] + (a_i == b_j ? match : sub), M[i-1][j] + del) and E[0] = 0, the row is
//      M[i][j] = j * ins + max_{k <= j} (E[k] - k * ins): the left-to-right dependency is a prefix maximum, taken 64 columns at a time
//      across the wave (the DPP scan of metrics.hip with max for min) with the running maximum carried between chunks.  Up to
//      NW_REG_CHUNKS x 64 = 1,024 columns the row and the reference ids stay in registers (nw_fill_regs<R>, the smallest R of 1, 2, 4, 8,
//      16 that holds the row); longer references keep both in LDS as int32 (nw_fill_lds), a lane only ever touching its own columns.
//   2. Directions.  A cell's direction is decided when the cell is final, in the walk's priority: 0 = ins (M == left + ins), else
//      1 = del (M == up + del), else 2 = diagonal.  The left neighbour arrives by a DPP shift after the scan.  Two ballots per
//      64-column chunk pack the 2 bits per cell into two 64-bit words, which lane 0 writes to the workspace with one 16-byte vector store.
//   3. End cell.  The fill tracks max M[i][lb] per row (lowest row wins) and reduces the last row (lowest column wins); value and index
//      travel in one int64 key so that one max decides both.
//   4. Walk.  Lane 0's chain of dependent loads over the direction words (a word is reloaded only when the row or the chunk changes),
//      la + lb steps at most, the columns packed into the workspace in reverse; all lanes then write them out in forward order, with
//      the gap runs of the prefix and of the tail computed, not walked.
// Workspace per launch: N * La * ceil(Lb / 64) * 16 bytes of directions, then N * (La + Lb) * 4 bytes of reversed columns.
#include "common.h"

namespace {

constexpr int NW_THREADS = 64;
constexpr int NW_NEG = -(1 << 30);  // below every E[k] - k * ins the envelope allows (|.| < 2 * 16,383 * 32,768 + 32,768 < 2^30)
constexpr int NW_REG_CHUNKS = 16;
constexpr int NW_MAX_SCORE = 32768;

struct NwScores {
	int match, sub, del, ins;
};

// (value, index) as one key: the larger value wins, then the lower index
__device__ __forceinline__ long long nw_key(int value, int index) { return (long long)value * 65536 + (0xFFFF - index); }

// The part of a chunk after the scan, shared by both tiers: x = prefix max of E - j * ins over the chunk, run / left_carry = the running
// maximum and M[i][j0 - 1] carried from the chunk before.  Returns M[i][j] (0 in a column past lb) and stores the chunk's directions.
__device__ __forceinline__ int nw_finish_chunk(int x, int& run, int& left_carry, int up, int j, bool valid, NwScores s, uint64_t* dir_word) {
	const int v = max(x, run);
	run = __builtin_amdgcn_readlane(v, NW_THREADS - 1);
	const int m = valid ? v + j * s.ins : 0;
	const int left = wave_dpp<0x138>(left_carry, m);  // wave_shr:1, lane 0 <- M[i][j0 - 1]
	left_carry = __builtin_amdgcn_readlane(m, NW_THREADS - 1);
	const bool is_ins = m == left + s.ins;
	const bool is_del = !is_ins && m == up + s.del;
	const uint64_t lo = __ballot(valid && is_del), hi = __ballot(valid && !is_ins && !is_del);
	if (threadIdx.x == 0) *reinterpret_cast<ulonglong2*>(dir_word) = make_ulonglong2(lo, hi);
	return m;
}

// The fill with the row in registers: lane l holds columns j = 1 + 64 c + l, c < R.  1 <= lb <= 64 R, la >= 1.  Returns the end cell's key.
template <int R>
__device__ long long nw_fill_regs(const int32_t* __restrict__ a, const int32_t* __restrict__ b, int la, int lb, NwScores s, uint64_t* dirs) {
	const int lane = threadIdx.x;
	const int cb = (lb + NW_THREADS - 1) / NW_THREADS, cl = (lb - 1) / NW_THREADS;
	int up[R], id[R];
#pragma unroll
	for (int c = 0; c < R; ++c) {
		const int j = 1 + NW_THREADS * c + lane;
		up[c] = 0;
		id[c] = j <= lb ? b[j - 1] : 0;
	}
	int best = 0, best_i = 0;  // of this lane's column of chunk cl; only the lane of column lb is read
	int av = 0;
	for (int i = 1; i <= la; ++i) {
		if (((i - 1) & (NW_THREADS - 1)) == 0) av = i - 1 + lane < la ? a[i - 1 + lane] : 0;
		const int ai = __shfl(av, (i - 1) & (NW_THREADS - 1));
		int x[R];
#pragma unroll
		for (int c = 0; c < R; ++c) {  // independent scans: row i - 1 is all they read
			const int j = 1 + NW_THREADS * c + lane;
			const int diag = wave_dpp<0x138>(c == 0 ? 0 : __builtin_amdgcn_readlane(up[c > 0 ? c - 1 : 0], NW_THREADS - 1), up[c]);
			const int e = max(diag + (id[c] == ai ? s.match : s.sub), up[c] + s.del);
			x[c] = wave_prefix_max(j <= lb ? e - j * s.ins : NW_NEG, NW_NEG);
		}
		int run = 0, left_carry = 0;
#pragma unroll
		for (int c = 0; c < R; ++c) {
			if (c < cb) {
				const int j = 1 + NW_THREADS * c + lane;
				up[c] = nw_finish_chunk(x[c], run, left_carry, up[c], j, j <= lb, s, dirs + 2 * ((size_t)(i - 1) * cb + c));
				if (c == cl && up[c] > best) {
					best = up[c];
					best_i = i;
				}
			}
		}
	}
	if (la >= lb) return __shfl(nw_key(best, best_i), (lb - 1) % NW_THREADS);
	long long k = lane == 0 ? nw_key(0, 0) : nw_key(NW_NEG, 0);
#pragma unroll
	for (int c = 0; c < R; ++c) {
		const int j = 1 + NW_THREADS * c + lane;
		if (j <= lb) {
			const long long kj = nw_key(up[c], j);
			k = kj > k ? kj : k;
		}
	}
	return wave_max(k);
}

// The fill with the row (row[j] = M[i-1][j], j <= lb) and the reference ids (bid[j-1]) in LDS, one chunk after the other.
__device__ long long nw_fill_lds(const int32_t* __restrict__ a, const int32_t* __restrict__ b, int la, int lb, NwScores s, uint64_t* dirs, int* row,
                                 int* bid) {
	const int lane = threadIdx.x;
	const int cb = (lb + NW_THREADS - 1) / NW_THREADS, cl = (lb - 1) / NW_THREADS;
	for (int j = lane; j <= lb; j += NW_THREADS) {
		row[j] = 0;
		if (j < lb) bid[j] = b[j];
	}
	__syncthreads();
	int best = 0, best_i = 0;
	int av = 0;
	for (int i = 1; i <= la; ++i) {
		if (((i - 1) & (NW_THREADS - 1)) == 0) av = i - 1 + lane < la ? a[i - 1 + lane] : 0;
		const int ai = __shfl(av, (i - 1) & (NW_THREADS - 1));
		int diag_carry = 0, run = 0, left_carry = 0;
		for (int c = 0; c < cb; ++c) {
			const int j = 1 + NW_THREADS * c + lane;
			const bool valid = j <= lb;
			const int up = valid ? row[j] : 0;
			const int diag = wave_dpp<0x138>(diag_carry, up);
			diag_carry = __builtin_amdgcn_readlane(up, NW_THREADS - 1);
			const int e = max(diag + (valid && bid[j - 1] == ai ? s.match : s.sub), up + s.del);
			const int x = wave_prefix_max(valid ? e - j * s.ins : NW_NEG, NW_NEG);
			const int m = nw_finish_chunk(x, run, left_carry, up, j, valid, s, dirs + 2 * ((size_t)(i - 1) * cb + c));
			if (valid) row[j] = m;
			if (c == cl && m > best) {
				best = m;
				best_i = i;
			}
		}
	}
	if (la >= lb) return __shfl(nw_key(best, best_i), (lb - 1) % NW_THREADS);
	long long k = lane == 0 ? nw_key(0, 0) : nw_key(NW_NEG, 0);
	for (int j = 1 + lane; j <= lb; j += NW_THREADS) {
		const long long kj = nw_key(row[j], j);
		k = kj > k ? kj : k;
	}
	return wave_max(k);
}

__device__ __forceinline__ uint32_t nw_pack(int ai, int bj) { return (uint32_t)(ai + 1) | ((uint32_t)(bj + 1) << 16); }

__global__ __launch_bounds__(NW_THREADS) void nw_align_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ a_lengths,
                                                              const int32_t* __restrict__ b, const int32_t* __restrict__ b_lengths,
                                                              int32_t* __restrict__ a_index, int32_t* __restrict__ b_index,
                                                              int32_t* __restrict__ n_cols, int32_t* __restrict__ score, uint64_t* dir_base,
                                                              uint32_t* walk_base, int La, int Lb, NwScores s) {
	extern __shared__ __align__(16) int nw_smem[];
	const int lane = threadIdx.x;
	const int pair = blockIdx.x;
	const int la = clamp_len(a_lengths[pair], La), lb = clamp_len(b_lengths[pair], Lb);
	const int32_t* pa = a + (size_t)pair * La;
	const int32_t* pb = b + (size_t)pair * Lb;
	const int CB = (Lb + NW_THREADS - 1) / NW_THREADS;
	uint64_t* dirs = dir_base + 2 * (size_t)pair * La * CB;
	uint32_t* walk = walk_base + (size_t)pair * (La + Lb);
	const int cb = (lb + NW_THREADS - 1) / NW_THREADS;

	// the end cell (ei, ej) and its score
	long long key = nw_key(0, 0);
	if (la > 0 && lb > 0) {
		key = cb <= 1 ? nw_fill_regs<1>(pa, pb, la, lb, s, dirs) : cb <= 2 ? nw_fill_regs<2>(pa, pb, la, lb, s, dirs)
		    : cb <= 4 ? nw_fill_regs<4>(pa, pb, la, lb, s, dirs) : cb <= 8 ? nw_fill_regs<8>(pa, pb, la, lb, s, dirs)
		    : cb <= NW_REG_CHUNKS ? nw_fill_regs<NW_REG_CHUNKS>(pa, pb, la, lb, s, dirs)
		                          : nw_fill_lds(pa, pb, la, lb, s, dirs, nw_smem, nw_smem + Lb + NW_THREADS);
	}
	const int end_index = 0xFFFF - (int)(key & 0xFFFF);
	const int end_score = (int)((key - (key & 0xFFFF)) / 65536);
	const int ei = la < lb ? la : end_index, ej = la < lb ? end_index : lb;
	const int tail = la < lb ? lb - ej : la - ei;
	__syncthreads();  // lane 0's direction words are in memory before the walk reads them

	// the walk, lane 0: columns in reverse into walk[]
	int i = ei, j = ej, n_walk = 0;
	if (lane == 0) {
		int have_i = -1, have_c = -1;
		uint64_t lo = 0, hi = 0;
		while (i > 0 && j > 0) {
			const int c = (j - 1) / NW_THREADS, bit = (j - 1) % NW_THREADS;
			if (i != have_i || c != have_c) {
				const ulonglong2 w = *reinterpret_cast<const ulonglong2*>(dirs + 2 * ((size_t)(i - 1) * cb + c));
				lo = w.x;
				hi = w.y;
				have_i = i;
				have_c = c;
			}
			if ((hi >> bit) & 1) {
				walk[n_walk++] = nw_pack(i - 1, j - 1);
				--i;
				--j;
			} else if ((lo >> bit) & 1) {
				walk[n_walk++] = nw_pack(i - 1, -1);
				--i;
			} else {
				walk[n_walk++] = nw_pack(-1, j - 1);
				--j;
			}
		}
	}
	i = __shfl(i, 0);
	j = __shfl(j, 0);
	n_walk = __shfl(n_walk, 0);
	__syncthreads();  // walk[] is in memory before every lane reads it

	// forward order: the prefix against gaps, the walked columns, the tail against gaps; -1 past the last column
	const int prefix = i + j;  // one of them is 0
	const int n = prefix + n_walk + tail;
	int32_t* oa = a_index + (size_t)pair * (La + Lb);
	int32_t* ob = b_index + (size_t)pair * (La + Lb);
	for (int k = lane; k < La + Lb; k += NW_THREADS) {
		int ca = -1, cbj = -1;
		if (k < prefix) {
			ca = i > 0 ? k : -1;
			cbj = j > 0 ? k : -1;
		} else if (k < prefix + n_walk) {
			const uint32_t w = walk[n_walk - 1 - (k - prefix)];
			ca = (int)(w & 0xFFFF) - 1;
			cbj = (int)(w >> 16) - 1;
		} else if (k < n) {
			const int t = k - prefix - n_walk;
			ca = la < lb ? -1 : ei + t;
			cbj = la < lb ? ej + t : -1;
		}
		oa[k] = ca;
		ob[k] = cbj;
	}
	if (lane == 0) {
		n_cols[pair] = n;
		score[pair] = end_score;
	}
}

inline bool nw_shape_ok(int N, int La, int Lb) {
	return N >= 1 && N < (1 << 20) && La >= 0 && La <= CONVASR_METRIC_MAX_LEN && Lb >= 0 && Lb <= CONVASR_METRIC_MAX_LEN;
}

inline int64_t nw_dir_bytes(int N, int La, int Lb) { return (int64_t)N * La * ((Lb + NW_THREADS - 1) / NW_THREADS) * 16; }

}  // namespace

extern "C" int64_t convasr_nw_align_workspace_bytes(int N, int La, int Lb) {
	if (!nw_shape_ok(N, La, Lb)) {
		convasr_fail(CONVASR_EINVAL, "nw_align_workspace_bytes: N %d in [1, 2^20), La %d and Lb %d in [0, %d] expected", N, La, Lb, CONVASR_METRIC_MAX_LEN);
		return -1;
	}
	return nw_dir_bytes(N, La, Lb) + (int64_t)N * (La + Lb) * 4;
}

extern "C" int convasr_nw_align(const int32_t* a, const int32_t* a_lengths, const int32_t* b, const int32_t* b_lengths, int32_t* a_index,
                                int32_t* b_index, int32_t* n_cols, int32_t* score, void* workspace, int64_t workspace_bytes, int N, int La,
                                int Lb, int match, int sub, int del, int ins, void* stream) {
	CONVASR_CHECK_ARG(a && a_lengths && b && b_lengths && a_index && b_index && n_cols && score && workspace, "nw_align: NULL pointer");
	CONVASR_CHECK_ARG(N >= 1 && N < (1 << 20), "nw_align: N = %d pairs, 1 to 2^20 - 1 expected", N);
	CONVASR_CHECK_ARG(nw_shape_ok(N, La, Lb), "nw_align: La %d and Lb %d must be in [0, %d]", La, Lb, CONVASR_METRIC_MAX_LEN);
	CONVASR_CHECK_ARG(abs(match) <= NW_MAX_SCORE && abs(sub) <= NW_MAX_SCORE && abs(del) <= NW_MAX_SCORE && abs(ins) <= NW_MAX_SCORE,
	                  "nw_align: scores (%d, %d, %d, %d) must lie in [-%d, %d]", match, sub, del, ins, NW_MAX_SCORE, NW_MAX_SCORE);
	const int64_t need = convasr_nw_align_workspace_bytes(N, La, Lb);
	CONVASR_CHECK_ARG(workspace_bytes >= need, "nw_align: workspace of %lld bytes, %lld needed for N %d, La %d, Lb %d", (long long)workspace_bytes,
	                  (long long)need, N, La, Lb);
	CONVASR_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "nw_align: workspace must be 16-byte aligned");
	const size_t lds = Lb > NW_REG_CHUNKS * NW_THREADS ? 4 * (size_t)(2 * Lb + 2 * NW_THREADS) : 0;  // the row (Lb + 1) and the reference ids (Lb)
	static unsigned long long set = 0;
	convasr_allow_160k_lds(reinterpret_cast<const void*>(nw_align_kernel), set);
	uint64_t* dirs = static_cast<uint64_t*>(workspace);
	uint32_t* walk = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + nw_dir_bytes(N, La, Lb));
	hipLaunchKernelGGL(nw_align_kernel, dim3(N), dim3(NW_THREADS), lds, (hipStream_t)stream, a, a_lengths, b, b_lengths, a_index, b_index, n_cols,
	                   score, dirs, walk, La, Lb, NwScores{match, sub, del, ins});
	CONVASR_CHECK_LAUNCH("nw_align");
	return 0;
}
