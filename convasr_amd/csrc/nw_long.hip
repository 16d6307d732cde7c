// The two integer DPs of the scoring step for whole recordings, on many CUs: convasr_nw_align_long (the alignment of csrc/align.hip,
// bit for bit) and convasr_edit_distance_long (the Levenshtein distance of csrc/metrics.hip over ready-made unit ids), both up to
// 131,071 units a side.  The one-wave-per-pair kernels stop at 16,383 units and run one long pair on one CU; an hour of speech is
// ~55,000 characters.  The semantics are normative in include/convasr_hip.h and restated by tests/_align_ref.py / tests/_metrics_ref.py.
//
// The (la + 1) x (lb + 1) matrix is cut into square tiles of NWL_T x NWL_T cells: tile (ti, tj) holds rows ti * NWL_T + 1 .. and
// columns tj * NWL_T + 1 .. (row 0 and column 0 are the boundary conditions).  A tile depends on the tile above it (its last row), the
// tile left of it (its last column) and the tile above-left (one corner cell).  Tiles with ti + tj = k are independent: launch k of a
// plain sequence of launches runs them for all N pairs, one wave per tile.  Every byte a tile reads from another tile was written by an
// earlier launch; nothing waits, spins or polls inside a launch, and no atomic is used.
//   rows[pair][ti][j], j <= Lb: row (ti + 1) * NWL_T of the matrix -- written by the tiles of tile row ti, read by tile row ti + 1
//     (entry tj * NWL_T is the corner of tile (ti + 1, tj)).
//   cols[pair][tj][i], i <= La: column (tj + 1) * NWL_T -- written by the tiles of tile column tj, read by tile column tj + 1.
// Row 0 and column 0 are never stored: a tile of the first tile row / column substitutes the boundary condition.
//
// Fill (both DPs): lane l holds columns j0 + 64 c + l, c < NWL_C, of the row above in registers; a row is E[j] from the row above, a DPP
// prefix maximum (minimum) per 64-column chunk, and the running maximum carried between chunks -- the formulation of align.hip /
// metrics.hip.  The left neighbour's column enters a row twice: as the initial running maximum M[i][j0 - 1] - (j0 - 1) * ins and as lane
// 0's left neighbour; its value at the row before is lane 0's diagonal.  Integer maxima are exact, so the cut changes no cell.
// Alignment only: 2 direction bits per cell, per tile contiguously (row r of the tile: 2 x 64-bit ballots per chunk = NWL_C x 16 bytes);
// the end cell as a per-tile best key (value * 2^18 + (2^18 - 1 - index): the larger value, then the lower index) left by the tiles of
// the last tile row (la < lb) or the last tile column, reduced by the walk.  Walk: one wave per pair stages the direction rows of the
// tile it is in into LDS, lane 0 walks inside LDS and writes the columns in reverse into the workspace; all lanes then write them
// forward, the gap runs of the prefix and of the tail computed, not walked.
#include "common.h"

namespace {

constexpr int NWL_T = 256;                    // tile edge (cells), a multiple of 64
constexpr int NWL_C = NWL_T / 64;             // 64-column chunks per lane
constexpr int NWL_TILE_WORDS = NWL_T * NWL_C * 2;  // 64-bit direction words per tile (16 KiB)
constexpr int NWL_MAX_LEN = 131071;
constexpr int NWL_MAX_SCORE = 2048;
constexpr int NWL_NEG = -(1 << 30);  // below every E[k] - k * ins the envelope allows: |cell| <= 2048 * 262,142 < 2^29, |k * ins| <= 2048 * 131,071
constexpr int NWL_BIG = 1 << 20;     // above every distance (<= 131,071) and every E[k] - k
constexpr int NWL_GRID_Y = 32768;    // pairs per grid.y; grid.z takes the rest (N < 2^20)

struct NwlScores {
	int match, sub, del, ins;
};

// (value, index) as one key: the larger value wins, then the lower index (index < 2^18, |value| < 2^29: |key| < 2^48)
__device__ __forceinline__ long long nwl_key(int value, int index) { return (long long)value * 262144 + (0x3FFFF - index); }

// M[.][j] of a register row for the column of chunk `which`, lane `at` (both wave-uniform): scalar selects over four readlanes (an
// indexed read of the register row would be moved to LDS by the compiler)
__device__ __forceinline__ int nwl_pick(const int (&v)[NWL_C], int which, int at) {
	int r = __builtin_amdgcn_readlane(v[0], at);
#pragma unroll
	for (int c = 1; c < NWL_C; ++c) {
		const int vc = __builtin_amdgcn_readlane(v[c], at);
		r = which == c ? vc : r;
	}
	return r;
}

struct NwlTile {
	int pair, ti, tj, la, lb, i0, j0, i_end;
	bool live;
};

// which tile this workgroup fills; live = false for a tile wholly outside the pair's own la x lb (or a pair past N)
__device__ __forceinline__ NwlTile nwl_tile(const int32_t* a_lengths, const int32_t* b_lengths, int N, int La, int Lb, int diag, int ti_lo) {
	NwlTile t;
	t.pair = blockIdx.y + blockIdx.z * gridDim.y;
	t.live = false;
	if (t.pair >= N) return t;
	t.ti = ti_lo + (int)blockIdx.x;
	t.tj = diag - t.ti;
	t.la = clamp_len(a_lengths[t.pair], La);
	t.lb = clamp_len(b_lengths[t.pair], Lb);
	t.i0 = t.ti * NWL_T + 1;
	t.j0 = t.tj * NWL_T + 1;
	t.i_end = min(t.la, t.i0 + NWL_T - 1);
	t.live = t.i0 <= t.la && t.j0 <= t.lb;
	return t;
}

__global__ __launch_bounds__(64) void nw_long_fill_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ a_lengths, const int32_t* __restrict__ b,
                                                          const int32_t* __restrict__ b_lengths, uint64_t* __restrict__ dirs, int* __restrict__ rows,
                                                          int* __restrict__ cols, long long* __restrict__ endk, int N, int La, int Lb, int nTi, int nTj,
                                                          int nEnd, int diag, int ti_lo, NwlScores s) {
	const NwlTile t = nwl_tile(a_lengths, b_lengths, N, La, Lb, diag, ti_lo);
	if (!t.live) return;
	const int lane = threadIdx.x;
	const int la = t.la, lb = t.lb, ti = t.ti, tj = t.tj, i0 = t.i0, j0 = t.j0, i_end = t.i_end;
	const int32_t* pa = a + (size_t)t.pair * La;
	const int32_t* pb = b + (size_t)t.pair * Lb;
	int* above = rows + ((size_t)t.pair * nTi + (ti > 0 ? ti - 1 : 0)) * (Lb + 1);  // (read for ti > 0 only)
	int* below = rows + ((size_t)t.pair * nTi + ti) * (Lb + 1);
	const int* left = cols + ((size_t)t.pair * nTj + (tj > 0 ? tj - 1 : 0)) * (La + 1);  // (read for tj > 0 only)
	int* right = cols + ((size_t)t.pair * nTj + tj) * (La + 1);
	uint64_t* dt = dirs + ((size_t)t.pair * nTi * nTj + (size_t)ti * nTj + tj) * NWL_TILE_WORDS;
	const bool cols_full = j0 + NWL_T - 1 <= lb;  // the tile's last column exists: it is published for tile column tj + 1
	const bool end_col = la >= lb && (lb - 1) / NWL_T == tj;  // column lb is in this tile and decides the end cell
	const int cl = __builtin_amdgcn_readfirstlane(((lb - 1) % NWL_T) / 64), lane_lb = __builtin_amdgcn_readfirstlane((lb - 1) % 64);

	int up[NWL_C], id[NWL_C];
#pragma unroll
	for (int c = 0; c < NWL_C; ++c) {
		const int j = j0 + 64 * c + lane;
		id[c] = j <= lb ? pb[j - 1] : 0;
		up[c] = (ti > 0 && j <= lb) ? above[j] : 0;
	}
	int prev_left = (ti > 0 && tj > 0) ? above[j0 - 1] : 0;  // M[i - 1][j0 - 1]: the corner, then the left column
	int best = NWL_NEG, best_i = 0;  // of column lb over this tile's rows, the lowest row first (wave-uniform)
	int av = 0, lv = 0, cv = 0;
	for (int i = i0; i <= i_end; ++i) {
		const int r = i - i0, q = r & 63;
		if (q == 0) {
			av = i - 1 + lane < la ? pa[i - 1 + lane] : 0;
			lv = (tj > 0 && i + lane <= i_end) ? left[i + lane] : 0;
		}
		const int ai = __shfl(av, q), left_i = __shfl(lv, q);  // M[i][j0 - 1]
		int x[NWL_C];
#pragma unroll
		for (int c = 0; c < NWL_C; ++c) {  // independent scans: row i - 1 is all they read
			const int j = j0 + 64 * c + lane;
			const int diagv = wave_dpp<0x138>(c == 0 ? prev_left : __builtin_amdgcn_readlane(up[c > 0 ? c - 1 : 0], 63), up[c]);
			const int e = max(diagv + (id[c] == ai ? s.match : s.sub), up[c] + s.del);
			x[c] = wave_prefix_max(j <= lb ? e - j * s.ins : NWL_NEG, NWL_NEG);
		}
		int run = left_i - (j0 - 1) * s.ins, left_carry = left_i;
		uint64_t w[2 * NWL_C];
#pragma unroll
		for (int c = 0; c < NWL_C; ++c) {
			const int j = j0 + 64 * c + lane;
			const bool valid = j <= lb;
			const int v = max(x[c], run);
			run = __builtin_amdgcn_readlane(v, 63);
			const int m = valid ? v + j * s.ins : 0;
			const int lft = wave_dpp<0x138>(left_carry, m);  // wave_shr:1, lane 0 <- M[i][j - 1] of the chunk before
			left_carry = __builtin_amdgcn_readlane(m, 63);
			const bool is_ins = m == lft + s.ins;
			const bool is_del = !is_ins && m == up[c] + s.del;
			w[2 * c] = __ballot(valid && is_del);
			w[2 * c + 1] = __ballot(valid && !is_ins && !is_del);
			up[c] = m;
		}
		prev_left = left_i;
		uint64_t mine = w[0];
#pragma unroll
		for (int k = 1; k < 2 * NWL_C; ++k) mine = lane == k ? w[k] : mine;
		if (lane < 2 * NWL_C) dt[r * (2 * NWL_C) + lane] = mine;
		if (end_col) {
			const int m = nwl_pick(up, cl, lane_lb);
			if (m > best) {
				best = m;
				best_i = i;
			}
		}
		if (cols_full) {  // column j0 + NWL_T - 1, 64 rows per store
			const int last = __builtin_amdgcn_readlane(up[NWL_C - 1], 63);
			cv = lane == q ? last : cv;
			if ((q == 63 || i == i_end) && lane <= q) right[i - q + lane] = cv;
		}
	}
	if (i_end == i0 + NWL_T - 1) {  // the tile's last row exists: it is published for tile row ti + 1
#pragma unroll
		for (int c = 0; c < NWL_C; ++c) {
			const int j = j0 + 64 * c + lane;
			if (j <= lb) below[j] = up[c];
		}
	}
	long long* ek = endk + (size_t)t.pair * nEnd;
	if (end_col) {
		if (lane == 0) ek[ti] = nwl_key(best, best_i);
	} else if (la < lb && i_end == la) {  // row la is this tile's last: its best column
		long long k = nwl_key(NWL_NEG, 0);
#pragma unroll
		for (int c = 0; c < NWL_C; ++c) {
			const int j = j0 + 64 * c + lane;
			if (j <= lb) {
				const long long kj = nwl_key(up[c], j);
				k = kj > k ? kj : k;
			}
		}
		k = wave_max(k);
		if (lane == 0) ek[tj] = k;
	}
}

__global__ __launch_bounds__(64) void nw_long_walk_kernel(const int32_t* __restrict__ a_lengths, const int32_t* __restrict__ b_lengths,
                                                          int32_t* __restrict__ a_index, int32_t* __restrict__ b_index, int32_t* __restrict__ n_cols,
                                                          int32_t* __restrict__ score, const uint64_t* __restrict__ dirs, const long long* __restrict__ endk,
                                                          int2* __restrict__ walk_base, int La, int Lb, int nTi, int nTj, int nEnd) {
	__shared__ __align__(16) uint64_t win[NWL_TILE_WORDS];
	const int lane = threadIdx.x;
	const int pair = blockIdx.x;
	const int la = clamp_len(a_lengths[pair], La), lb = clamp_len(b_lengths[pair], Lb);
	const uint64_t* dp = dirs + (size_t)pair * nTi * nTj * NWL_TILE_WORDS;
	int2* walk = walk_base + (size_t)pair * (La + Lb);

	// the end cell (ei, ej) and its score: row 0 / column 0 give (0, index 0), the tiles of the last tile row / column the rest
	long long key = nwl_key(0, 0);
	if (la > 0 && lb > 0) {
		const int n = (la < lb ? lb - 1 : la - 1) / NWL_T + 1;
		const long long* ek = endk + (size_t)pair * nEnd;
		for (int k = lane; k < n; k += 64) key = ek[k] > key ? ek[k] : key;
		key = wave_max(key);
	}
	const int end_index = 0x3FFFF - (int)(key & 0x3FFFF);
	const int end_score = (int)((key - (key & 0x3FFFF)) / 262144);
	const int ei = la < lb ? la : end_index, ej = la < lb ? end_index : lb;
	const int tail = la < lb ? lb - ej : la - ei;

	// the walk: the direction rows 0 .. (i - 1) % NWL_T of the tile of (i, j) into LDS, lane 0 walks until it leaves the tile
	int i = ei, j = ej, n_walk = 0;
	while (i > 0 && j > 0) {
		const int ti = (i - 1) / NWL_T, tj = (j - 1) / NWL_T;
		const ulonglong2* src = reinterpret_cast<const ulonglong2*>(dp + ((size_t)ti * nTj + tj) * NWL_TILE_WORDS);
		const int n16 = ((i - 1) % NWL_T + 1) * NWL_C;
		for (int k = lane; k < n16; k += 64) reinterpret_cast<ulonglong2*>(win)[k] = src[k];
		__syncthreads();
		if (lane == 0) {
			while (i > 0 && j > 0 && (i - 1) / NWL_T == ti && (j - 1) / NWL_T == tj) {
				const int cj = (j - 1) % NWL_T;
				const int word = (((i - 1) % NWL_T) * NWL_C + cj / 64) * 2, bit = cj % 64;
				if ((win[word + 1] >> bit) & 1) {
					walk[n_walk++] = make_int2(i - 1, j - 1);
					--i;
					--j;
				} else if ((win[word] >> bit) & 1) {
					walk[n_walk++] = make_int2(i - 1, -1);
					--i;
				} else {
					walk[n_walk++] = make_int2(-1, j - 1);
					--j;
				}
			}
		}
		i = __shfl(i, 0);
		j = __shfl(j, 0);
		n_walk = __shfl(n_walk, 0);
		__syncthreads();  // win[] is refilled by the next tile; walk[] is in memory before every lane reads it
	}

	// forward order: the prefix against gaps, the walked columns, the tail against gaps; -1 past the last column
	const int prefix = i + j;  // one of them is 0
	const int n = prefix + n_walk + tail;
	int32_t* oa = a_index + (size_t)pair * (La + Lb);
	int32_t* ob = b_index + (size_t)pair * (La + Lb);
	for (int k = lane; k < La + Lb; k += 64) {
		int ca = -1, cb = -1;
		if (k < prefix) {
			ca = i > 0 ? k : -1;
			cb = j > 0 ? k : -1;
		} else if (k < prefix + n_walk) {
			const int2 wk = walk[n_walk - 1 - (k - prefix)];
			ca = wk.x;
			cb = wk.y;
		} else if (k < n) {
			const int tk = k - prefix - n_walk;
			ca = la < lb ? -1 : ei + tk;
			cb = la < lb ? ej + tk : -1;
		}
		oa[k] = ca;
		ob[k] = cb;
	}
	if (lane == 0) {
		n_cols[pair] = n;
		score[pair] = end_score;
	}
}

// Levenshtein: the same tiles with min for max, D[i][0] = i, D[0][j] = j; no directions.  The tile of cell (la, lb) writes the distance.
__global__ __launch_bounds__(64) void ed_long_fill_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ a_lengths, const int32_t* __restrict__ b,
                                                          const int32_t* __restrict__ b_lengths, int32_t* __restrict__ distance, int* __restrict__ rows,
                                                          int* __restrict__ cols, int N, int La, int Lb, int nTi, int nTj, int diag, int ti_lo) {
	const NwlTile t = nwl_tile(a_lengths, b_lengths, N, La, Lb, diag, ti_lo);
	if (!t.live) return;
	const int lane = threadIdx.x;
	const int la = t.la, lb = t.lb, ti = t.ti, tj = t.tj, i0 = t.i0, j0 = t.j0, i_end = t.i_end;
	const int32_t* pa = a + (size_t)t.pair * La;
	const int32_t* pb = b + (size_t)t.pair * Lb;
	int* above = rows + ((size_t)t.pair * nTi + (ti > 0 ? ti - 1 : 0)) * (Lb + 1);
	int* below = rows + ((size_t)t.pair * nTi + ti) * (Lb + 1);
	const int* left = cols + ((size_t)t.pair * nTj + (tj > 0 ? tj - 1 : 0)) * (La + 1);
	int* right = cols + ((size_t)t.pair * nTj + tj) * (La + 1);
	const bool cols_full = j0 + NWL_T - 1 <= lb;

	// columns past lb compute garbage that no valid column reads: a valid column's diagonal comes from the column before it, also valid
	int up[NWL_C], id[NWL_C];
#pragma unroll
	for (int c = 0; c < NWL_C; ++c) {
		const int j = j0 + 64 * c + lane;
		id[c] = j <= lb ? pb[j - 1] : 0;
		up[c] = (ti > 0 && j <= lb) ? above[j] : j;
	}
	int prev_left = ti == 0 ? j0 - 1 : tj == 0 ? i0 - 1 : above[j0 - 1];  // D[i - 1][j0 - 1]
	int av = 0, lv = 0, cv = 0;
	for (int i = i0; i <= i_end; ++i) {
		const int r = i - i0, q = r & 63;
		if (q == 0) {
			av = i - 1 + lane < la ? pa[i - 1 + lane] : 0;
			lv = (tj > 0 && i + lane <= i_end) ? left[i + lane] : i + lane;
		}
		const int ai = __shfl(av, q), left_i = __shfl(lv, q);  // D[i][j0 - 1]
		int x[NWL_C];
#pragma unroll
		for (int c = 0; c < NWL_C; ++c) {
			const int j = j0 + 64 * c + lane;
			const int diagv = wave_dpp<0x138>(c == 0 ? prev_left : __builtin_amdgcn_readlane(up[c > 0 ? c - 1 : 0], 63), up[c]);
			x[c] = wave_prefix_min(j <= lb ? min(up[c] + 1, diagv + (id[c] != ai)) - j : NWL_BIG, NWL_BIG);
		}
		int run = left_i - (j0 - 1);
#pragma unroll
		for (int c = 0; c < NWL_C; ++c) {
			const int v = min(x[c], run);
			run = __builtin_amdgcn_readlane(v, 63);
			up[c] = v + j0 + 64 * c + lane;
		}
		prev_left = left_i;
		if (cols_full) {
			const int last = __builtin_amdgcn_readlane(up[NWL_C - 1], 63);
			cv = lane == q ? last : cv;
			if ((q == 63 || i == i_end) && lane <= q) right[i - q + lane] = cv;
		}
	}
	if (i_end == i0 + NWL_T - 1) {
#pragma unroll
		for (int c = 0; c < NWL_C; ++c) {
			const int j = j0 + 64 * c + lane;
			if (j <= lb) below[j] = up[c];
		}
	}
	if (i_end == la && (lb - 1) / NWL_T == tj) {
		const int d = nwl_pick(up, __builtin_amdgcn_readfirstlane(((lb - 1) % NWL_T) / 64), __builtin_amdgcn_readfirstlane((lb - 1) % 64));
		if (lane == 0) distance[t.pair] = d;
	}
}

// the pairs no tile runs for: an empty side leaves the other side's length
__global__ __launch_bounds__(256) void ed_long_empty_kernel(const int32_t* __restrict__ a_lengths, const int32_t* __restrict__ b_lengths,
                                                            int32_t* __restrict__ distance, int N, int La, int Lb) {
	const int pair = blockIdx.x * 256 + threadIdx.x;
	if (pair >= N) return;
	const int la = clamp_len(a_lengths[pair], La), lb = clamp_len(b_lengths[pair], Lb);
	if (la == 0 || lb == 0) distance[pair] = la + lb;
}

inline int64_t nwl_up(int64_t n) { return (n + 255) & ~(int64_t)255; }
inline int nwl_tiles(int L) { return (L + NWL_T - 1) / NWL_T; }

struct NwlLayout {
	int nTi, nTj, nEnd;
	int64_t rows_off, cols_off, end_off, walk_off, bytes;  // (the directions are at offset 0)
};

// align = false: the two boundary families only
inline NwlLayout nwl_layout(int N, int La, int Lb, bool align) {
	NwlLayout y;
	y.nTi = nwl_tiles(La);
	y.nTj = nwl_tiles(Lb);
	y.nEnd = max(max(y.nTi, y.nTj), 1);
	y.rows_off = align ? nwl_up((int64_t)N * y.nTi * y.nTj * NWL_TILE_WORDS * 8) : 0;
	y.cols_off = y.rows_off + nwl_up((int64_t)N * y.nTi * (Lb + 1) * 4);
	y.end_off = y.cols_off + nwl_up((int64_t)N * y.nTj * (La + 1) * 4);
	y.walk_off = y.end_off + (align ? nwl_up((int64_t)N * y.nEnd * 8) : 0);
	y.bytes = y.walk_off + (align ? nwl_up((int64_t)N * ((int64_t)La + Lb) * 8) : 0);
	return y;
}

inline int nwl_check(const char* who, int N, int La, int Lb) {
	if (N < 1 || N >= (1 << 20)) return convasr_fail(CONVASR_EINVAL, "%s: N = %d pairs, 1 to 2^20 - 1 expected", who, N);
	if (La < 0 || Lb < 0) return convasr_fail(CONVASR_EINVAL, "%s: La %d and Lb %d must be >= 0", who, La, Lb);
	if (La > NWL_MAX_LEN || Lb > NWL_MAX_LEN) return convasr_fail(CONVASR_EUNSUPPORTED, "%s: La %d and Lb %d must be at most %d", who, La, Lb, NWL_MAX_LEN);
	return 0;
}

// launch k runs the tiles ti + tj = k of all N pairs
template <typename Launch>
inline void nwl_sweep(int N, int nTi, int nTj, Launch launch) {
	const unsigned gy = (unsigned)min(N, NWL_GRID_Y), gz = (unsigned)((N + NWL_GRID_Y - 1) / NWL_GRID_Y);
	for (int k = 0; nTi > 0 && nTj > 0 && k < nTi + nTj - 1; ++k) {
		const int ti_lo = max(0, k - nTj + 1), ti_hi = min(k, nTi - 1);
		launch(dim3((unsigned)(ti_hi - ti_lo + 1), gy, gz), k, ti_lo);
	}
}

}  // namespace

extern "C" int convasr_nw_align_long_tile(void) { return NWL_T; }

extern "C" int64_t convasr_nw_align_long_workspace_bytes(int N, int La, int Lb) {
	if (nwl_check("nw_align_long_workspace_bytes", N, La, Lb) != 0) return -1;
	return nwl_layout(N, La, Lb, true).bytes;
}

extern "C" int64_t convasr_edit_distance_long_workspace_bytes(int N, int La, int Lb) {
	if (nwl_check("edit_distance_long_workspace_bytes", N, La, Lb) != 0) return -1;
	return nwl_layout(N, La, Lb, false).bytes;
}

// parts: 1 = the fill, 2 = the walk over a workspace that a fill with the same arguments left, 3 = both (measurements time the two apart)
extern "C" int convasr_nw_align_long_parts(const int32_t* a, const int32_t* a_lengths, const int32_t* b, const int32_t* b_lengths, int32_t* a_index,
                                           int32_t* b_index, int32_t* n_cols, int32_t* score, void* workspace, int64_t workspace_bytes, int N, int La,
                                           int Lb, int match, int sub, int del, int ins, int parts, void* stream) {
	CONVASR_CHECK_ARG(parts >= 1 && parts <= 3, "nw_align_long: parts %d is not 1 (fill), 2 (walk) or 3 (both)", parts);
	CONVASR_CHECK_ARG(a && a_lengths && b && b_lengths && a_index && b_index && n_cols && score && workspace, "nw_align_long: NULL pointer");
	if (const int e = nwl_check("nw_align_long", N, La, Lb)) return e;
	CONVASR_CHECK_ARG(abs(match) <= NWL_MAX_SCORE && abs(sub) <= NWL_MAX_SCORE && abs(del) <= NWL_MAX_SCORE && abs(ins) <= NWL_MAX_SCORE,
	                  "nw_align_long: scores (%d, %d, %d, %d) must lie in [-%d, %d]", match, sub, del, ins, NWL_MAX_SCORE, NWL_MAX_SCORE);
	const NwlLayout y = nwl_layout(N, La, Lb, true);
	CONVASR_CHECK_ARG(workspace_bytes >= y.bytes, "nw_align_long: workspace of %lld bytes, %lld needed for N %d, La %d, Lb %d", (long long)workspace_bytes,
	                  (long long)y.bytes, N, La, Lb);
	CONVASR_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "nw_align_long: workspace must be 16-byte aligned");
	hipStream_t st = (hipStream_t)stream;
	char* ws = static_cast<char*>(workspace);
	uint64_t* dirs = reinterpret_cast<uint64_t*>(ws);
	int* rows = reinterpret_cast<int*>(ws + y.rows_off);
	int* cols = reinterpret_cast<int*>(ws + y.cols_off);
	long long* endk = reinterpret_cast<long long*>(ws + y.end_off);
	int2* walk = reinterpret_cast<int2*>(ws + y.walk_off);
	const NwlScores s{match, sub, del, ins};
	if (parts & 1)
		nwl_sweep(N, y.nTi, y.nTj, [&](dim3 grid, int k, int ti_lo) {
			hipLaunchKernelGGL(nw_long_fill_kernel, grid, dim3(64), 0, st, a, a_lengths, b, b_lengths, dirs, rows, cols, endk, N, La, Lb, y.nTi, y.nTj, y.nEnd, k,
			                   ti_lo, s);
		});
	CONVASR_CHECK_LAUNCH("nw_align_long (fill)");
	if (parts & 2)
		hipLaunchKernelGGL(nw_long_walk_kernel, dim3(N), dim3(64), 0, st, a_lengths, b_lengths, a_index, b_index, n_cols, score, dirs, endk, walk, La, Lb, y.nTi,
		                   y.nTj, y.nEnd);
	CONVASR_CHECK_LAUNCH("nw_align_long (walk)");
	return 0;
}

extern "C" int convasr_nw_align_long(const int32_t* a, const int32_t* a_lengths, const int32_t* b, const int32_t* b_lengths, int32_t* a_index,
                                     int32_t* b_index, int32_t* n_cols, int32_t* score, void* workspace, int64_t workspace_bytes, int N, int La, int Lb,
                                     int match, int sub, int del, int ins, void* stream) {
	return convasr_nw_align_long_parts(a, a_lengths, b, b_lengths, a_index, b_index, n_cols, score, workspace, workspace_bytes, N, La, Lb, match, sub, del,
	                                   ins, 3, stream);
}

extern "C" int convasr_edit_distance_long(const int32_t* a, const int32_t* a_lengths, const int32_t* b, const int32_t* b_lengths, int32_t* distance,
                                          void* workspace, int64_t workspace_bytes, int N, int La, int Lb, void* stream) {
	CONVASR_CHECK_ARG(a && a_lengths && b && b_lengths && distance && workspace, "edit_distance_long: NULL pointer");
	if (const int e = nwl_check("edit_distance_long", N, La, Lb)) return e;
	const NwlLayout y = nwl_layout(N, La, Lb, false);
	CONVASR_CHECK_ARG(workspace_bytes >= y.bytes, "edit_distance_long: workspace of %lld bytes, %lld needed for N %d, La %d, Lb %d",
	                  (long long)workspace_bytes, (long long)y.bytes, N, La, Lb);
	CONVASR_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "edit_distance_long: workspace must be 16-byte aligned");
	hipStream_t st = (hipStream_t)stream;
	char* ws = static_cast<char*>(workspace);
	int* rows = reinterpret_cast<int*>(ws + y.rows_off);
	int* cols = reinterpret_cast<int*>(ws + y.cols_off);
	hipLaunchKernelGGL(ed_long_empty_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, a_lengths, b_lengths, distance, N, La, Lb);
	nwl_sweep(N, y.nTi, y.nTj, [&](dim3 grid, int k, int ti_lo) {
		hipLaunchKernelGGL(ed_long_fill_kernel, grid, dim3(64), 0, st, a, a_lengths, b, b_lengths, distance, rows, cols, N, La, Lb, y.nTi, y.nTj, k, ti_lo);
	});
	CONVASR_CHECK_LAUNCH("edit_distance_long");
	return 0;
}
