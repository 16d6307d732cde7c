// Two-channel diarization on the device: the reference's select_speaker (diarization.py:58-99), models.rle1d (models.py:777-785) and the
// counts behind speaker_error (diarization.py:175-201).  The semantics are normative in include/convasr_hip.h and restated in numpy by
// tests/_diar_ref.py.  Every kernel is a streaming pass whose cost does not depend on a window size:
//
//   slide_max_kernel   sliding maximum, stride 1, window K, -inf padding: van Herk / Gil-Werman.  A workgroup loads a span of S = THREADS x 31
//       padded positions into LDS (|x| or -x taken at the load), every thread takes 31 consecutive ones into registers (a stride of 31 words
//       between lanes: no bank conflict) and computes, over blocks of K aligned to the output coordinate, the suffix maxima h (written back
//       over the span) and the prefix maxima g (kept in registers); the carries between threads are a segmented max-scan (wave shuffles, then
//       the wave totals through LDS).  out[i] = max(h[i], g[i + K - 1]) is formed in place by the thread that owns g, and the first
//       T = S - K + 1 words of the span leave as coalesced stores.  S = 7,936 (256 threads, 31 KiB) for K <= 2,048, 31,744 (1,024 threads,
//       124 KiB) above: a tile re-reads K - 1 inputs of its neighbour, 35 % at K = 2,048 and at K = 8,192, 2.07 x at K = 16,384.
//   kth_*              k-th smallest of non-negative floats: their bit patterns order as unsigned integers, so three histogram passes over
//       digits of 11, 11 and 10 bits (LDS histogram per workgroup, flushed with atomics) and a one-workgroup pick after each give the exact
//       value.
//   scan_*             int32 prefix sum over any length: per-tile sums, one workgroup scans the sums, per-tile scan with the offset.  Used for
//       the speaker sign (+1 / 0 / -1 of channel 0 against channel 1, compared, not subtracted) and for the run boundaries of rle1d.
//   diar_combine_kernel  box sums as differences of the prefix sum, their sign, the 3-tap repair, the silence tests (one IEEE add and one IEEE
//       divide per channel; this file is built without fast-math) and both outputs.
//   rle_*              boundary flags -> count (one host read) -> starts / lengths / values.
//   spk_err_*          the seven counts per permutation in one pass over both masks, per-workgroup partials and a finishing launch.
// No memset or copy node: every word a kernel reads was written by a kernel of the same call.
#include "common.h"

namespace {

constexpr int DIAR_E = 31;  // elements per thread of the sliding maximum (odd: conflict-free LDS stride)
constexpr int DIAR_SMALL_THREADS = 256, DIAR_LARGE_THREADS = 1024, DIAR_SMALL_K = 2048;
constexpr int64_t DIAR_MAX_LEN = CONVASR_DIAR_MAX_LEN;
constexpr int DIAR_MAX_K = CONVASR_DIAR_MAX_KERNEL;

inline int64_t slide_out_len(int64_t Lin, int K) { return Lin + 2 * (int64_t)(K / 2) - K + 1; }
inline int slide_threads(int K) { return K <= DIAR_SMALL_K ? DIAR_SMALL_THREADS : DIAR_LARGE_THREADS; }
inline int64_t up256(int64_t x) { return (x + 255) / 256 * 256; }

// ---------------------------------------------------------------------------------------------------------------- sliding maximum

template <int THREADS>
__global__ __launch_bounds__(THREADS) void slide_max_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t Lin, int64_t Lout, int K, int pad,
                                                            int flags) {
	constexpr int S = THREADS * DIAR_E, WAVES = THREADS / 64;
	extern __shared__ __align__(16) float sm_span[];  // S floats, then per wave: prefix total, prefix flag, suffix total, suffix flag
	float* wave_pv = sm_span + S;
	int* wave_pf = reinterpret_cast<int*>(wave_pv + WAVES);
	float* wave_sv = reinterpret_cast<float*>(wave_pf + WAVES);
	int* wave_sf = reinterpret_cast<int*>(wave_sv + WAVES);
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int T = S - K + 1;
	const int64_t i0 = (int64_t)blockIdx.x * T;
	const float* src = in + (size_t)blockIdx.y * Lin;
	const bool take_abs = flags & CONVASR_SLIDE_ABS, negate = flags & CONVASR_SLIDE_NEG;

	for (int l = tid; l < S; l += THREADS) {
		const int64_t j = i0 + l - pad;
		float v = -INFINITY;
		if (j >= 0 && j < Lin) {
			v = src[j];
			v = take_abs ? fabsf(v) : v;
			v = negate ? -v : v;
		}
		sm_span[l] = v;
	}
	__syncthreads();

	float a[DIAR_E];
#pragma unroll
	for (int e = 0; e < DIAR_E; ++e) a[e] = sm_span[tid * DIAR_E + e];
	const int r0 = (int)((i0 + (int64_t)tid * DIAR_E) % K);      // position of a[0] inside its block of K
	const int r_last = (int)((r0 + (int64_t)(DIAR_E - 1)) % K);  // of a[E - 1]

	// this thread's totals: (a block boundary was met, the maximum since it / over the whole chunk)
	float pv = -INFINITY, sv = -INFINITY;
	int pf = 0, sf = 0;
	{
		int r = r0;
#pragma unroll
		for (int e = 0; e < DIAR_E; ++e) {
			if (r == 0) { pv = a[e]; pf = 1; } else pv = fmaxf(pv, a[e]);
			r = r + 1 == K ? 0 : r + 1;
		}
		r = r_last;
#pragma unroll
		for (int e = DIAR_E - 1; e >= 0; --e) {
			if (r == K - 1) { sv = a[e]; sf = 1; } else sv = fmaxf(sv, a[e]);
			r = r == 0 ? K - 1 : r - 1;
		}
	}
	// segmented max-scan over the wave: (f1, v1) then (f2, v2) = (f1 | f2, f2 ? v2 : max(v1, v2)); prefix runs up the lanes, suffix down
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const float opv = __shfl_up(pv, d), osv = __shfl_down(sv, d);
		const int opf = __shfl_up(pf, d), osf = __shfl_down(sf, d);
		if (lane >= d) { pv = pf ? pv : fmaxf(pv, opv); pf |= opf; }
		if (lane + d < 64) { sv = sf ? sv : fmaxf(sv, osv); sf |= osf; }
	}
	if (lane == 63) { wave_pv[wave] = pv; wave_pf[wave] = pf; }
	if (lane == 0) { wave_sv[wave] = sv; wave_sf[wave] = sf; }
	// exclusive within the wave
	float epv = __shfl_up(pv, 1), esv = __shfl_down(sv, 1);
	int epf = __shfl_up(pf, 1), esf = __shfl_down(sf, 1);
	if (lane == 0) { epv = -INFINITY; epf = 0; }
	if (lane == 63) { esv = -INFINITY; esf = 0; }
	__syncthreads();  // wave totals visible; every thread has its a[] out of the span
	float cpv = -INFINITY, csv = -INFINITY;
	for (int w = 0; w < wave; ++w) cpv = wave_pf[w] ? wave_pv[w] : fmaxf(cpv, wave_pv[w]);
	for (int w = WAVES - 1; w > wave; --w) csv = wave_sf[w] ? wave_sv[w] : fmaxf(csv, wave_sv[w]);
	const float carry_p = epf ? epv : fmaxf(cpv, epv), carry_s = esf ? esv : fmaxf(csv, esv);

	{  // suffix maxima into the span, prefix maxima over a[]
		float run = carry_s;
		int r = r_last;
#pragma unroll
		for (int e = DIAR_E - 1; e >= 0; --e) {
			run = r == K - 1 ? a[e] : fmaxf(run, a[e]);
			sm_span[tid * DIAR_E + e] = run;
			r = r == 0 ? K - 1 : r - 1;
		}
		run = carry_p;
		r = r0;
#pragma unroll
		for (int e = 0; e < DIAR_E; ++e) {
			run = r == 0 ? a[e] : fmaxf(run, a[e]);
			a[e] = run;
			r = r + 1 == K ? 0 : r + 1;
		}
	}
	__syncthreads();
	// out[i] = max(h[i], g[i + K - 1]): word i of the span is read and written by the owner of g[i + K - 1] alone
#pragma unroll
	for (int e = 0; e < DIAR_E; ++e) {
		const int il = tid * DIAR_E + e - (K - 1);
		if (il >= 0) sm_span[il] = fmaxf(sm_span[il], a[e]);
	}
	__syncthreads();
	float* dst = out + (size_t)blockIdx.y * Lout;
	for (int l = tid; l < T; l += THREADS) {
		const int64_t i = i0 + l;
		if (i < Lout) dst[i] = negate ? -sm_span[l] : sm_span[l];
	}
}

int launch_slide_max(const float* in, float* out, int C, int64_t Lin, int K, int flags, hipStream_t stream) {
	const int64_t Lout = slide_out_len(Lin, K);
	const int threads = slide_threads(K);
	const int S = threads * DIAR_E, T = S - K + 1;
	const int64_t tiles = (Lout + T - 1) / T;
	const size_t lds = (size_t)S * 4 + 4 * (threads / 64) * 4;
	if (threads == DIAR_SMALL_THREADS) {
		hipLaunchKernelGGL(slide_max_kernel<DIAR_SMALL_THREADS>, dim3((unsigned)tiles, C), dim3(threads), lds, stream, in, out, Lin, Lout, K, K / 2, flags);
	} else {
		static unsigned long long set = 0;
		convasr_allow_160k_lds(reinterpret_cast<const void*>(slide_max_kernel<DIAR_LARGE_THREADS>), set);
		hipLaunchKernelGGL(slide_max_kernel<DIAR_LARGE_THREADS>, dim3((unsigned)tiles, C), dim3(threads), lds, stream, in, out, Lin, Lout, K, K / 2, flags);
	}
	CONVASR_CHECK_LAUNCH("sliding_max");
	return 0;
}

// ---------------------------------------------------------------------------------------------------------------- k-th smallest value

constexpr int KTH_BINS = 2048, KTH_THREADS = 256, KTH_PER_BLOCK = KTH_THREADS * 32;
constexpr int KTH_WORDS = 2 + 3 * KTH_BINS;  // per channel: the prefix found so far, the rank left inside it, three histograms

__global__ __launch_bounds__(KTH_THREADS) void kth_init_kernel(unsigned* ws, unsigned k) {
	unsigned* st = ws + (size_t)blockIdx.x * KTH_WORDS;
	for (int i = threadIdx.x; i < KTH_WORDS; i += KTH_THREADS) st[i] = i == 1 ? k : 0u;
}

template <int PASS>
__global__ __launch_bounds__(KTH_THREADS) void kth_hist_kernel(const float* __restrict__ x, unsigned* ws, int64_t L) {
	__shared__ unsigned hist[KTH_BINS];
	unsigned* st = ws + (size_t)blockIdx.y * KTH_WORDS;
	const unsigned prefix = st[0];
	const unsigned* src = reinterpret_cast<const unsigned*>(x) + (size_t)blockIdx.y * L;
	for (int i = threadIdx.x; i < KTH_BINS; i += KTH_THREADS) hist[i] = 0;
	__syncthreads();
	for (int64_t i = (int64_t)blockIdx.x * KTH_THREADS + threadIdx.x; i < L; i += (int64_t)gridDim.x * KTH_THREADS) {
		const unsigned u = src[i];
		if (PASS == 0) atomicAdd(&hist[u >> 21], 1u);
		else if (PASS == 1) { if ((u >> 21) == (prefix >> 21)) atomicAdd(&hist[(u >> 10) & 0x7FFu], 1u); }
		else { if ((u >> 10) == (prefix >> 10)) atomicAdd(&hist[u & 0x3FFu], 1u); }
	}
	__syncthreads();
	unsigned* g = st + 2 + PASS * KTH_BINS;
	for (int i = threadIdx.x; i < KTH_BINS; i += KTH_THREADS)
		if (hist[i]) atomicAdd(&g[i], hist[i]);
}

// exclusive prefix sum of one int per thread over a workgroup of THREADS (a multiple of 64, at most 1,024); *total = the sum
template <int THREADS>
__device__ __forceinline__ int block_exclusive_scan(int v, int* total) {
	__shared__ int wave_tot[THREADS / 64];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int inc = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const int o = __shfl_up(inc, d);
		if (lane >= d) inc += o;
	}
	__syncthreads();  // (a previous use of wave_tot is over)
	if (lane == 63) wave_tot[wave] = inc;
	__syncthreads();
	int base = 0, all = 0;
	for (int w = 0; w < THREADS / 64; ++w) {
		if (w < wave) base += wave_tot[w];
		all += wave_tot[w];
	}
	*total = all;
	return base + inc - v;
}

template <int PASS>
__global__ __launch_bounds__(KTH_THREADS) void kth_pick_kernel(unsigned* ws, float* out) {
	unsigned* st = ws + (size_t)blockIdx.x * KTH_WORDS;
	const unsigned* g = st + 2 + PASS * KTH_BINS;
	const unsigned prefix = st[0], krem = st[1];  // 1 <= krem <= the number of elements under the prefix
	constexpr int PER = KTH_BINS / KTH_THREADS;
	unsigned h[PER], sum = 0;
#pragma unroll
	for (int j = 0; j < PER; ++j) { h[j] = g[threadIdx.x * PER + j]; sum += h[j]; }
	int total;
	unsigned cum = (unsigned)block_exclusive_scan<KTH_THREADS>((int)sum, &total);  // (counts stay below 2^31)
#pragma unroll
	for (int j = 0; j < PER; ++j) {
		if (cum < krem && krem <= cum + h[j]) {
			const unsigned d = threadIdx.x * PER + j;
			const unsigned p = prefix | (PASS == 0 ? d << 21 : PASS == 1 ? d << 10 : d);
			st[0] = p;
			st[1] = krem - cum;
			if (PASS == 2) out[blockIdx.x] = __uint_as_float(p);
		}
		cum += h[j];
	}
}

int launch_kth(const float* x, float* out, unsigned* ws, int C, int64_t L, int64_t k, hipStream_t stream) {
	const int64_t want = (L + KTH_PER_BLOCK - 1) / KTH_PER_BLOCK;
	const unsigned blocks = (unsigned)(want < 1 ? 1 : want > 2048 ? 2048 : want);
	hipLaunchKernelGGL(kth_init_kernel, dim3(C), dim3(KTH_THREADS), 0, stream, ws, (unsigned)k);
	hipLaunchKernelGGL(kth_hist_kernel<0>, dim3(blocks, C), dim3(KTH_THREADS), 0, stream, x, ws, L);
	hipLaunchKernelGGL(kth_pick_kernel<0>, dim3(C), dim3(KTH_THREADS), 0, stream, ws, out);
	hipLaunchKernelGGL(kth_hist_kernel<1>, dim3(blocks, C), dim3(KTH_THREADS), 0, stream, x, ws, L);
	hipLaunchKernelGGL(kth_pick_kernel<1>, dim3(C), dim3(KTH_THREADS), 0, stream, ws, out);
	hipLaunchKernelGGL(kth_hist_kernel<2>, dim3(blocks, C), dim3(KTH_THREADS), 0, stream, x, ws, L);
	hipLaunchKernelGGL(kth_pick_kernel<2>, dim3(C), dim3(KTH_THREADS), 0, stream, ws, out);
	CONVASR_CHECK_LAUNCH("kth_value");
	return 0;
}

// ---------------------------------------------------------------------------------------------------------------- int32 prefix sums

constexpr int SCAN_THREADS = 256, SCAN_PER = 8, SCAN_TILE = SCAN_THREADS * SCAN_PER;  // 2,048 elements per workgroup

// +1 / 0 / -1 as channel 0 is above / equal to / below channel 1 (the sign of their difference: two distinct floats never subtract to 0)
struct SignOf {
	const float* d0;
	const float* d1;
	__device__ __forceinline__ int operator()(int64_t i) const {
		const float a = d0[i], b = d1[i];
		return a > b ? 1 : a < b ? -1 : 0;
	}
};
// 1 where element i starts a run (i >= 1 and x[i] != x[i - 1])
template <typename T>
struct BoundaryOf {
	const T* x;
	__device__ __forceinline__ int operator()(int64_t i) const { return i > 0 && x[i] != x[i - 1] ? 1 : 0; }
};

template <typename F>
__global__ __launch_bounds__(SCAN_THREADS) void scan_tile_sum_kernel(F f, int64_t n, int* sums) {
	const int64_t base = (int64_t)blockIdx.x * SCAN_TILE;
	int v = 0;
#pragma unroll
	for (int j = 0; j < SCAN_PER; ++j) {
		const int64_t i = base + j * SCAN_THREADS + threadIdx.x;
		if (i < n) v += f(i);
	}
	int total;
	block_exclusive_scan<SCAN_THREADS>(v, &total);
	if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// in place: sums[b] <- the sum of the tiles before b, sums[nb] <- the sum of all
__global__ __launch_bounds__(1024) void scan_sums_kernel(int* sums, int nb) {
	const int per = (nb + 1023) / 1024;
	const int lo = min(nb, (int)threadIdx.x * per), hi = min(nb, lo + per);
	int v = 0;
	for (int i = lo; i < hi; ++i) v += sums[i];
	int total;
	int run = block_exclusive_scan<1024>(v, &total);
	for (int i = lo; i < hi; ++i) {
		const int s = sums[i];
		sums[i] = run;
		run += s;
	}
	if (threadIdx.x == 0) sums[nb] = total;
}

// One tile in the order of scan_tile_sum_kernel: element (j, tid) is base + j * SCAN_THREADS + tid, so the lanes of a wave touch consecutive
// words in every load and store.  v[j] = f of it (0 past n), inc[j] = the sum of the tile's elements up to and including it: a shuffle scan
// per row and wave, then the 8 x 4 (row, wave) totals through LDS.
template <typename F>
__device__ __forceinline__ void scan_tile_rows(F f, int64_t base, int64_t n, int (&v)[SCAN_PER], int (&inc)[SCAN_PER]) {
	constexpr int WAVES = SCAN_THREADS / 64;
	__shared__ int row_tot[SCAN_PER * WAVES];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
	for (int j = 0; j < SCAN_PER; ++j) {
		const int64_t i = base + j * SCAN_THREADS + threadIdx.x;
		v[j] = i < n ? f(i) : 0;
		int x = v[j];
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const int o = __shfl_up(x, d);
			if (lane >= d) x += o;
		}
		inc[j] = x;
		if (lane == 63) row_tot[j * WAVES + wave] = x;
	}
	__syncthreads();
	int run = 0;
#pragma unroll
	for (int j = 0; j < SCAN_PER; ++j) {
#pragma unroll
		for (int w = 0; w < WAVES; ++w) {
			if (w == wave) inc[j] += run;
			run += row_tot[j * WAVES + w];
		}
	}
}

// the inclusive prefix sum of f over [0, n) -> P
template <typename F>
__global__ __launch_bounds__(SCAN_THREADS) void scan_write_kernel(F f, int64_t n, const int* sums, int* P) {
	const int64_t base = (int64_t)blockIdx.x * SCAN_TILE;
	int v[SCAN_PER], inc[SCAN_PER];
	scan_tile_rows(f, base, n, v, inc);
	const int before = sums[blockIdx.x];
#pragma unroll
	for (int j = 0; j < SCAN_PER; ++j) {
		const int64_t i = base + j * SCAN_THREADS + threadIdx.x;
		if (i < n) P[i] = before + inc[j];
	}
}

inline int scan_tiles(int64_t n) { return (int)((n + SCAN_TILE - 1) / SCAN_TILE); }
inline int64_t scan_sums_bytes(int64_t n) { return up256(((int64_t)scan_tiles(n) + 1) * 4); }

// ---------------------------------------------------------------------------------------------------------------- select_speaker

struct DiarGeom {
	int64_t L1, Ld, Le, Ls, L;
};
inline DiarGeom diar_geom(int64_t N, int Ksil, int Ksig, int Kspk) {
	DiarGeom g;
	g.L1 = slide_out_len(N, Ksig);
	g.Ld = slide_out_len(N, Ksil);
	g.Le = slide_out_len(g.Ld, Ksil);
	g.Ls = slide_out_len(g.L1, Kspk);
	g.L = g.Le < g.Ls ? g.Le : g.Ls;
	return g;
}

// sign of the zero-padded box sum around position i of the speaker sign, 0 outside [0, Ls)
__device__ __forceinline__ int box_sign(const int* __restrict__ P, int64_t i, int64_t L1, int64_t Ls, int K, int pad) {
	if (i < 0 || i >= Ls) return 0;
	int64_t lo = i - pad, hi = lo + K - 1;
	lo = lo < 0 ? 0 : lo;
	hi = hi > L1 - 1 ? L1 - 1 : hi;
	const int s = P[hi] - (lo > 0 ? P[lo - 1] : 0);
	return s > 0 ? 1 : s < 0 ? -1 : 0;
}

__global__ __launch_bounds__(256) void diar_combine_kernel(const float* __restrict__ eroded, const float* __restrict__ kth, const int* __restrict__ P,
                                                           float* __restrict__ speaker_id, uint8_t* __restrict__ mask, DiarGeom g, int Kspk, float abs_thr,
                                                           float rel_thr, float eps) {
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= g.L) return;
	const int pad = Kspk / 2;
	int b = box_sign(P, i, g.L1, g.Ls, Kspk, pad);
	if (b == 0) {  // the 3-tap repair: a 0 between a +1 and a -1 (zero outside the array) becomes +1
		const int l = box_sign(P, i - 1, g.L1, g.Ls, Kspk, pad), r = box_sign(P, i + 1, g.L1, g.Ls, Kspk, pad);
		if (l != 0 && l + r == 0) b = 1;
	}
	const float e0 = eroded[i], e1 = eroded[(size_t)g.Le + i];
	const bool s0 = e0 < abs_thr || e0 / (eps + kth[0]) < rel_thr;
	const bool s1 = e1 < abs_thr || e1 / (eps + kth[1]) < rel_thr;
	const bool both = s0 && s1;
	speaker_id[i] = both || b == 0 ? 0.f : b > 0 ? 1.f : 2.f;
	mask[i] = both;
	mask[(size_t)g.L + i] = !s0 && b == 1;
	mask[2 * (size_t)g.L + i] = !s1 && b == -1;
}

struct DiarWs {
	int64_t smoothed, dilated, eroded, prefix, sums, kth, kth_out, total;
};
inline DiarWs diar_ws(const DiarGeom& g) {
	DiarWs w;
	int64_t at = 0;
	w.smoothed = at; at += up256(2 * g.L1 * 4);
	w.dilated = at; at += up256(2 * g.Ld * 4);
	w.eroded = at; at += up256(2 * g.Le * 4);
	w.prefix = at; at += up256(g.L1 * 4);
	w.sums = at; at += scan_sums_bytes(g.L1);
	w.kth = at; at += up256(2 * KTH_WORDS * 4);
	w.kth_out = at; at += 256;
	w.total = at;
	return w;
}

inline bool diar_shape_ok(int64_t N, int Ksil, int Ksig, int Kspk) {
	return N >= 1 && N <= DIAR_MAX_LEN && Ksil >= 1 && Ksil <= DIAR_MAX_K && Ksig >= 1 && Ksig <= DIAR_MAX_K && Kspk >= 1 && Kspk <= DIAR_MAX_K;
}

template <typename F>
int launch_scan(F f, int64_t n, int* sums, int* P, hipStream_t stream) {
	const int nb = scan_tiles(n);
	hipLaunchKernelGGL(scan_tile_sum_kernel<F>, dim3(nb), dim3(SCAN_THREADS), 0, stream, f, n, sums);
	hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, stream, sums, nb);
	hipLaunchKernelGGL(scan_write_kernel<F>, dim3(nb), dim3(SCAN_THREADS), 0, stream, f, n, (const int*)sums, P);
	CONVASR_CHECK_LAUNCH("prefix sum");
	return 0;
}

// ---------------------------------------------------------------------------------------------------------------- run-length encoding

// starts[1 + (boundaries before i)] = i for every boundary i; starts[0] = 0
template <typename F>
__global__ __launch_bounds__(SCAN_THREADS) void rle_starts_kernel(F f, int64_t n, int64_t runs, const int* sums, int64_t* starts) {
	const int64_t base = (int64_t)blockIdx.x * SCAN_TILE;
	int v[SCAN_PER], inc[SCAN_PER];
	scan_tile_rows(f, base, n, v, inc);
	const int64_t before = sums[blockIdx.x];
#pragma unroll
	for (int j = 0; j < SCAN_PER; ++j) {
		const int64_t at = before + inc[j];  // boundaries up to and including this one = its slot in starts
		if (v[j] && at < runs) starts[at] = base + j * SCAN_THREADS + threadIdx.x;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) starts[0] = 0;
}

template <typename T>
__global__ __launch_bounds__(256) void rle_finish_kernel(const T* __restrict__ x, int64_t n, int64_t runs, const int64_t* __restrict__ starts,
                                                         int64_t* __restrict__ lengths, T* __restrict__ values) {
	const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (r >= runs) return;
	const int64_t s = starts[r], e = r + 1 < runs ? starts[r + 1] : n;
	lengths[r] = e - s;
	values[r] = x[s];
}

template <typename T>
int rle_count(const void* x, int64_t n, int* sums, hipStream_t stream) {
	const BoundaryOf<T> f{static_cast<const T*>(x)};
	const int nb = scan_tiles(n);
	hipLaunchKernelGGL(scan_tile_sum_kernel<BoundaryOf<T>>, dim3(nb), dim3(SCAN_THREADS), 0, stream, f, n, sums);
	hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, stream, sums, nb);
	CONVASR_CHECK_LAUNCH("rle1d_count");
	return 0;
}

template <typename T>
int rle_write(const void* x, int64_t n, int64_t runs, const int* sums, int64_t* starts, int64_t* lengths, void* values, hipStream_t stream) {
	const BoundaryOf<T> f{static_cast<const T*>(x)};
	hipLaunchKernelGGL(rle_starts_kernel<BoundaryOf<T>>, dim3(scan_tiles(n)), dim3(SCAN_THREADS), 0, stream, f, n, runs, sums, starts);
	hipLaunchKernelGGL(rle_finish_kernel<T>, dim3((unsigned)((runs + 255) / 256)), dim3(256), 0, stream, static_cast<const T*>(x), n, runs,
	                   (const int64_t*)starts, lengths, static_cast<T*>(values));
	CONVASR_CHECK_LAUNCH("rle1d_write");
	return 0;
}

inline bool rle_type_ok(int elem_bytes, int is_float) {
	return is_float ? elem_bytes == 4 : (elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8);
}

// ---------------------------------------------------------------------------------------------------------------- speaker error counts

constexpr int SPK_MAX_PERMS = CONVASR_SPEAKER_MAX_PERMS, SPK_COUNTS = 7, SPK_THREADS = 256;
struct SpkPerms {
	int n;
	int row[SPK_MAX_PERMS][2];  // the rows of the hypothesis mask that stand for speakers 1 and 2
};

__global__ __launch_bounds__(SPK_THREADS) void spk_err_kernel(const uint8_t* __restrict__ ref, const uint8_t* __restrict__ hyp, int64_t n, SpkPerms perms,
                                                              unsigned long long* partial) {
	__shared__ unsigned long long acc[SPK_MAX_PERMS * SPK_COUNTS];
	for (int j = threadIdx.x; j < SPK_MAX_PERMS * SPK_COUNTS; j += SPK_THREADS) acc[j] = 0;
	__syncthreads();
	unsigned cnt[SPK_MAX_PERMS][SPK_COUNTS] = {};
	for (int64_t i = (int64_t)blockIdx.x * SPK_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SPK_THREADS) {
		const bool r1 = ref[(size_t)n + i], r2 = ref[2 * (size_t)n + i];
		const bool h[3] = {hyp[i] != 0, hyp[(size_t)n + i] != 0, hyp[2 * (size_t)n + i] != 0};
		const bool kept = r1 != r2;
#pragma unroll
		for (int p = 0; p < SPK_MAX_PERMS; ++p) {
			if (p < perms.n) {
				const int a = perms.row[p][0], b = perms.row[p][1];
				const bool h1 = a == 0 ? h[0] : a == 1 ? h[1] : h[2], h2 = b == 0 ? h[0] : b == 1 ? h[1] : h[2];
				const bool mismatch = r1 != h1 || r2 != h2;
				cnt[p][0] += mismatch && kept;                             // mismatches where exactly one reference speaker talks
				cnt[p][1] += mismatch;                                     // mismatches over every position
				cnt[p][2] += (h1 && r2 && !r1) || (h2 && r1 && !r2);       // confusion
				cnt[p][3] += (h1 || h2) && !r1 && !r2;                     // false alarm
				cnt[p][4] += !h1 && !h2 && (r1 || r2);                     // miss
				cnt[p][5] += kept;                                         // positions where exactly one reference speaker talks
				cnt[p][6] += r1 || r2;                                     // total: positions where a reference speaker talks
			}
		}
	}
#pragma unroll
	for (int p = 0; p < SPK_MAX_PERMS; ++p) {
#pragma unroll
		for (int c = 0; c < SPK_COUNTS; ++c) {
			unsigned v = cnt[p][c];
#pragma unroll
			for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
			if ((threadIdx.x & 63) == 0 && v) atomicAdd(&acc[p * SPK_COUNTS + c], (unsigned long long)v);
		}
	}
	__syncthreads();
	for (int j = threadIdx.x; j < SPK_MAX_PERMS * SPK_COUNTS; j += SPK_THREADS) partial[(size_t)blockIdx.x * SPK_MAX_PERMS * SPK_COUNTS + j] = acc[j];
}

__global__ __launch_bounds__(64) void spk_err_finish_kernel(const unsigned long long* __restrict__ partial, int blocks, int n_out, int64_t* counts) {
	const int j = threadIdx.x;
	if (j >= n_out) return;
	unsigned long long s = 0;
	for (int b = 0; b < blocks; ++b) s += partial[(size_t)b * SPK_MAX_PERMS * SPK_COUNTS + j];
	counts[j] = (int64_t)s;
}

inline int spk_blocks(int64_t n) {
	const int64_t want = (n + SPK_THREADS * 16 - 1) / (SPK_THREADS * 16);
	return (int)(want < 1 ? 1 : want > 1024 ? 1024 : want);
}

}  // namespace

// ==================================================================================================================== C ABI

extern "C" int64_t convasr_sliding_max_out_len(int64_t Lin, int K) {
	if (Lin < 1 || Lin > DIAR_MAX_LEN || K < 1 || K > DIAR_MAX_K) {
		convasr_fail(CONVASR_EINVAL, "sliding_max_out_len: length %lld in [1, %lld] and window %d in [1, %d] expected", (long long)Lin, (long long)DIAR_MAX_LEN, K,
		             DIAR_MAX_K);
		return -1;
	}
	return slide_out_len(Lin, K);
}

extern "C" int convasr_sliding_max_tile(int K) {
	if (K < 1 || K > DIAR_MAX_K) return convasr_fail(CONVASR_EINVAL, "sliding_max_tile: window %d, 1 to %d expected", K, DIAR_MAX_K);
	return slide_threads(K) * DIAR_E - K + 1;
}

extern "C" int convasr_sliding_max(const float* in, float* out, int C, int64_t Lin, int K, int flags, void* stream) {
	CONVASR_CHECK_ARG(in && out, "sliding_max: NULL pointer");
	CONVASR_CHECK_ARG(C >= 1 && C <= 65535, "sliding_max: %d rows, 1 to 65535 expected", C);
	CONVASR_CHECK_ARG(Lin >= 1 && Lin <= DIAR_MAX_LEN, "sliding_max: length %lld, 1 to %lld expected", (long long)Lin, (long long)DIAR_MAX_LEN);
	CONVASR_CHECK_ARG(K >= 1 && K <= DIAR_MAX_K, "sliding_max: window %d, 1 to %d expected", K, DIAR_MAX_K);
	CONVASR_CHECK_ARG((flags & ~(CONVASR_SLIDE_ABS | CONVASR_SLIDE_NEG)) == 0, "sliding_max: unknown flags %d", flags);
	return launch_slide_max(in, out, C, Lin, K, flags, (hipStream_t)stream);
}

extern "C" int64_t convasr_kth_value_workspace_bytes(int C) {
	if (C < 1 || C > 65535) {
		convasr_fail(CONVASR_EINVAL, "kth_value_workspace_bytes: %d rows, 1 to 65535 expected", C);
		return -1;
	}
	return up256((int64_t)C * KTH_WORDS * 4);
}

extern "C" int convasr_kth_value(const float* x, float* out, void* workspace, int64_t workspace_bytes, int C, int64_t L, int64_t k, void* stream) {
	CONVASR_CHECK_ARG(x && out && workspace, "kth_value: NULL pointer");
	CONVASR_CHECK_ARG(C >= 1 && C <= 65535, "kth_value: %d rows, 1 to 65535 expected", C);
	CONVASR_CHECK_ARG(L >= 1 && L <= DIAR_MAX_LEN + 1, "kth_value: length %lld, 1 to %lld expected", (long long)L, (long long)DIAR_MAX_LEN + 1);
	CONVASR_CHECK_ARG(k >= 1 && k <= L, "kth_value: k = %lld, 1 to the length %lld expected", (long long)k, (long long)L);
	CONVASR_CHECK_ARG(workspace_bytes >= convasr_kth_value_workspace_bytes(C), "kth_value: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
	                  (long long)convasr_kth_value_workspace_bytes(C));
	CONVASR_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "kth_value: workspace must be 16-byte aligned");
	return launch_kth(x, out, static_cast<unsigned*>(workspace), C, L, k, (hipStream_t)stream);
}

extern "C" int64_t convasr_sign_prefix_sum_workspace_bytes(int64_t L) {
	if (L < 1 || L > DIAR_MAX_LEN + 1) {
		convasr_fail(CONVASR_EINVAL, "sign_prefix_sum_workspace_bytes: length %lld, 1 to %lld expected", (long long)L, (long long)DIAR_MAX_LEN + 1);
		return -1;
	}
	return scan_sums_bytes(L);
}

extern "C" int convasr_scan_tile(void) { return SCAN_TILE; }

extern "C" int convasr_sign_prefix_sum(const float* d, int32_t* prefix, void* workspace, int64_t workspace_bytes, int64_t L, void* stream) {
	CONVASR_CHECK_ARG(d && prefix && workspace, "sign_prefix_sum: NULL pointer");
	CONVASR_CHECK_ARG(L >= 1 && L <= DIAR_MAX_LEN + 1, "sign_prefix_sum: length %lld, 1 to %lld expected", (long long)L, (long long)DIAR_MAX_LEN + 1);
	CONVASR_CHECK_ARG(workspace_bytes >= scan_sums_bytes(L), "sign_prefix_sum: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
	                  (long long)scan_sums_bytes(L));
	return launch_scan(SignOf{d, d + L}, L, static_cast<int*>(workspace), prefix, (hipStream_t)stream);
}

extern "C" int64_t convasr_select_speaker_out_len(int64_t N, int kernel_size_smooth_silence, int kernel_size_smooth_signal, int kernel_size_smooth_speaker) {
	if (!diar_shape_ok(N, kernel_size_smooth_silence, kernel_size_smooth_signal, kernel_size_smooth_speaker)) {
		convasr_fail(CONVASR_EINVAL, "select_speaker_out_len: N %lld in [1, %lld] and kernel sizes (%d, %d, %d) in [1, %d] expected", (long long)N,
		             (long long)DIAR_MAX_LEN, kernel_size_smooth_silence, kernel_size_smooth_signal, kernel_size_smooth_speaker, DIAR_MAX_K);
		return -1;
	}
	return diar_geom(N, kernel_size_smooth_silence, kernel_size_smooth_signal, kernel_size_smooth_speaker).L;
}

extern "C" int64_t convasr_select_speaker_workspace_bytes(int64_t N, int kernel_size_smooth_silence, int kernel_size_smooth_signal,
                                                          int kernel_size_smooth_speaker) {
	if (!diar_shape_ok(N, kernel_size_smooth_silence, kernel_size_smooth_signal, kernel_size_smooth_speaker)) {
		convasr_fail(CONVASR_EINVAL, "select_speaker_workspace_bytes: N %lld in [1, %lld] and kernel sizes (%d, %d, %d) in [1, %d] expected", (long long)N,
		             (long long)DIAR_MAX_LEN, kernel_size_smooth_silence, kernel_size_smooth_signal, kernel_size_smooth_speaker, DIAR_MAX_K);
		return -1;
	}
	return diar_ws(diar_geom(N, kernel_size_smooth_silence, kernel_size_smooth_signal, kernel_size_smooth_speaker)).total;
}

extern "C" int convasr_select_speaker(const float* signal, float* speaker_id, uint8_t* mask, void* workspace, int64_t workspace_bytes, int64_t N,
                                      int kernel_size_smooth_silence, int kernel_size_smooth_signal, int kernel_size_smooth_speaker,
                                      float silence_absolute_threshold, float silence_relative_threshold, float eps, int64_t k, void* stream) {
	const int Ksil = kernel_size_smooth_silence, Ksig = kernel_size_smooth_signal, Kspk = kernel_size_smooth_speaker;
	CONVASR_CHECK_ARG(signal && speaker_id && mask && workspace, "select_speaker: NULL pointer");
	CONVASR_CHECK_ARG(N >= 1 && N <= DIAR_MAX_LEN, "select_speaker: N = %lld samples per channel, 1 to %lld expected", (long long)N, (long long)DIAR_MAX_LEN);
	CONVASR_CHECK_ARG(diar_shape_ok(N, Ksil, Ksig, Kspk), "select_speaker: kernel sizes (%d, %d, %d) must lie in [1, %d]", Ksil, Ksig, Kspk, DIAR_MAX_K);
	const DiarGeom g = diar_geom(N, Ksil, Ksig, Kspk);
	CONVASR_CHECK_ARG(k >= 1 && k <= g.L1, "select_speaker: k = int(normalization_percentile * %lld) = %lld, 1 to %lld expected", (long long)g.L1,
	                  (long long)k, (long long)g.L1);
	const DiarWs w = diar_ws(g);
	CONVASR_CHECK_ARG(workspace_bytes >= w.total, "select_speaker: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)w.total);
	CONVASR_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "select_speaker: workspace must be 16-byte aligned");
	char* base = static_cast<char*>(workspace);
	float* smoothed = reinterpret_cast<float*>(base + w.smoothed);
	float* dilated = reinterpret_cast<float*>(base + w.dilated);
	float* eroded = reinterpret_cast<float*>(base + w.eroded);
	int* prefix = reinterpret_cast<int*>(base + w.prefix);
	int* sums = reinterpret_cast<int*>(base + w.sums);
	unsigned* kth_ws = reinterpret_cast<unsigned*>(base + w.kth);
	float* kth = reinterpret_cast<float*>(base + w.kth_out);
	hipStream_t s = (hipStream_t)stream;
	int rc;
	if ((rc = launch_slide_max(signal, smoothed, 2, N, Ksig, CONVASR_SLIDE_ABS, s))) return rc;
	if ((rc = launch_slide_max(signal, dilated, 2, N, Ksil, CONVASR_SLIDE_ABS, s))) return rc;
	if ((rc = launch_slide_max(dilated, eroded, 2, g.Ld, Ksil, CONVASR_SLIDE_NEG, s))) return rc;
	if ((rc = launch_kth(smoothed, kth, kth_ws, 2, g.L1, k, s))) return rc;
	if ((rc = launch_scan(SignOf{smoothed, smoothed + g.L1}, g.L1, sums, prefix, s))) return rc;
	hipLaunchKernelGGL(diar_combine_kernel, dim3((unsigned)((g.L + 255) / 256)), dim3(256), 0, s, (const float*)eroded, (const float*)kth, (const int*)prefix,
	                   speaker_id, mask, g, Kspk, silence_absolute_threshold, silence_relative_threshold, eps);
	CONVASR_CHECK_LAUNCH("select_speaker");
	return 0;
}

extern "C" int64_t convasr_rle1d_workspace_bytes(int64_t n) {
	if (n < 1 || n > CONVASR_RLE_MAX_LEN) {
		convasr_fail(CONVASR_EINVAL, "rle1d_workspace_bytes: %lld elements, 1 to %lld expected", (long long)n, (long long)CONVASR_RLE_MAX_LEN);
		return -1;
	}
	return scan_sums_bytes(n);
}

extern "C" int convasr_rle1d_count(const void* x, int elem_bytes, int is_float, int64_t n, void* workspace, int64_t workspace_bytes, void* stream) {
	CONVASR_CHECK_ARG(x && workspace, "rle1d_count: NULL pointer");
	CONVASR_CHECK_ARG(n >= 1 && n <= CONVASR_RLE_MAX_LEN, "rle1d_count: %lld elements, 1 to %lld expected", (long long)n, (long long)CONVASR_RLE_MAX_LEN);
	CONVASR_CHECK_ARG(rle_type_ok(elem_bytes, is_float), "rle1d_count: elements of %d bytes (float: %d); integers of 1, 2, 4, 8 bytes and fp32 expected", elem_bytes,
	                  is_float);
	CONVASR_CHECK_ARG(workspace_bytes >= scan_sums_bytes(n), "rle1d_count: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
	                  (long long)scan_sums_bytes(n));
	int* sums = static_cast<int*>(workspace);
	hipStream_t s = (hipStream_t)stream;
	if (is_float) return rle_count<float>(x, n, sums, s);
	return elem_bytes == 1 ? rle_count<uint8_t>(x, n, sums, s) : elem_bytes == 2 ? rle_count<uint16_t>(x, n, sums, s)
	     : elem_bytes == 4 ? rle_count<uint32_t>(x, n, sums, s) : rle_count<uint64_t>(x, n, sums, s);
}

extern "C" int64_t convasr_rle1d_count_offset(int64_t n) {
	if (n < 1 || n > CONVASR_RLE_MAX_LEN) {
		convasr_fail(CONVASR_EINVAL, "rle1d_count_offset: %lld elements, 1 to %lld expected", (long long)n, (long long)CONVASR_RLE_MAX_LEN);
		return -1;
	}
	return (int64_t)scan_tiles(n) * 4;
}

extern "C" int convasr_rle1d_write(const void* x, int elem_bytes, int is_float, int64_t n, const void* workspace, int64_t workspace_bytes, int64_t runs,
                                   int64_t* starts, int64_t* lengths, void* values, void* stream) {
	CONVASR_CHECK_ARG(x && workspace && starts && lengths && values, "rle1d_write: NULL pointer");
	CONVASR_CHECK_ARG(n >= 1 && n <= CONVASR_RLE_MAX_LEN, "rle1d_write: %lld elements, 1 to %lld expected", (long long)n, (long long)CONVASR_RLE_MAX_LEN);
	CONVASR_CHECK_ARG(runs >= 1 && runs <= n, "rle1d_write: %lld runs of %lld elements", (long long)runs, (long long)n);
	CONVASR_CHECK_ARG(rle_type_ok(elem_bytes, is_float), "rle1d_write: elements of %d bytes (float: %d); integers of 1, 2, 4, 8 bytes and fp32 expected", elem_bytes,
	                  is_float);
	CONVASR_CHECK_ARG(workspace_bytes >= scan_sums_bytes(n), "rle1d_write: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
	                  (long long)scan_sums_bytes(n));
	const int* sums = static_cast<const int*>(workspace);
	hipStream_t s = (hipStream_t)stream;
	if (is_float) return rle_write<float>(x, n, runs, sums, starts, lengths, values, s);
	return elem_bytes == 1 ? rle_write<uint8_t>(x, n, runs, sums, starts, lengths, values, s)
	     : elem_bytes == 2 ? rle_write<uint16_t>(x, n, runs, sums, starts, lengths, values, s)
	     : elem_bytes == 4 ? rle_write<uint32_t>(x, n, runs, sums, starts, lengths, values, s)
	                       : rle_write<uint64_t>(x, n, runs, sums, starts, lengths, values, s);
}

extern "C" int64_t convasr_speaker_error_counts_workspace_bytes(int64_t n) {
	if (n < 1 || n > CONVASR_RLE_MAX_LEN) {
		convasr_fail(CONVASR_EINVAL, "speaker_error_counts_workspace_bytes: %lld positions, 1 to %lld expected", (long long)n, (long long)CONVASR_RLE_MAX_LEN);
		return -1;
	}
	return up256((int64_t)spk_blocks(n) * SPK_MAX_PERMS * SPK_COUNTS * 8);
}

extern "C" int convasr_speaker_error_counts(const uint8_t* ref_mask, const uint8_t* hyp_mask, const int32_t* perms, int n_perms, int64_t n, int64_t* counts,
                                            void* workspace, int64_t workspace_bytes, void* stream) {
	CONVASR_CHECK_ARG(ref_mask && hyp_mask && perms && counts && workspace, "speaker_error_counts: NULL pointer");
	CONVASR_CHECK_ARG(n >= 1 && n <= CONVASR_RLE_MAX_LEN, "speaker_error_counts: %lld positions, 1 to %lld expected", (long long)n, (long long)CONVASR_RLE_MAX_LEN);
	CONVASR_CHECK_ARG(n_perms >= 1 && n_perms <= SPK_MAX_PERMS, "speaker_error_counts: %d permutations, 1 to %d expected", n_perms, SPK_MAX_PERMS);
	SpkPerms p;
	p.n = n_perms;
	for (int i = 0; i < SPK_MAX_PERMS; ++i) p.row[i][0] = p.row[i][1] = 0;
	for (int i = 0; i < n_perms; ++i) {
		for (int j = 1; j < 3; ++j) {
			CONVASR_CHECK_ARG(perms[3 * i + j] >= 0 && perms[3 * i + j] <= 2, "speaker_error_counts: mapping %d names row %d of a 3-row mask", i, perms[3 * i + j]);
			p.row[i][j - 1] = perms[3 * i + j];
		}
	}
	CONVASR_CHECK_ARG(workspace_bytes >= convasr_speaker_error_counts_workspace_bytes(n), "speaker_error_counts: workspace of %lld bytes, %lld needed",
	                  (long long)workspace_bytes, (long long)convasr_speaker_error_counts_workspace_bytes(n));
	CONVASR_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "speaker_error_counts: workspace must be 8-byte aligned");
	const int blocks = spk_blocks(n);
	unsigned long long* partial = static_cast<unsigned long long*>(workspace);
	hipLaunchKernelGGL(spk_err_kernel, dim3(blocks), dim3(SPK_THREADS), 0, (hipStream_t)stream, ref_mask, hyp_mask, n, p, partial);
	hipLaunchKernelGGL(spk_err_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const unsigned long long*)partial, blocks, n_perms * SPK_COUNTS, counts);
	CONVASR_CHECK_LAUNCH("speaker_error_counts");
	return 0;
}
