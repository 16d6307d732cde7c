// Speech-activity detection and the cutting of a long recording into utterance-sized segments (convasr_amd/vad.py, transcribe.transcribe_long).
// The reference's vad.py wraps webrtcvad, a C library this project does not have; the detector here is DEFINED BY THIS PROJECT
// (include/convasr_hip.h) and unpinned against it.  Every result is exact -- maxima, comparisons, integers, one IEEE add and divide per frame
// -- so no result depends on the launch geometry.
//
// frame_peak: the one pass over the samples.  A group of 1 to 64 lanes owns a frame; the lanes walk it in 16-byte loads between a scalar head
//   (up to the first 16-byte boundary: the row of channel c starts at c N elements, unaligned for odd N) and a scalar tail, then reduce over the
//   group with shuffles.  The group width grows with the frame length so that a lane reads about 16 samples.
// vad_frames: one workgroup per channel walks the frame array in tiles of VF_TILE and carries its scan state from tile to tile.  Each smoothing
//   step is two sweeps: ascending, "the last frame <= i of the wanted kind" (a running maximum of indices) into the workspace; descending, "the
//   next frame >= i of that kind" (a running minimum), combined at once with the stored value into the step's result, in place.
// vad_segments_count / _write: two calls around one host read, as rle1d.  count marks where segments start -- the first frame of every run,
//   and for a run longer than max_frames the cut points, a wave per run taking the lowest index of the smallest peak in the window -- and
//   leaves their number per channel; write ranks the marks with a prefix sum and writes (channel, first, count).
// gather_segments: B segments into a zero-padded (B, Tpad) fp32 batch in one launch.
#include "common.h"

#define VAD_MAX_CHANNELS 8
#define VAD_MAX_LEN (1ll << 28)
#define VAD_MAX_FRAME 65536
#define FP_THREADS 256
#define VF_THREADS 1024
#define VF_PER 8
#define VF_TILE (VF_THREADS * VF_PER)
#define GS_THREADS 256

static inline int64_t vad_up256(int64_t n) { return (n + 255) / 256 * 256; }

// ---------------------------------------------------------------------------------------------------------------- frame peaks

// lanes per frame: the power of two >= F / 16, 1 to 64
static int fp_group(int F) {
	int g = 1;
	while (g < 64 && g * 16 < F) g <<= 1;
	return g;
}

template <typename T> struct FpElem;
template <> struct FpElem<float> {
	typedef float acc_t;
	static constexpr int V = 4;
	__device__ static __forceinline__ float one(const float* p) { return fabsf(*p); }
	__device__ static __forceinline__ float vec(const float* p) {
		const float4 v = *reinterpret_cast<const float4*>(p);
		return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
	}
	__device__ static __forceinline__ float join(float a, float b) { return fmaxf(a, b); }
	__device__ static __forceinline__ float finish(float a) { return a; }
};
template <> struct FpElem<int16_t> {
	typedef int acc_t;
	static constexpr int V = 8;
	__device__ static __forceinline__ int one(const int16_t* p) { return abs((int)*p); }
	__device__ static __forceinline__ int vec(const int16_t* p) {
		const uint4 v = *reinterpret_cast<const uint4*>(p);
		const unsigned w[4] = {v.x, v.y, v.z, v.w};
		int m = 0;
#pragma unroll
		for (int i = 0; i < 4; ++i) m = max(m, max(abs((int)(int16_t)(w[i] & 0xffffu)), abs((int)(int16_t)(w[i] >> 16))));
		return m;
	}
	__device__ static __forceinline__ int join(int a, int b) { return max(a, b); }
	__device__ static __forceinline__ float finish(int a) { return __fdiv_rn((float)a, 32767.f); }  // the s2f rule: one correctly rounded divide, of the maximum of |int32(x)|
};

// peaks[c][f] over all C * nF frames; G lanes per frame, FP_THREADS / G frames per workgroup and step
template <typename T>
__global__ __launch_bounds__(FP_THREADS) void frame_peak_kernel(const T* __restrict__ x, float* __restrict__ peaks, int64_t N, int F, int64_t nF, int64_t frames, int G) {
	typedef FpElem<T> E;
	constexpr int V = E::V;
	const int lane = threadIdx.x & (G - 1), per = FP_THREADS / G;
	for (int64_t g0 = (int64_t)blockIdx.x * per; g0 < frames; g0 += (int64_t)gridDim.x * per) {
		const int64_t g = g0 + threadIdx.x / G;  // (uniform over the G lanes of a group, so the shuffles below stay inside lanes that took the same branch)
		typename E::acc_t m = 0;
		if (g < frames) {
			const int64_t c = g / nF, f = g - c * nF, start = f * (int64_t)F;
			const int len = (int)min((int64_t)F, N - start);  // >= 1: f < nF = ceil(N / F)
			const T* p = x + c * N + start;
			int head = (int)(((16 - ((uintptr_t)p & 15)) & 15) / sizeof(T));  // elements up to the first 16-byte boundary (p is aligned to its element)
			head = min(head, len);
			const int nvec = (len - head) / V, tail0 = head + nvec * V;
			for (int i = lane; i < head; i += G) m = E::join(m, E::one(p + i));
			for (int i = lane; i < nvec; i += G) m = E::join(m, E::vec(p + head + i * V));
			for (int i = tail0 + lane; i < len; i += G) m = E::join(m, E::one(p + i));
		}
		for (int o = G >> 1; o > 0; o >>= 1) m = E::join(m, __shfl_xor(m, o, 64));
		if (g < frames && lane == 0) peaks[g] = E::finish(m);
	}
}

static int vad_check_signal(const char* name, int dtype, int C, int64_t N) {
	CONVASR_CHECK_ARG(dtype == CONVASR_I16 || dtype == CONVASR_F32, "%s: signal dtype %d is neither CONVASR_I16 nor CONVASR_F32", name, dtype);
	CONVASR_CHECK_ARG(C >= 1 && C <= VAD_MAX_CHANNELS, "%s: %d channels, 1 to %d expected", name, C, VAD_MAX_CHANNELS);
	CONVASR_CHECK_ARG(N >= 1 && N <= VAD_MAX_LEN, "%s: %lld samples per channel, 1 to 2^28 expected", name, (long long)N);
	return 0;
}

extern "C" int convasr_frame_peak_tile(int frame_len) {
	if (frame_len < 1 || frame_len > VAD_MAX_FRAME) return convasr_fail(CONVASR_EINVAL, "frame_peak_tile: frame length %d, 1 to %d expected", frame_len, VAD_MAX_FRAME);
	return FP_THREADS / fp_group(frame_len);
}

extern "C" int convasr_frame_peak(const void* signal, int dtype, int C, int64_t N, int frame_len, float* peaks, void* stream) {
	if (const int e = vad_check_signal("frame_peak", dtype, C, N)) return e;
	CONVASR_CHECK_ARG(frame_len >= 1 && frame_len <= VAD_MAX_FRAME, "frame_peak: frame length %d, 1 to %d expected", frame_len, VAD_MAX_FRAME);
	CONVASR_CHECK_ARG(signal && peaks, "frame_peak: NULL pointer");
	CONVASR_CHECK_ARG(((uintptr_t)signal & (dtype == CONVASR_I16 ? 1 : 3)) == 0, "frame_peak: signal is not aligned to its element size");
	const int G = fp_group(frame_len), per = FP_THREADS / G;
	const int64_t nF = ceil_div64(N, frame_len), frames = nF * C, want = ceil_div64(frames, per), cap = (int64_t)convasr_cu_count() * 8;  // (8 workgroups of 4 waves fill a compute unit; more frames than that are walked in a stride loop)
	const unsigned blocks = (unsigned)(want < cap ? want : cap);
	if (dtype == CONVASR_I16) hipLaunchKernelGGL(frame_peak_kernel<int16_t>, dim3(blocks), dim3(FP_THREADS), 0, (hipStream_t)stream, (const int16_t*)signal, peaks, N, frame_len, nF, frames, G);
	else hipLaunchKernelGGL(frame_peak_kernel<float>, dim3(blocks), dim3(FP_THREADS), 0, (hipStream_t)stream, (const float*)signal, peaks, N, frame_len, nF, frames, G);
	CONVASR_CHECK_LAUNCH("frame_peak");
	return 0;
}

// ---------------------------------------------------------------------------------------------------------------- raw mask and smoothing

// exclusive scan over the workgroup's threads, in thread order, of a running maximum (MX) or minimum; *total = over all threads
template <bool MX>
__device__ __forceinline__ int vf_exclusive(int v, int ident, int* total, int* wave_tot) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int inc = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const int o = __shfl_up(inc, d, 64);
		if (lane >= d) inc = MX ? max(inc, o) : min(inc, o);
	}
	__syncthreads();  // (a previous use of wave_tot is over)
	if (lane == 63) wave_tot[wave] = inc;
	__syncthreads();
	int base = ident, all = ident;
#pragma unroll
	for (int w = 0; w < VF_THREADS / 64; ++w) {
		const int t = wave_tot[w];
		if (w < wave) base = MX ? max(base, t) : min(base, t);
		all = MX ? max(all, t) : min(all, t);
	}
	*total = all;
	int before = __shfl_up(inc, 1, 64);
	if (lane == 0) before = ident;
	return MX ? max(base, before) : min(base, before);
}

// prev[i] = the largest j <= i with m[j] == want, -1 where there is none
__device__ void vf_prev_sweep(const uint8_t* m, int want, int n, int* prev, int* wave_tot) {
	int carry = -1;
	for (int t0 = 0; t0 < n; t0 += VF_TILE) {
		const int i0 = t0 + threadIdx.x * VF_PER;
		int loc[VF_PER], last = -1;
#pragma unroll
		for (int e = 0; e < VF_PER; ++e) {
			const int i = i0 + e;
			if (i < n && m[i] == want) last = i;
			loc[e] = last;
		}
		int total;
		const int ex = max(vf_exclusive<true>(last, -1, &total, wave_tot), carry);
#pragma unroll
		for (int e = 0; e < VF_PER; ++e)
			if (i0 + e < n) prev[i0 + e] = max(loc[e], ex);
		carry = max(carry, total);
	}
}

// m[i] = f(i, m[i], prev[i], next[i]) with next[i] = the smallest j >= i with m[j] == want, n where there is none: tiles in descending order, and
// inside a tile thread t owns chunk VF_THREADS - 1 - t, so that the scan in thread order runs down the indices.  In place: a thread reads its own
// eight frames before it writes them, and nothing else reads them afterwards.
template <typename Fn>
__device__ void vf_next_sweep(uint8_t* m, int want, int n, const int* prev, int* wave_tot, Fn f) {
	int carry = n;
	for (int t0 = (n - 1) / VF_TILE * VF_TILE; t0 >= 0; t0 -= VF_TILE) {
		const int i0 = t0 + (VF_THREADS - 1 - (int)threadIdx.x) * VF_PER;
		int loc[VF_PER], v[VF_PER], nxt = n;
#pragma unroll
		for (int e = VF_PER - 1; e >= 0; --e) {
			const int i = i0 + e;
			v[e] = i < n ? m[i] : 0;
			if (i < n && v[e] == want) nxt = i;
			loc[e] = nxt;
		}
		int total;
		const int ex = min(vf_exclusive<false>(nxt, n, &total, wave_tot), carry);
#pragma unroll
		for (int e = 0; e < VF_PER; ++e) {
			const int i = i0 + e;
			if (i < n) m[i] = f(i, v[e], prev[i], min(loc[e], ex)) ? 1 : 0;
		}
		carry = min(carry, total);
	}
}

__global__ __launch_bounds__(VF_THREADS) void vad_frames_kernel(const float* __restrict__ peaks, const float* __restrict__ level, uint8_t* raw, uint8_t* mask, int* ws, int nF, int nfull,
                                                                float abs_thr, float rel_thr, float eps, int G, int S, int P) {
	__shared__ int wave_tot[VF_THREADS / 64];
	const int c = blockIdx.x;
	const float* pk = peaks + (int64_t)c * nF;
	uint8_t* r = raw + (int64_t)c * nF;
	uint8_t* m = mask + (int64_t)c * nF;
	int* prev = ws + (int64_t)c * nF;
	const float denom = __fadd_rn(eps, level[c]);
	for (int i = threadIdx.x; i < nF; i += VF_THREADS) {
		const float p = pk[i];
		const bool speech = i < nfull && !(p < abs_thr || __fdiv_rn(p, denom) < rel_thr);
		r[i] = m[i] = speech ? 1 : 0;
	}
	__syncthreads();
	if (G > 1) {  // a silent run between two speech frames, shorter than G
		vf_prev_sweep(m, 1, nF, prev, wave_tot);
		__syncthreads();
		vf_next_sweep(m, 1, nF, prev, wave_tot, [=](int i, int v, int p, int nx) { return v || (p >= 0 && nx < nF && nx - p - 1 < G); });
		__syncthreads();
	}
	if (S > 1) {  // a speech run shorter than S: between the last silent frame before i and the next one after it (-1 and nF at the ends)
		vf_prev_sweep(m, 0, nF, prev, wave_tot);
		__syncthreads();
		vf_next_sweep(m, 0, nF, prev, wave_tot, [=](int i, int v, int p, int nx) { return v && nx - p - 1 >= S; });
		__syncthreads();
	}
	if (P > 0) {  // within P frames of a speech frame
		vf_prev_sweep(m, 1, nF, prev, wave_tot);
		__syncthreads();
		vf_next_sweep(m, 1, nF, prev, wave_tot, [=](int i, int v, int p, int nx) { return (p >= 0 && i - p <= P) || (nx < nF && nx - i <= P); });
	}
}

static int vad_check_frames(const char* name, int C, int64_t nF) {
	CONVASR_CHECK_ARG(C >= 1 && C <= VAD_MAX_CHANNELS, "%s: %d channels, 1 to %d expected", name, C, VAD_MAX_CHANNELS);
	CONVASR_CHECK_ARG(nF >= 1 && nF <= VAD_MAX_LEN, "%s: %lld frames per channel, 1 to 2^28 expected", name, (long long)nF);
	return 0;
}

extern "C" int64_t convasr_vad_frames_workspace_bytes(int C, int64_t n_frames) {
	if (vad_check_frames("vad_frames_workspace_bytes", C, n_frames)) return -1;
	return vad_up256((int64_t)C * n_frames * 4);
}

extern "C" int convasr_vad_frames(const float* peaks, const float* level, int C, int64_t n_frames, int64_t n_full, float abs_thr, float rel_thr, float eps, int64_t G, int64_t S,
                                  int64_t P, uint8_t* raw, uint8_t* mask, void* workspace, int64_t workspace_bytes, void* stream) {
	if (const int e = vad_check_frames("vad_frames", C, n_frames)) return e;
	CONVASR_CHECK_ARG(n_full >= 1 && n_full <= n_frames && n_frames - n_full <= 1, "vad_frames: %lld full frames of %lld, all of them or all but the last expected, at least 1",
	                  (long long)n_full, (long long)n_frames);
	CONVASR_CHECK_ARG(G >= 0 && S >= 0 && P >= 0, "vad_frames: negative smoothing length (G %lld S %lld P %lld)", (long long)G, (long long)S, (long long)P);
	CONVASR_CHECK_ARG(peaks && level && raw && mask && workspace, "vad_frames: NULL pointer");
	CONVASR_CHECK_ARG(workspace_bytes >= vad_up256((int64_t)C * n_frames * 4) && ((uintptr_t)workspace & 3) == 0, "vad_frames: a 4-byte aligned workspace of %lld bytes needed, %lld given",
	                  (long long)vad_up256((int64_t)C * n_frames * 4), (long long)workspace_bytes);
	const auto clip = [&](int64_t v) { return (int)(v < n_frames + 1 ? v : n_frames + 1); };  // (longer than the recording: the same as its length + 1)
	hipLaunchKernelGGL(vad_frames_kernel, dim3(C), dim3(VF_THREADS), 0, (hipStream_t)stream, peaks, level, raw, mask, (int*)workspace, (int)n_frames, (int)n_full, abs_thr, rel_thr, eps,
	                   clip(G), clip(S), clip(P));
	CONVASR_CHECK_LAUNCH("vad_frames");
	return 0;
}

// ---------------------------------------------------------------------------------------------------------------- segments

#define VS_RUNS 1024  // run starts one tile of VS_RUNS frames can hold

// workspace: [0, 256): per-channel segment counts (int32); then C * nF bytes: 1 where a segment starts
__global__ __launch_bounds__(VF_THREADS) void vad_segments_count_kernel(const uint8_t* __restrict__ mask, const float* __restrict__ peaks, int nF, int M, int* counts, uint8_t* flags) {
	__shared__ int runs[VS_RUNS];
	__shared__ int n_runs, n_seg;
	const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint8_t* m = mask + (int64_t)c * nF;
	const float* pk = peaks + (int64_t)c * nF;
	uint8_t* fl = flags + (int64_t)c * nF;
	if (threadIdx.x == 0) n_seg = 0;
	for (int i = threadIdx.x; i < nF; i += VF_THREADS) fl[i] = 0;
	__syncthreads();
	const int half = (M + 1) / 2;
	for (int t0 = 0; t0 < nF; t0 += VS_RUNS) {
		if (threadIdx.x == 0) n_runs = 0;
		__syncthreads();
		const int i = t0 + threadIdx.x;
		if (i < nF && m[i] && (i == 0 || !m[i - 1])) {
			fl[i] = 1;
			atomicAdd(&n_seg, 1);
			if (M >= 2) runs[atomicAdd(&n_runs, 1)] = i;  // (the order in the list does not matter: runs do not touch)
		}
		__syncthreads();
		// a wave per run: while frames a .. a + M are all speech the run is longer than M; cut at the lowest index of the smallest peak in [a + half, a + M)
		for (int r = wave; r < n_runs; r += VF_THREADS / 64) {
			int a = runs[r];
			while (a + M < nF) {
				int all = 1, best = 0x7fffffff;
				float low = INFINITY;
				for (int j = a + lane; j <= a + M; j += 64) {
					all &= m[j] ? 1 : 0;
					if (j >= a + half && j < a + M) {
						const float p = pk[j];
						if (p < low) { low = p; best = j; }  // (ascending j per lane: the lowest index of this lane's minimum)
					}
				}
#pragma unroll
				for (int o = 32; o > 0; o >>= 1) {
					all &= __shfl_xor(all, o, 64);
					const float ol = __shfl_xor(low, o, 64);
					const int ob = __shfl_xor(best, o, 64);
					if (ol < low || (ol == low && ob < best)) { low = ol; best = ob; }
				}
				if (!all || best >= nF) break;
				if (lane == 0) { fl[best] = 1; atomicAdd(&n_seg, 1); }
				a = best;
			}
		}
		__syncthreads();
	}
	if (threadIdx.x == 0) counts[c] = n_seg;
}

// rank the marks (an exclusive prefix sum carried over the tiles), write channel and first sample at a mark and the end sample at the last frame of
// every segment into count[], then turn the ends into counts
__global__ __launch_bounds__(VF_THREADS) void vad_segments_write_kernel(const uint8_t* __restrict__ mask, int nF, int F, int64_t N, int C, const int* __restrict__ counts, const uint8_t* __restrict__ flags,
                                                                        int64_t total, int64_t* channel, int64_t* first, int64_t* count) {
	__shared__ int wave_tot[VF_THREADS / 64];
	const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint8_t* m = mask + (int64_t)c * nF;
	const uint8_t* fl = flags + (int64_t)c * nF;
	int64_t base = 0;
	for (int k = 0; k < c; ++k) base += counts[k];
	const int mine = counts[c];
	if (base + mine > total) return;  // (the host passed another total than the one it read: write nothing)
	int carry = 0;
	for (int t0 = 0; t0 < nF; t0 += VF_THREADS) {
		const int i = t0 + threadIdx.x;
		const int v = i < nF ? fl[i] : 0;
		int inc = v;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const int o = __shfl_up(inc, d, 64);
			if (lane >= d) inc += o;
		}
		__syncthreads();
		if (lane == 63) wave_tot[wave] = inc;
		__syncthreads();
		int before = carry, all = 0;
#pragma unroll
		for (int w = 0; w < VF_THREADS / 64; ++w) {
			if (w < wave) before += wave_tot[w];
			all += wave_tot[w];
		}
		const int rank = before + inc - v;  // marks before frame i
		if (i < nF && m[i]) {
			if (v && rank < mine) {
				channel[base + rank] = c;
				first[base + rank] = (int64_t)i * F;
			}
			const bool last = i + 1 == nF || !m[i + 1] || fl[i + 1];
			const int seg = rank + v - 1;  // the segment frame i belongs to
			if (last && seg >= 0 && seg < mine) count[base + seg] = min((int64_t)(i + 1) * F, N);
		}
		carry += all;
	}
	__syncthreads();
	for (int s = threadIdx.x; s < mine; s += VF_THREADS) count[base + s] -= first[base + s];
}

extern "C" int64_t convasr_vad_segments_workspace_bytes(int C, int64_t n_frames) {
	if (vad_check_frames("vad_segments_workspace_bytes", C, n_frames)) return -1;
	return 256 + vad_up256((int64_t)C * n_frames);
}

static int vad_check_segments(const char* name, int C, int64_t n_frames, int64_t workspace_bytes) {
	if (const int e = vad_check_frames(name, C, n_frames)) return e;
	CONVASR_CHECK_ARG(workspace_bytes >= 256 + vad_up256((int64_t)C * n_frames), "%s: a workspace of %lld bytes needed, %lld given", name, (long long)(256 + vad_up256((int64_t)C * n_frames)),
	                  (long long)workspace_bytes);
	return 0;
}

extern "C" int convasr_vad_segments_count(const uint8_t* mask, const float* peaks, int C, int64_t n_frames, int64_t max_frames, void* workspace, int64_t workspace_bytes, void* stream) {
	if (const int e = vad_check_segments("vad_segments_count", C, n_frames, workspace_bytes)) return e;
	CONVASR_CHECK_ARG(max_frames == 0 || max_frames >= 2, "vad_segments_count: max_frames %lld is neither 0 (no cutting) nor at least 2", (long long)max_frames);
	CONVASR_CHECK_ARG(mask && peaks && workspace && ((uintptr_t)workspace & 3) == 0, "vad_segments_count: NULL pointer or a workspace that is not 4-byte aligned");
	const int M = max_frames >= n_frames ? 0 : (int)max_frames;  // (no run is longer than the recording)
	hipLaunchKernelGGL(vad_segments_count_kernel, dim3(C), dim3(VF_THREADS), 0, (hipStream_t)stream, mask, peaks, (int)n_frames, M, (int*)workspace, (uint8_t*)workspace + 256);
	CONVASR_CHECK_LAUNCH("vad_segments_count");
	return 0;
}

extern "C" int convasr_vad_segments_write(const uint8_t* mask, int C, int64_t n_frames, int frame_len, int64_t N, const void* workspace, int64_t workspace_bytes, int64_t total,
                                          int64_t* channel, int64_t* first, int64_t* count, void* stream) {
	if (const int e = vad_check_segments("vad_segments_write", C, n_frames, workspace_bytes)) return e;
	CONVASR_CHECK_ARG(frame_len >= 1 && frame_len <= VAD_MAX_FRAME, "vad_segments_write: frame length %d, 1 to %d expected", frame_len, VAD_MAX_FRAME);
	CONVASR_CHECK_ARG(N >= 1 && N <= VAD_MAX_LEN && n_frames == ceil_div64(N, frame_len), "vad_segments_write: %lld frames is not ceil(%lld / %d), or N outside [1, 2^28]", (long long)n_frames,
	                  (long long)N, frame_len);
	CONVASR_CHECK_ARG(total >= 1 && total <= (int64_t)C * n_frames, "vad_segments_write: %lld segments, 1 to C x frames expected", (long long)total);
	CONVASR_CHECK_ARG(mask && workspace && channel && first && count, "vad_segments_write: NULL pointer");
	hipLaunchKernelGGL(vad_segments_write_kernel, dim3(C), dim3(VF_THREADS), 0, (hipStream_t)stream, mask, (int)n_frames, frame_len, N, C, (const int*)workspace, (const uint8_t*)workspace + 256, total,
	                   channel, first, count);
	CONVASR_CHECK_LAUNCH("vad_segments_write");
	return 0;
}

// ---------------------------------------------------------------------------------------------------------------- gather

// seg: (3, B) int64 on the device: channels, first samples, counts.  The host has checked its own copy of them; the clamps below keep a read inside
// the signal even if the two copies differ.
template <typename T>
__global__ __launch_bounds__(GS_THREADS) void gather_segments_kernel(const T* __restrict__ x, const int64_t* __restrict__ seg, float* __restrict__ out, int C, int64_t N, int B, int64_t Tpad) {
	const int b = blockIdx.y;
	int64_t ch = seg[b], first = seg[B + b], count = seg[2 * (int64_t)B + b];
	if (ch < 0 || ch >= C || first < 0 || first >= N) count = 0;
	count = min(count, N - first);
	const T* src = x + ch * N + first;
	float* dst = out + (int64_t)b * Tpad;
	for (int64_t t = (int64_t)blockIdx.x * GS_THREADS + threadIdx.x; t < Tpad; t += (int64_t)gridDim.x * GS_THREADS) {
		float v = 0.f;
		if (t < count) v = sizeof(T) == 2 ? __fdiv_rn((float)src[t], 32767.f) : (float)src[t];
		dst[t] = v;
	}
}

extern "C" int convasr_gather_segments(const void* signal, int dtype, int C, int64_t N, const int64_t* segments_host, const int64_t* segments, int B, float* out, int64_t Tpad, void* stream) {
	if (const int e = vad_check_signal("gather_segments", dtype, C, N)) return e;
	CONVASR_CHECK_ARG(B >= 1 && B <= 65535, "gather_segments: %d segments, 1 to 65535 expected", B);
	CONVASR_CHECK_ARG(segments_host, "gather_segments: NULL pointer");
	int64_t longest = 0;
	for (int b = 0; b < B; ++b) {
		const int64_t ch = segments_host[b], first = segments_host[B + b], count = segments_host[2 * (int64_t)B + b];
		CONVASR_CHECK_ARG(ch >= 0 && ch < C, "gather_segments: segment %d is on channel %lld of %d", b, (long long)ch, C);
		CONVASR_CHECK_ARG(first >= 0 && count >= 1 && first <= N && count <= N - first, "gather_segments: segment %d, samples [%lld, %lld + %lld), leaves [0, %lld) or is empty", b, (long long)first,
		                  (long long)first, (long long)count, (long long)N);
		longest = count > longest ? count : longest;
	}
	CONVASR_CHECK_ARG(Tpad >= longest && Tpad <= 2 * VAD_MAX_LEN, "gather_segments: Tpad %lld below the longest segment (%lld) or above 2^29", (long long)Tpad, (long long)longest);
	CONVASR_CHECK_ARG(signal && segments && out, "gather_segments: NULL pointer");
	const int64_t want = ceil_div64(Tpad, GS_THREADS);
	const dim3 grid((unsigned)(want < 65536 ? want : 65536), B);
	if (dtype == CONVASR_I16) hipLaunchKernelGGL(gather_segments_kernel<int16_t>, grid, dim3(GS_THREADS), 0, (hipStream_t)stream, (const int16_t*)signal, segments, out, C, N, B, Tpad);
	else hipLaunchKernelGGL(gather_segments_kernel<float>, grid, dim3(GS_THREADS), 0, (hipStream_t)stream, (const float*)signal, segments, out, C, N, B, Tpad);
	CONVASR_CHECK_LAUNCH("gather_segments");
	return 0;
}
