// convasr_topk_frames / convasr_distill_kl: the k largest logits of every frame (the storage format of a teacher's posteriors) and the
// frame-level KL term of a student against such a truncated teacher, with its gradient.  The rules are normative in include/convasr_hip.h
// and restated in float64 numpy by tests/_distill_ref.py.
//
// Both read channels-last fp32 logits (B, T, C) once, with csrc/uncertainty.hip's two mappings:
//   C <= 64: one THREAD per frame.  A workgroup of 128 threads copies its 128 frames into LDS with coalesced 4-byte loads (rows at the odd
//     stride C | 1: the 64 lanes of a wave, each walking its own row, hit 64 different banks), then every thread works on its own row out
//     of LDS, classes in index order, no cross-lane step.  The KL kernel writes the gradient row back over the staged logits and the
//     workgroup copies the tile out the way it came in, so the (B, T, C) gradient leaves in coalesced stores too.
//   C > 64: one WAVE per frame, lane = class mod 64, four frames per workgroup; per-lane partials in class order, then xor butterflies (a
//     fixed tree); later walks re-read the row from the cache.
// Top-k turns every logit into an unsigned key whose integer order is the rule's value order, keeps the keys in LDS and runs k rounds of
// "take the largest key left, lowest class first, and zero it": no per-thread array (a runtime-indexed one would live in scratch), k * C
// integer compares a frame.
// The frame sum kd[b] is a second small launch over the per-frame values, one workgroup per utterance, fp64 partials in a fixed tree: no
// atomics anywhere, two runs are bit-equal.
#include "common.h"

namespace {

constexpr int DK_FRAMES = 128;   // row mapping: frames (= threads) per workgroup
constexpr int DK_ROW_MAX_C = 64; // row mapping up to this many classes (convasr_frame_uncertainty_row_classes())
constexpr int DK_WAVES = 4;      // wave mapping: frames (= waves) per workgroup
constexpr int DK_SUM_THREADS = 256;
constexpr int DK_WAVE_LDS_BYTES = 32 * 1024;  // top-k, wave mapping: the keys of a workgroup's rows (4 waves up to 2,048 classes, 2 up to 4,096, 1 above)

__device__ __forceinline__ void dk_store_value(void* p, int dtype, int64_t i, float v) {
	if (dtype == CONVASR_F16) ((f16_t*)p)[i] = (f16_t)v;  // round-to-nearest-even, +-inf beyond 65504
	else ((float*)p)[i] = v;
}
__device__ __forceinline__ void dk_store_index(void* p, int dtype, int64_t i, int c) {
	if (dtype == CONVASR_INDEX_U8) ((uint8_t*)p)[i] = (uint8_t)c;
	else if (dtype == CONVASR_INDEX_I16) ((int16_t*)p)[i] = (int16_t)c;
	else ((int32_t*)p)[i] = c;
}
__device__ __forceinline__ float dk_load_value(const void* p, int dtype, int64_t i) {
	return dtype == CONVASR_F16 ? (float)((const f16_t*)p)[i] : ((const float*)p)[i];
}
// (a negative int16 / int32 index comes out negative: the callers compare unsigned, so it is out of range like one >= C)
__device__ __forceinline__ int dk_load_index(const void* p, int dtype, int64_t i) {
	return dtype == CONVASR_INDEX_U8 ? (int)((const uint8_t*)p)[i] : dtype == CONVASR_INDEX_I16 ? (int)((const int16_t*)p)[i] : ((const int32_t*)p)[i];
}

__device__ __forceinline__ int dk_valid_frames(const int64_t* lengths, int64_t b, int T) {
	const int64_t n = lengths[b];
	return n < 0 ? 0 : n > T ? T : (int)n;
}

// the workgroup's nrows rows of C floats, consecutive in global memory, <-> the LDS tile at stride C | 1
template <bool TO_LDS> __device__ __forceinline__ void dk_copy_tile(float* tile, float* g, int nrows, int C, int tid) {
	const int stride = C | 1, total = nrows * C, dq = DK_FRAMES / C, dr = DK_FRAMES % C;
	int f = tid / C, c = tid - f * C;
#pragma unroll 4
	for (int i = tid; i < total; i += DK_FRAMES) {
		if (TO_LDS) tile[f * stride + c] = g[i];
		else g[i] = tile[f * stride + c];
		f += dq;
		c += dr;
		if (c >= C) { c -= C; ++f; }
	}
}

// ------------------------------------------------------------------------------------------------ top-k

// A logit as an unsigned key whose integer order is the rule's value order: larger value = larger key, every NaN the largest key, -0.0 and
// 0.0 the same key.  No value maps to 0 (-inf gives 0x007fffff): 0 marks an entry that has been taken.
__device__ __forceinline__ unsigned tk_key(float v) {
	const unsigned u = __float_as_uint(v);
	unsigned key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
	if (v == 0.f) key = 0x80000000u;
	if (v != v) key = 0xffffffffu;
	return key;
}

// Row mapping: the tile holds KEYS (made in the coalesced copy); round j takes the largest key left in the thread's row -- scanning the
// classes upwards with a strict compare, so among equal keys the lowest class -- and overwrites it with 0.  The value's own bits (the sign
// of a zero, a NaN's payload) are re-read from global memory, which the copy has just pulled through the cache.
__global__ __launch_bounds__(DK_FRAMES) void tk_row_kernel(const float* __restrict__ logits, void* __restrict__ values, int vdt, void* __restrict__ indices, int idt,
                                                           int64_t rows, int C, int k) {
	extern __shared__ unsigned tk_tile[];  // DK_FRAMES rows at stride C | 1
	const int tid = threadIdx.x, stride = C | 1;
	const int64_t row0 = (int64_t)blockIdx.x * DK_FRAMES;
	const int nrows = rows - row0 < DK_FRAMES ? (int)(rows - row0) : DK_FRAMES;
	{
		const float* g = logits + row0 * C;
		const int total = nrows * C, dq = DK_FRAMES / C, dr = DK_FRAMES % C;
		int f = tid / C, c = tid - f * C;
#pragma unroll 4
		for (int i = tid; i < total; i += DK_FRAMES) {
			tk_tile[f * stride + c] = tk_key(g[i]);
			f += dq;
			c += dr;
			if (c >= C) { c -= C; ++f; }
		}
	}
	__syncthreads();
	if (tid >= nrows) return;
	unsigned* r = tk_tile + tid * stride;
	const float* own = logits + (row0 + tid) * C;
	const int64_t o = (row0 + tid) * k;
	for (int j = 0; j < k; ++j) {
		unsigned bk = 0;
		int bi = 0;  // (k <= C: a key above 0 is left in every round)
#pragma unroll 4
		for (int c = 0; c < C; ++c) {
			const unsigned key = r[c];
			if (key > bk) { bk = key; bi = c; }
		}
		r[bi] = 0;
		dk_store_value(values, vdt, o + j, own[bi]);
		dk_store_index(indices, idt, o + j, bi);
	}
}

// Wave mapping: lane l owns the classes l, l + 64, ... and keeps their keys in the wave's own LDS row (at most DK_WAVE_LDS_BYTES: the host
// launches fewer waves per workgroup for wide rows); a round is the lane's best key left, a butterfly over (key, ~class) as one 64-bit
// number, and the owner zeroing its entry.  No lane reads another lane's LDS words: no barrier.
__global__ __launch_bounds__(DK_WAVES * 64) void tk_wave_kernel(const float* __restrict__ logits, void* __restrict__ values, int vdt, void* __restrict__ indices, int idt,
                                                                int64_t rows, int C, int k) {
	extern __shared__ unsigned tk_tile[];  // one row of C keys per wave
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
	if (row >= rows) return;
	const float* r = logits + row * C;
	unsigned* keys = tk_tile + (size_t)wave * C;
	for (int c = lane; c < C; c += 64) keys[c] = tk_key(r[c]);
	float mine_v = 0.f;
	int mine_i = 0;
	for (int j = 0; j < k; ++j) {
		unsigned bk = 0;
		int bi = 0;
		for (int c = lane; c < C; c += 64) {
			const unsigned key = keys[c];
			if (key > bk) { bk = key; bi = c; }
		}
		unsigned lo = ~(unsigned)bi;  // among equal keys the lower class is the larger number
#pragma unroll
		for (int s = 32; s > 0; s >>= 1) {  // both lanes of a pair end with the same entry
			const unsigned ok = __shfl_xor(bk, s, 64), ol = __shfl_xor(lo, s, 64);
			if (ok > bk || (ok == bk && ol > lo)) { bk = ok; lo = ol; }
		}
		const int wi = (int)~lo;  // (k <= C: some lane had a key above 0, so this is a real class)
		if ((wi & 63) == lane) keys[wi] = 0;
		if (lane == j) { mine_v = r[wi]; mine_i = wi; }  // lane j keeps winner j: one coalesced store at the end (k <= 32)
	}
	if (lane < k) {
		dk_store_value(values, vdt, row * k + lane, mine_v);
		dk_store_index(indices, idt, row * k + lane, mine_i);
	}
}

// ------------------------------------------------------------------------------------------------ KL against a truncated teacher

struct DkArgs {
	const float* logits;
	const void* values;
	const void* indices;
	const int64_t* lengths;
	float *frames, *grad;
	int64_t rows;
	int T, C, k, vdt, idt;
	float inv_tau, tau, tau2;
};

__global__ __launch_bounds__(DK_FRAMES) void dk_row_kernel(DkArgs a) {
	extern __shared__ float dk_tile[];
	const int tid = threadIdx.x, C = a.C, k = a.k;
	const int64_t row0 = (int64_t)blockIdx.x * DK_FRAMES;
	const int nrows = a.rows - row0 < DK_FRAMES ? (int)(a.rows - row0) : DK_FRAMES;
	dk_copy_tile<true>(dk_tile, const_cast<float*>(a.logits) + row0 * C, nrows, C, tid);
	__syncthreads();
	if (tid < nrows) {
		float* r = dk_tile + tid * (C | 1);
		const int64_t row = row0 + tid, b = row / a.T;
		const bool live = (int)(row - b * a.T) < dk_valid_frames(a.lengths, b, a.T);
		float kl = 0.f;
		if (live) {
			float m = -INFINITY, S = 0.f;
			for (int c = 0; c < C; ++c) m = fmaxf(m, r[c] * a.inv_tau);
			for (int c = 0; c < C; ++c) S += expf(r[c] * a.inv_tau - m);
			const int64_t o = row * k;
			float mu = -INFINITY;
			for (int j = 0; j < k; ++j) mu = fmaxf(mu, dk_load_value(a.values, a.vdt, o + j) * a.inv_tau);
			float Sp = 0.f, acc = 0.f;
			bool bad = false;
			for (int j = 0; j < k; ++j) {
				const float u = dk_load_value(a.values, a.vdt, o + j) * a.inv_tau - mu, e = expf(u);
				const int c = dk_load_index(a.indices, a.idt, o + j);
				const bool out = (unsigned)c >= (unsigned)C;
				bad |= out;
				const float s = out ? 0.f : r[c] * a.inv_tau - m;
				Sp += e;
				acc += e * (u - s);
			}
			kl = a.tau2 * (acc / Sp - (logf(Sp) - logf(S)));
			if (bad) kl = __builtin_nanf("");
			if (a.grad) {
				const float gq = a.tau / S, gp = a.tau / Sp;
				for (int c = 0; c < C; ++c) r[c] = bad ? __builtin_nanf("") : gq * expf(r[c] * a.inv_tau - m);
				if (!bad)
					for (int j = 0; j < k; ++j) {  // in teacher order: a class named twice loses both shares, in that order
						const float u = dk_load_value(a.values, a.vdt, o + j) * a.inv_tau - mu;
						r[dk_load_index(a.indices, a.idt, o + j)] -= gp * expf(u);
					}
			}
		} else if (a.grad) {
			for (int c = 0; c < C; ++c) r[c] = 0.f;
		}
		a.frames[row] = kl;
	}
	if (!a.grad) return;
	__syncthreads();
	dk_copy_tile<false>(dk_tile, a.grad + row0 * C, nrows, C, tid);
}

__global__ __launch_bounds__(DK_WAVES * 64) void dk_wave_kernel(DkArgs a) {
	const int64_t row = (int64_t)blockIdx.x * DK_WAVES + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63, C = a.C, k = a.k;
	if (row >= a.rows) return;
	const int64_t b = row / a.T;
	const bool live = (int)(row - b * a.T) < dk_valid_frames(a.lengths, b, a.T);
	float* g = a.grad ? a.grad + row * C : nullptr;
	if (!live) {
		if (g) for (int c = lane; c < C; c += 64) g[c] = 0.f;
		if (lane == 0) a.frames[row] = 0.f;
		return;
	}
	const float* r = a.logits + row * C;
	float m = -INFINITY, S = 0.f;
	for (int c = lane; c < C; c += 64) m = fmaxf(m, r[c] * a.inv_tau);
	m = wave_max(m);
	for (int c = lane; c < C; c += 64) S += expf(r[c] * a.inv_tau - m);
	S = wave_sum(S);
	// lane j holds teacher entry j (k <= 32); the lanes past k hold nothing: e = 0
	const bool has = lane < k;
	const float v = has ? dk_load_value(a.values, a.vdt, row * k + lane) * a.inv_tau : -INFINITY;
	const int ci = has ? dk_load_index(a.indices, a.idt, row * k + lane) : 0;
	const float mu = wave_max(v);
	const bool out = (unsigned)ci >= (unsigned)C;
	const float u = has ? v - mu : 0.f, e = has ? expf(u) : 0.f;
	const float s = (has && !out) ? r[ci] * a.inv_tau - m : 0.f;
	const float Sp = wave_sum(e), acc = wave_sum(e * (u - s));
	const bool bad = __ballot(out) != 0;
	if (lane == 0) a.frames[row] = bad ? __builtin_nanf("") : a.tau2 * (acc / Sp - (logf(Sp) - logf(S)));
	if (!g) return;
	const float gq = a.tau / S, pj = (a.tau / Sp) * e;
	for (int c0 = 0; c0 < C; c0 += 64) {  // (a wave-uniform loop: every lane stays active for the lane reads below)
		const int c = c0 + lane;
		float q = c < C ? gq * expf(r[c] * a.inv_tau - m) : 0.f;
		for (int j = 0; j < k; ++j) {  // in teacher order, as the row mapping does it
			const int cj = __builtin_amdgcn_readlane(ci, j);
			const float p = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pj), j));
			if (cj == c) q -= p;
		}
		if (c < C) g[c] = bad ? __builtin_nanf("") : q;
	}
}

// kd[b] = the sum of the utterance's per-frame values: thread i adds frames i, i + 256, ... in fp64, a butterfly per wave, the four waves
// in order, one rounding to fp32
__global__ __launch_bounds__(DK_SUM_THREADS) void dk_sum_kernel(const float* __restrict__ frames, const int64_t* __restrict__ lengths, float* __restrict__ kd, int T) {
	__shared__ double red[DK_SUM_THREADS / 64];
	const int b = blockIdx.x, tid = threadIdx.x;
	const int n = dk_valid_frames(lengths, b, T);
	const float* f = frames + (int64_t)b * T;
	double sum = 0.0;
	for (int t = tid; t < n; t += DK_SUM_THREADS) sum += (double)f[t];
#pragma unroll
	for (int s = 32; s > 0; s >>= 1) sum += __shfl_xor(sum, s, 64);
	if ((tid & 63) == 0) red[tid >> 6] = sum;
	__syncthreads();
	if (tid != 0) return;
	for (int i = 1; i < DK_SUM_THREADS / 64; ++i) sum += red[i];
	kd[b] = (float)sum;
}

bool dk_value_dtype(int d) { return d == CONVASR_F32 || d == CONVASR_F16; }
bool dk_index_dtype(int d) { return d == CONVASR_INDEX_U8 || d == CONVASR_INDEX_I16 || d == CONVASR_INDEX_I32; }

}  // namespace

extern "C" int convasr_topk_frames_max_k(void) { return CONVASR_TOPK_MAX_K; }

extern "C" int convasr_topk_frames(const float* logits, void* values, int values_dtype, void* indices, int indices_dtype, int B, int T, int C, int k,
                                   void* stream) {
	CONVASR_CHECK_ARG(logits && values && indices, "topk_frames: NULL pointer");
	CONVASR_CHECK_ARG(B >= 1 && T >= 1 && (int64_t)B * T < (1ll << 31), "topk_frames: B %d and T %d must be >= 1 and B * T below 2^31", B, T);
	CONVASR_CHECK_ARG(C >= 2 && C <= CONVASR_UNCERTAINTY_MAX_CLASSES, "topk_frames: %d classes, 2 to %d expected", C, CONVASR_UNCERTAINTY_MAX_CLASSES);
	CONVASR_CHECK_ARG(k >= 1 && k <= CONVASR_TOPK_MAX_K && k <= C, "topk_frames: k = %d, 1 to min(C = %d, %d) expected", k, C, CONVASR_TOPK_MAX_K);
	CONVASR_CHECK_ARG(dk_value_dtype(values_dtype), "topk_frames: values are fp32 or fp16, got dtype code %d", values_dtype);
	CONVASR_CHECK_ARG(dk_index_dtype(indices_dtype), "topk_frames: indices are uint8, int16 or int32, got index code %d", indices_dtype);
	CONVASR_CHECK_ARG(indices_dtype != CONVASR_INDEX_U8 || C <= 256, "topk_frames: uint8 indices cannot name %d classes (at most 256)", C);
	const int64_t rows = (int64_t)B * T;
	hipStream_t s = (hipStream_t)stream;
	if (C <= DK_ROW_MAX_C) {
		const size_t lds = (size_t)DK_FRAMES * (C | 1) * sizeof(float);
		hipLaunchKernelGGL(tk_row_kernel, dim3((unsigned)ceil_div64(rows, DK_FRAMES)), dim3(DK_FRAMES), lds, s, logits, values, values_dtype, indices, indices_dtype, rows, C, k);
	} else {
		const int waves = C * 4 * DK_WAVES <= DK_WAVE_LDS_BYTES ? DK_WAVES : C * 4 * 2 <= DK_WAVE_LDS_BYTES ? 2 : 1;
		hipLaunchKernelGGL(tk_wave_kernel, dim3((unsigned)ceil_div64(rows, waves)), dim3(waves * 64), (size_t)waves * C * sizeof(unsigned), s, logits, values, values_dtype, indices, indices_dtype, rows, C, k);
	}
	CONVASR_CHECK_LAUNCH("topk_frames");
	return 0;
}

extern "C" int convasr_distill_kl(const float* logits, const void* values, int values_dtype, const void* indices, int indices_dtype,
                                  const int64_t* lengths, float* kd, float* kd_frames, float* grad, int B, int T, int C, int k, float tau, void* stream) {
	CONVASR_CHECK_ARG(logits && values && indices && lengths && kd_frames, "distill_kl: NULL pointer");
	CONVASR_CHECK_ARG(B >= 1 && T >= 1 && (int64_t)B * T < (1ll << 31), "distill_kl: B %d and T %d must be >= 1 and B * T below 2^31", B, T);
	CONVASR_CHECK_ARG(C >= 2 && C <= CONVASR_UNCERTAINTY_MAX_CLASSES, "distill_kl: %d classes, 2 to %d expected", C, CONVASR_UNCERTAINTY_MAX_CLASSES);
	CONVASR_CHECK_ARG(k >= 1 && k <= CONVASR_TOPK_MAX_K && k <= C, "distill_kl: k = %d, 1 to min(C = %d, %d) expected", k, C, CONVASR_TOPK_MAX_K);
	CONVASR_CHECK_ARG(dk_value_dtype(values_dtype), "distill_kl: teacher values are fp32 or fp16, got dtype code %d", values_dtype);
	CONVASR_CHECK_ARG(dk_index_dtype(indices_dtype), "distill_kl: teacher indices are uint8, int16 or int32, got index code %d", indices_dtype);
	CONVASR_CHECK_ARG(indices_dtype != CONVASR_INDEX_U8 || C <= 256, "distill_kl: uint8 indices cannot name %d classes (at most 256)", C);
	CONVASR_CHECK_ARG(tau > 0.f && tau < INFINITY, "distill_kl: temperature %g, a finite value > 0 expected", (double)tau);
	DkArgs a;
	a.logits = logits; a.values = values; a.indices = indices; a.lengths = lengths; a.frames = kd_frames; a.grad = grad;
	a.rows = (int64_t)B * T; a.T = T; a.C = C; a.k = k; a.vdt = values_dtype; a.idt = indices_dtype;
	a.inv_tau = 1.f / tau; a.tau = tau; a.tau2 = tau * tau;
	hipStream_t s = (hipStream_t)stream;
	if (C <= DK_ROW_MAX_C) {
		const size_t lds = (size_t)DK_FRAMES * (C | 1) * sizeof(float);
		hipLaunchKernelGGL(dk_row_kernel, dim3((unsigned)ceil_div64(a.rows, DK_FRAMES)), dim3(DK_FRAMES), lds, s, a);
	} else {
		hipLaunchKernelGGL(dk_wave_kernel, dim3((unsigned)ceil_div64(a.rows, DK_WAVES)), dim3(DK_WAVES * 64), 0, s, a);
	}
	CONVASR_CHECK_LAUNCH("distill_kl");
	if (kd) {
		hipLaunchKernelGGL(dk_sum_kernel, dim3((unsigned)B), dim3(DK_SUM_THREADS), 0, s, kd_frames, lengths, kd, T);
		CONVASR_CHECK_LAUNCH("distill_kl (frame sum)");
	}
	return 0;
}
