// convasr_frame_uncertainty / convasr_span_uncertainty: how sure the model is of every frame and of every word.  The rule is normative in
// include/convasr_hip.h and restated in float64 numpy by tests/_uncertainty_ref.py.
//
// Frame pass: one read of the channels-last fp32 log-probs (B, T, C) gives the argmax (convasr_argmax's total order, re-implemented here:
// NaN above every number, ties to the lower index), the two largest probabilities and their margin, the entropy, the blank's probability
// and the entropy of the distribution renormalised without the blank.  Two mappings:
//   C <= 64 (the 38-class alphabet): one THREAD per frame.  A workgroup of 128 threads copies its 128 frames -- 128 x C consecutive
//     floats, 19 KB at C = 38 -- into LDS with coalesced 4-byte loads (rows land at an odd stride C | 1, so the 64 lanes of a wave, each
//     walking its own row, hit 64 different banks); then every thread walks its row twice out of LDS: classes in index order, no
//     cross-lane step, every lane busy whatever C is (one wave per frame with lane = class idles 26 of 64 lanes at C = 38), and the
//     summation order is the class order.
//   C > 64: one WAVE per frame, lane = class mod 64, four frames per workgroup; per-lane partials in class order, then xor butterflies
//     (a fixed tree); the second walk re-reads the row from the cache.
// Span pass: one workgroup of 256 threads per span, whatever its length (1 frame to a whole recording): thread i takes frames
// begin + i, begin + i + 256, ... and events first + i, ..., partials in fp64, then a butterfly per wave and the four waves in order.
// The tree depends on the span alone: a span's outputs do not change with N, with the other spans or with their order.
#include "common.h"

namespace {

constexpr int FU_FRAMES = 128;   // row mapping: frames (= threads) per workgroup
constexpr int FU_ROW_MAX_C = 64; // row mapping up to this many classes
constexpr int FU_WAVES = 4;      // wave mapping: frames (= waves) per workgroup
constexpr int SU_THREADS = 256;

struct FuOut {
	int64_t* idx;
	float *p1, *margin, *entropy, *entropy_nb, *p_eps;
};

// the value order of the argmax: NaN ranks above every number, two NaNs are equal
__device__ __forceinline__ bool fu_gt(float a, float b) { return a != a ? !(b != b) : a > b; }
// ... on (value, index) pairs: among equals the lower index wins
__device__ __forceinline__ bool fu_beats(float v, int i, float best, int bi) {
	const bool vn = v != v, bn = best != best;
	if (vn || bn) return vn && (!bn || i < bi);
	return v > best || (v == best && i < bi);
}

__device__ __forceinline__ int fu_valid_frames(const int64_t* lengths, int64_t b, int T) {
	if (!lengths) return T;
	const int64_t n = lengths[b];
	return n < 0 ? 0 : n > T ? T : (int)n;
}

// one frame's outputs from its reduced quantities: the largest value and its index, the second largest value, -sum p log p, the blank's
// log-prob, and S = sum exp(d), A = sum exp(d) d over the classes other than the blank with d = lp - (their maximum)
__device__ __forceinline__ void fu_store(const FuOut& o, int64_t row, bool live, bool has_nan, int bi, float best, float second, float ent,
                                         float lp_eps, float S, float A) {
	if (o.idx) o.idx[row] = bi;
	float p1 = expf(best), margin = p1 - expf(second), pe = expf(lp_eps), enb = logf(S) - A / S;
	if (has_nan) p1 = margin = ent = pe = enb = __builtin_nanf("");
	if (!live) p1 = margin = ent = pe = enb = 0.f;
	if (o.p1) o.p1[row] = p1;
	if (o.margin) o.margin[row] = margin;
	if (o.entropy) o.entropy[row] = ent;
	if (o.entropy_nb) o.entropy_nb[row] = enb;
	if (o.p_eps) o.p_eps[row] = pe;
}

__global__ __launch_bounds__(FU_FRAMES) void fu_row_kernel(const float* __restrict__ lp, const int64_t* __restrict__ lengths, FuOut o, int64_t rows,
                                                           int T, int C, int eps_id) {
	extern __shared__ float fu_tile[];  // FU_FRAMES rows at stride C | 1
	const int stride = C | 1, tid = threadIdx.x;
	const int64_t row0 = (int64_t)blockIdx.x * FU_FRAMES;
	const int nrows = rows - row0 < FU_FRAMES ? (int)(rows - row0) : FU_FRAMES;
	const int total = nrows * C;
	const float* g = lp + row0 * C;
	const int dq = FU_FRAMES / C, dr = FU_FRAMES % C;
	int f = tid / C, c = tid - f * C;
	// (a copy with 16 loads in flight per thread before the first LDS write was measured: 27.1 us against 24.0 and 25.8 us of this loop at
	// 64 x 753 x 38 in runs of their own -- no gain outside the spread between runs, not kept)
#pragma unroll 4
	for (int i = tid; i < total; i += FU_FRAMES) {
		fu_tile[f * stride + c] = g[i];
		f += dq;
		c += dr;
		if (c >= C) { c -= C; ++f; }
	}
	__syncthreads();
	if (tid >= nrows) return;
	const float* r = fu_tile + tid * stride;
	float best = r[0], second = -INFINITY, ent = 0.f, top_nb = -INFINITY;
	int bi = 0;
	bool has_nan = false;
	for (int k = 0; k < C; ++k) {
		const float v = r[k];
		has_nan |= v != v;
		ent -= expf(v) * v;
		if (k > 0) {
			if (fu_gt(v, best)) { second = best; best = v; bi = k; }
			else if (fu_gt(v, second)) second = v;
		}
		if (k != eps_id) top_nb = fmaxf(top_nb, v);
	}
	float S = 0.f, A = 0.f;
	for (int k = 0; k < C; ++k) {
		if (k == eps_id) continue;
		const float d = r[k] - top_nb, e = expf(d);
		S += e;
		A += e * d;
	}
	const int64_t row = row0 + tid, b = row / T;
	const bool live = (int)(row - b * T) < fu_valid_frames(lengths, b, T);
	fu_store(o, row, live, has_nan, bi, best, second, ent, r[eps_id], S, A);
}

__global__ __launch_bounds__(FU_WAVES * 64) void fu_wave_kernel(const float* __restrict__ lp, const int64_t* __restrict__ lengths, FuOut o, int64_t rows,
                                                                int T, int C, int eps_id) {
	const int64_t row = (int64_t)blockIdx.x * FU_WAVES + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	if (row >= rows) return;
	const float* r = lp + row * C;
	float best = -INFINITY, second = -INFINITY, ent = 0.f, top_nb = -INFINITY;
	int bi = 0x7fffffff;
	bool has_nan = false;
	for (int k = lane; k < C; k += 64) {
		const float v = r[k];
		has_nan |= v != v;
		ent -= expf(v) * v;
		if (fu_beats(v, k, best, bi)) { second = best; best = v; bi = k; }
		else if (fu_gt(v, second)) second = v;
		if (k != eps_id) top_nb = fmaxf(top_nb, v);
	}
#pragma unroll
	for (int s = 32; s > 0; s >>= 1) {  // both lanes of a pair end with the same (best, index, second)
		const float ov = __shfl_xor(best, s, 64), os = __shfl_xor(second, s, 64);
		const int oi = __shfl_xor(bi, s, 64);
		if (fu_beats(ov, oi, best, bi)) { second = fu_gt(best, os) ? best : os; best = ov; bi = oi; }
		else if (fu_gt(ov, second)) second = ov;
	}
	ent = wave_sum(ent);
	top_nb = wave_max(top_nb);
	has_nan = __ballot(has_nan) != 0;
	float S = 0.f, A = 0.f;
	for (int k = lane; k < C; k += 64) {
		if (k == eps_id) continue;
		const float d = r[k] - top_nb, e = expf(d);
		S += e;
		A += e * d;
	}
	S = wave_sum(S);
	A = wave_sum(A);
	if (lane != 0) return;
	const int64_t b = row / T;
	const bool live = (int)(row - b * T) < fu_valid_frames(lengths, b, T);
	fu_store(o, row, live, has_nan, bi, best, second, ent, r[eps_id], S, A);
}

// ------------------------------------------------------------------------------------------------ spans

struct SuArgs {
	const float* lp;
	const int64_t* idx;
	const float *p1, *margin, *entropy, *p_eps;
	const int64_t* utt;
	const int32_t *begin, *end;
	const int64_t *first, *tokens;
	const int32_t* frames;
	int64_t n_events;
	const int64_t *path, *frame_map;
	int32_t* n_out;
	float *confidence, *confidence_min, *margin_out, *entropy_out, *uncertainty;
	int B, T, Tp, C;
	float eps;
};

__device__ __forceinline__ int64_t su_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }
__device__ __forceinline__ float su_min(float a, float b) { return a != a ? a : b != b ? b : fminf(a, b); }  // a NaN stays

__device__ __forceinline__ double su_wave_sum(double v) {
#pragma unroll
	for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
	return v;
}
__device__ __forceinline__ float su_wave_min(float v) {
#pragma unroll
	for (int s = 32; s > 0; s >>= 1) v = su_min(v, __shfl_xor(v, s, 64));
	return v;
}

__global__ __launch_bounds__(SU_THREADS) void su_span_kernel(SuArgs a) {
	__shared__ double red_d[4][SU_THREADS / 64];
	__shared__ float red_f[2][SU_THREADS / 64];
	__shared__ int red_n[SU_THREADS / 64];
	const int k = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
	const int64_t u = su_clamp(a.utt[k], 0, a.B - 1);
	const int64_t b0 = su_clamp(a.begin[k], 0, a.Tp - 1), e0 = su_clamp(a.end[k], b0, a.Tp - 1);
	int64_t fb = b0, fe = e0;
	if (a.frame_map) {
		fb = su_clamp(a.frame_map[u * a.Tp + b0], 0, a.T - 1);
		fe = su_clamp(a.frame_map[u * a.Tp + e0], fb, a.T - 1);
	}
	// (without a map Tp == T: checked on the host)
	const float* H = a.entropy + u * a.T;
	const float* PE = a.p_eps + u * a.T;
	double sum_h = 0.0, num = 0.0, den = 0.0, sum_l = 0.0;
	for (int64_t t = fb + tid; t <= fe; t += SU_THREADS) {
		const double h = H[t], wt = 1.0 - (double)PE[t];
		sum_h += h;
		num += h * wt;
		den += wt;
	}
	float l_min = INFINITY, m_min = INFINITY;
	int n = 0;
	const bool events = a.tokens != nullptr;
	if (events) {
		const int64_t lo = su_clamp(a.first[k], 0, a.n_events), hi = su_clamp(a.first[k + 1], lo, a.n_events);
		for (int64_t j = lo + tid; j < hi; j += SU_THREADS) {
			const int64_t tk = a.tokens[j];
			const int32_t fr = a.frames[j];
			bool skip = j > lo && a.tokens[j - 1] == tk && a.frames[j - 1] == fr;
			const int64_t c = su_clamp(tk, 0, a.C - 1), p = su_clamp(fr, 0, a.Tp - 1);
			if (a.path && a.path[u * a.Tp + p] != tk) skip = true;
			if (skip) continue;
			const int64_t row = u * a.T + (a.frame_map ? su_clamp(a.frame_map[u * a.Tp + p], 0, a.T - 1) : p);
			const float l = a.lp[row * a.C + c];
			sum_l += l;
			l_min = su_min(l_min, l);
			m_min = su_min(m_min, a.idx[row] == c ? a.margin[row] : expf(l) - a.p1[row]);
			++n;
		}
	}
	sum_h = su_wave_sum(sum_h);
	num = su_wave_sum(num);
	den = su_wave_sum(den);
	sum_l = su_wave_sum(sum_l);
	l_min = su_wave_min(l_min);
	m_min = su_wave_min(m_min);
#pragma unroll
	for (int s = 32; s > 0; s >>= 1) n += __shfl_xor(n, s, 64);
	if (lane == 0) {
		red_d[0][w] = sum_h; red_d[1][w] = num; red_d[2][w] = den; red_d[3][w] = sum_l;
		red_f[0][w] = l_min; red_f[1][w] = m_min;
		red_n[w] = n;
	}
	__syncthreads();
	if (tid != 0) return;
	for (int i = 1; i < SU_THREADS / 64; ++i) {
		sum_h += red_d[0][i]; num += red_d[1][i]; den += red_d[2][i]; sum_l += red_d[3][i];
		l_min = su_min(l_min, red_f[0][i]); m_min = su_min(m_min, red_f[1][i]);
		n += red_n[i];
	}
	a.entropy_out[k] = (float)(sum_h / (double)(fe - fb + 1));
	a.uncertainty[k] = (float)(num / ((double)a.eps + den));
	if (!events) return;
	a.n_out[k] = n;
	a.confidence[k] = n ? expf((float)(sum_l / n)) : 0.f;
	a.confidence_min[k] = n ? expf(l_min) : 0.f;
	a.margin_out[k] = n ? m_min : 0.f;
}

}  // namespace

extern "C" int convasr_frame_uncertainty_row_classes(void) { return FU_ROW_MAX_C; }

extern "C" int convasr_frame_uncertainty(const float* log_probs, const int64_t* lengths, int64_t* idx, float* p1, float* margin, float* entropy,
                                         float* entropy_nb, float* p_eps, int B, int T, int C, int eps_id, void* stream) {
	CONVASR_CHECK_ARG(log_probs, "frame_uncertainty: NULL log_probs");
	CONVASR_CHECK_ARG(B >= 1 && T >= 1, "frame_uncertainty: B %d and T %d must be >= 1", B, T);
	CONVASR_CHECK_ARG((int64_t)B * T < (1ll << 31), "frame_uncertainty: B * T = %lld, at most 2^31 - 1", (long long)B * T);
	CONVASR_CHECK_ARG(C >= 2 && C <= CONVASR_UNCERTAINTY_MAX_CLASSES, "frame_uncertainty: %d classes, 2 to %d expected", C, CONVASR_UNCERTAINTY_MAX_CLASSES);
	CONVASR_CHECK_ARG(eps_id >= 0 && eps_id < C, "frame_uncertainty: eps_id %d outside [0, %d)", eps_id, C);
	const FuOut o = {idx, p1, margin, entropy, entropy_nb, p_eps};
	const int64_t rows = (int64_t)B * T;
	hipStream_t s = (hipStream_t)stream;
	if (C <= FU_ROW_MAX_C) {
		const size_t lds = (size_t)FU_FRAMES * (C | 1) * sizeof(float);
		hipLaunchKernelGGL(fu_row_kernel, dim3((unsigned)ceil_div64(rows, FU_FRAMES)), dim3(FU_FRAMES), lds, s, log_probs, lengths, o, rows, T, C, eps_id);
	} else {
		hipLaunchKernelGGL(fu_wave_kernel, dim3((unsigned)ceil_div64(rows, FU_WAVES)), dim3(FU_WAVES * 64), 0, s, log_probs, lengths, o, rows, T, C, eps_id);
	}
	CONVASR_CHECK_LAUNCH("frame_uncertainty");
	return 0;
}

extern "C" int convasr_span_uncertainty(const float* log_probs, const int64_t* idx, const float* p1, const float* margin, const float* entropy,
                                        const float* p_eps, const int64_t* utt, const int32_t* begin, const int32_t* end, const int64_t* first,
                                        const int64_t* tokens, const int32_t* frames, int64_t n_events, const int64_t* path, const int64_t* frame_map,
                                        int Tp, int32_t* n_out, float* confidence, float* confidence_min, float* margin_out, float* entropy_out,
                                        float* uncertainty, int64_t N, int B, int T, int C, float eps, void* stream) {
	CONVASR_CHECK_ARG(entropy && p_eps && utt && begin && end && entropy_out && uncertainty, "span_uncertainty: NULL pointer");
	CONVASR_CHECK_ARG(N >= 1 && N < (1ll << 31), "span_uncertainty: %lld spans, 1 to 2^31 - 1 expected", (long long)N);
	CONVASR_CHECK_ARG(B >= 1 && T >= 1 && (int64_t)B * T < (1ll << 31), "span_uncertainty: B %d and T %d must be >= 1 and B * T below 2^31", B, T);
	CONVASR_CHECK_ARG(Tp >= 1 && (int64_t)B * Tp < (1ll << 31), "span_uncertainty: B %d and a span grid of %d must be >= 1 and their product below 2^31", B, Tp);
	CONVASR_CHECK_ARG(frame_map || Tp == T, "span_uncertainty: a span grid of %d frames over %d frames needs a frame map", Tp, T);
	CONVASR_CHECK_ARG(C >= 2 && C <= CONVASR_UNCERTAINTY_MAX_CLASSES, "span_uncertainty: %d classes, 2 to %d expected", C, CONVASR_UNCERTAINTY_MAX_CLASSES);
	CONVASR_CHECK_ARG(eps >= 0.f, "span_uncertainty: eps %g < 0", (double)eps);
	const bool events = first || tokens || frames;
	if (events) {
		CONVASR_CHECK_ARG(first && tokens && frames, "span_uncertainty: first, tokens and frames come together");
		CONVASR_CHECK_ARG(n_events >= 0, "span_uncertainty: %lld events", (long long)n_events);
		CONVASR_CHECK_ARG(log_probs && idx && p1 && margin, "span_uncertainty: events need log_probs, idx, p1 and margin");
		CONVASR_CHECK_ARG(n_out && confidence && confidence_min && margin_out, "span_uncertainty: NULL output");
	} else {
		CONVASR_CHECK_ARG(!path, "span_uncertainty: a path without events");
	}
	SuArgs a;
	a.lp = log_probs; a.idx = idx; a.p1 = p1; a.margin = margin; a.entropy = entropy; a.p_eps = p_eps;
	a.utt = utt; a.begin = begin; a.end = end; a.first = first; a.tokens = tokens; a.frames = frames; a.n_events = n_events;
	a.path = path; a.frame_map = frame_map;
	a.n_out = n_out; a.confidence = confidence; a.confidence_min = confidence_min; a.margin_out = margin_out; a.entropy_out = entropy_out; a.uncertainty = uncertainty;
	a.B = B; a.T = T; a.Tp = Tp; a.C = C; a.eps = eps;
	hipLaunchKernelGGL(su_span_kernel, dim3((unsigned)N), dim3(SU_THREADS), 0, (hipStream_t)stream, a);
	CONVASR_CHECK_LAUNCH("span_uncertainty");
	return 0;
}
