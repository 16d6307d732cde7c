// convasr_ctc_keyword_search: where in an utterance is a phrase said, and how sure is the model.  The rule is normative in
// include/convasr_hip.h and restated in float32 numpy by tests/_kws_ref.py; every score is a chain of fp32 additions along one path, so the
// mapping below cannot change a bit of the result.
//
// One WAVE per (utterance, phrase): lane i holds A_i (the label y_i) and Z_i (the blank after it) as (score, begin) pairs.  A frame costs
// one better() inside the lane -- M = better(Z_i, A_i), which is both Z_i's next value before the blank is added and, where y_{i+1} != y_i,
// what lane i + 1 may take; otherwise that is Z_i alone -- one shift of that pair up one lane (two DPP moves), one better() against the
// lane's own A_i and two additions.  Begin travels with the score: no back-pointers, no walk back.  Lane L - 1 holds E(t) and runs the hit
// picker on it as the frames go by (every lane runs the same selects on its own prefix of the phrase, only lane L - 1 stores; a wave-uniform
// test skips the frames below the threshold with no candidate held), so nothing of size T leaves the kernel unless the dense outputs are
// asked for.
// KWS_WAVES waves of a workgroup take KWS_WAVES phrases of the SAME utterance and share its frames:
//   C <= KWS_STAGE_MAX_C (staged): tiles of F = min(64, 4096 / C) frames go through LDS.  All 256 threads fetch the tile's F x C consecutive
//     floats with coalesced 4-byte loads into registers (16 per thread) BEFORE the waves consume the current tile and write them to the other
//     LDS buffer after it, so the fetch of tile n + 1 is in flight during the ~F serial steps of tile n.  Rows lie at the odd stride C | 1; four
//     threads per row take m_t.  A wave reads lp[t, y_i], lp[t, blank] and m_t out of LDS eight frames ahead of the recurrence.
//   C > KWS_STAGE_MAX_C (gathered): a tile no longer fits the register budget of the fetch; per tile of 64 frames the waves take m_t of 16 rows
//     each (lane = class mod 64, a max butterfly) into LDS, then every lane gathers lp[t, y_i] from global memory (the rows were just read:
//     cache hits) eight frames ahead.
// All stores are plain vector stores; no workspace, no memset, one launch.
#include "common.h"

namespace {

constexpr int KWS_WAVES = 4;          // phrases (= waves) per workgroup
constexpr int KWS_THREADS = KWS_WAVES * 64;
constexpr int KWS_REGS = 16;          // floats per thread of one staged tile
constexpr int KWS_TILE_ELEMS = KWS_REGS * KWS_THREADS;  // 4096 floats
constexpr int KWS_MAX_FRAMES = 64;    // frames per tile at most
constexpr int KWS_STAGE_MAX_C = 256;  // staged up to this many classes (F >= 16)
constexpr int KWS_AHEAD = 8;          // frames whose operands are read before the recurrence needs them
constexpr int KWS_BUF = KWS_TILE_ELEMS + KWS_MAX_FRAMES;  // F * (C | 1) <= F * C + F

__host__ __device__ inline int kws_tile_frames(int C) {
	const int f = KWS_TILE_ELEMS / C;
	return C > KWS_STAGE_MAX_C || f > KWS_MAX_FRAMES ? KWS_MAX_FRAMES : f;
}

struct KwsArgs {
	const float* lp;
	const int64_t* lengths;
	const int32_t *tokens, *token_lengths;
	const float* thresholds;
	int32_t* count;
	float* hit_score;
	int32_t *hit_begin, *hit_end;
	float* dense_score;
	int32_t* dense_begin;
	int T, C, K, L_max, H, blank, min_gap;
};

// one wave's lattice and picker
struct KwsWave {
	float a, z;       // A_i, Z_i scores
	int ab, zb;       // ... and begins
	bool has;         // picker: a candidate is held
	float cs;
	int cb, ce, last_end, cnt;
};

// d_t(c) = lp[t, c] - m_t in one subtraction; a NaN counts as -inf
__device__ __forceinline__ float kws_d(float v, float m) {
	const float d = v - m;
	return d != d ? -INFINITY : d;
}

// One frame.  Written with & and | on the comparisons' results, not && and ||: hipcc turns the short-circuit forms into divergent branches
// (an exec-mask save, a scalar branch and a restore each), which cost the first version of this step ~170 instructions and ~900 cycles a frame.
template <bool DENSE>
__device__ __forceinline__ void kws_step(KwsWave& w, const KwsArgs& p, float dy, float db, int t, int lane, bool next_differs, bool last, float thr,
                                         int64_t out_row, int64_t dense_row) {
	// M = better(Z_i, A_i): the larger score, among equals the smaller begin (two -inf both carry -1)
	const bool a_wins = (w.a > w.z) | ((w.a == w.z) & (w.ab < w.zb));
	const float ms = a_wins ? w.a : w.z;
	const int mb = a_wins ? w.ab : w.zb;
	// what the next label may take: the blank after this label, and this label itself unless the next one repeats it
	// (lane i takes lane i - 1's: one DPP move, no trip through the LDS crossbar as __shfl_up's ds_bpermute_b32 makes; lane 0 is replaced below)
	float rs = wave_shr1(next_differs ? ms : w.z, 0.f);
	int rb = wave_dpp<0x138>(0, next_differs ? mb : w.zb);
	rs = lane == 0 ? 0.f : rs;  // a span may open at every frame
	rb = lane == 0 ? t : rb;
	w.z = ms + db;
	w.zb = w.z == -INFINITY ? -1 : mb;
	const bool r_wins = (rs > w.a) | ((rs == w.a) & (rb < w.ab));
	w.a = (r_wins ? rs : w.a) + dy;
	w.ab = w.a == -INFINITY ? -1 : (r_wins ? rb : w.ab);
	if (DENSE && last) {
		p.dense_score[dense_row + t] = w.a;
		p.dense_begin[dense_row + t] = w.ab;
	}
	// The picker, on lane L - 1 (E(t) = its A); the other lanes' picker state is never read.  Most frames lie below the threshold with no
	// candidate held: one wave-uniform test skips them.
	if (__builtin_amdgcn_ballot_w64(last & ((w.a >= thr) | w.has)) == 0) return;
	const bool take = (w.a >= thr) & (w.ab > w.last_end) & (!w.has | (w.a > w.cs) | ((w.a == w.cs) & (w.ab == w.cb)));
	w.has |= take;
	w.cs = take ? w.a : w.cs;
	w.cb = take ? w.ab : w.cb;
	w.ce = take ? t : w.ce;
	const bool emit = w.has & (t - w.ce >= p.min_gap);
	if (emit & last & (w.cnt < p.H)) {
		p.hit_score[out_row + w.cnt] = w.cs;
		p.hit_begin[out_row + w.cnt] = w.cb;
		p.hit_end[out_row + w.cnt] = w.ce;
	}
	w.cnt += emit;
	w.last_end = emit ? w.ce : w.last_end;
	w.has &= !emit;
}

// nf frames from t0 on; STAGED: rows in `rows` at `stride`, else rows of the utterance in global memory at g (frame t0) with stride C
template <bool STAGED, bool DENSE>
__device__ __forceinline__ void kws_consume(KwsWave& w, const KwsArgs& p, const float* rows, int stride, const float* m, int t0, int nf, int y, bool in_phrase, int lane,
                                            bool next_differs, bool last, float thr, int64_t out_row, int64_t dense_row) {
	for (int f0 = 0; f0 < nf; f0 += KWS_AHEAD) {
		float dy[KWS_AHEAD], db[KWS_AHEAD];
#pragma unroll
		for (int u = 0; u < KWS_AHEAD; ++u) {
			const int f = f0 + u < nf ? f0 + u : nf - 1;  // (the tail re-reads the last frame; its step is not taken)
			const float* r = rows + (int64_t)f * stride;
			const float mt = m[f];
			dy[u] = kws_d(r[y], mt);
			db[u] = kws_d(r[p.blank], mt);
		}
#pragma unroll
		for (int u = 0; u < KWS_AHEAD; ++u)
			if (f0 + u < nf) kws_step<DENSE>(w, p, in_phrase ? dy[u] : -INFINITY, db[u], t0 + f0 + u, lane, next_differs, last, thr, out_row, dense_row);
	}
}

template <bool DENSE>
__global__ __launch_bounds__(KWS_THREADS) void kws_kernel(KwsArgs p) {
	__shared__ float tile[2][KWS_BUF];
	__shared__ float mrow[2][KWS_MAX_FRAMES];
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int b = blockIdx.y, k = blockIdx.x * KWS_WAVES + wv;
	const int T = p.T, C = p.C;
	int n = T;
	if (p.lengths) {
		const int64_t v = p.lengths[b];
		n = v < 0 ? 0 : v > T ? T : (int)v;
	}
	// this wave's phrase: label y of lane i < L (clamped into [0, C): the host has checked it), -1 beyond
	const bool active = k < p.K;
	int L = 0, y = -1;
	bool next_differs = true;
	float thr = INFINITY;
	if (active) {
		L = p.token_lengths[k];
		L = L < 0 ? 0 : L > p.L_max ? p.L_max : L;
		thr = p.thresholds[k];
		const int32_t* tk = p.tokens + (int64_t)k * p.L_max;
		if (lane < L) { y = tk[lane]; y = y < 0 ? 0 : y >= C ? C - 1 : y; }
		if (lane + 1 < L) { int yn = tk[lane + 1]; yn = yn < 0 ? 0 : yn >= C ? C - 1 : yn; next_differs = yn != y; }
	}
	const bool last = active && lane == L - 1;
	const int yr = y < 0 ? 0 : y;  // the class a lane beyond the phrase reads (its value is replaced by -inf)
	const int64_t out_row = ((int64_t)b * p.K + (active ? k : 0)) * p.H, dense_row = ((int64_t)b * p.K + (active ? k : 0)) * T;
	KwsWave w;
	w.a = w.z = -INFINITY; w.ab = w.zb = -1; w.has = false; w.cs = 0.f; w.cb = w.ce = 0; w.last_end = -1; w.cnt = 0;
	const float* g = p.lp + (int64_t)b * T * C;
	const int F = kws_tile_frames(C), ntiles = (n + F - 1) / F;

	if (C <= KWS_STAGE_MAX_C) {
		const int stride = C | 1, dq = KWS_THREADS / C, dr = KWS_THREADS % C;
		float r[KWS_REGS];
		auto fetch = [&](int i) {  // tile i's floats into registers
			const int t0 = i * F, nf = n - t0 < F ? n - t0 : F, total = nf * C;
			const float* src = g + (int64_t)t0 * C;
#pragma unroll
			for (int j = 0; j < KWS_REGS; ++j) {
				const int idx = tid + j * KWS_THREADS;
				r[j] = idx < total ? src[idx] : 0.f;
			}
		};
		auto put = [&](int i) {  // ... and from there into LDS rows
			const int t0 = i * F, nf = n - t0 < F ? n - t0 : F, total = nf * C;
			float* dst = tile[i & 1];
			int f = tid / C, c = tid - f * C;
#pragma unroll
			for (int j = 0; j < KWS_REGS; ++j) {
				if (tid + j * KWS_THREADS < total) dst[f * stride + c] = r[j];
				f += dq;
				c += dr;
				if (c >= C) { c -= C; ++f; }
			}
		};
		auto row_max = [&](int i) {  // m_t of tile i: four threads per row, NaNs ignored
			const int t0 = i * F, nf = n - t0 < F ? n - t0 : F;
			const int row = tid >> 2, part = tid & 3;
			const float* src = tile[i & 1] + row * stride;
			float v = -INFINITY;
			if (row < nf)
				for (int c = part; c < C; c += 4) v = fmaxf(v, src[c]);
			v = fmaxf(v, __shfl_xor(v, 1, 64));
			v = fmaxf(v, __shfl_xor(v, 2, 64));
			if (row < nf && part == 0) mrow[i & 1][row] = v;
		};
		if (ntiles > 0) {
			fetch(0);
			put(0);
			__syncthreads();
			row_max(0);
			__syncthreads();
		}
		for (int i = 0; i < ntiles; ++i) {
			const bool more = i + 1 < ntiles;
			if (more) fetch(i + 1);
			const int t0 = i * F, nf = n - t0 < F ? n - t0 : F;
			if (L > 0) kws_consume<true, DENSE>(w, p, tile[i & 1], stride, mrow[i & 1], t0, nf, yr, y >= 0, lane, next_differs, last, thr, out_row, dense_row);
			if (more) put(i + 1);
			__syncthreads();
			if (more) row_max(i + 1);
			__syncthreads();
		}
	} else {
		for (int i = 0; i < ntiles; ++i) {
			const int t0 = i * F, nf = n - t0 < F ? n - t0 : F;
			const float* src = g + (int64_t)t0 * C;
			for (int row = wv; row < nf; row += KWS_WAVES) {
				float v = -INFINITY;
				for (int c = lane; c < C; c += 64) v = fmaxf(v, src[(int64_t)row * C + c]);
				v = wave_max(v);
				if (lane == 0) mrow[0][row] = v;
			}
			__syncthreads();
			if (L > 0) kws_consume<false, DENSE>(w, p, src, C, mrow[0], t0, nf, yr, y >= 0, lane, next_differs, last, thr, out_row, dense_row);
			__syncthreads();
		}
	}
	if (!active) return;
	if (last) {
		if (w.has) {  // after the last frame the held candidate is a hit
			if (w.cnt < p.H) {
				p.hit_score[out_row + w.cnt] = w.cs;
				p.hit_begin[out_row + w.cnt] = w.cb;
				p.hit_end[out_row + w.cnt] = w.ce;
			}
			++w.cnt;
		}
		p.count[(int64_t)b * p.K + k] = w.cnt;
	}
	if (L == 0 && lane == 0) p.count[(int64_t)b * p.K + k] = 0;
	// dense rows: (-inf, -1) past the utterance's length (an empty phrase: everywhere)
	if (DENSE)
		for (int t = (L > 0 ? n : 0) + lane; t < T; t += 64) {
			p.dense_score[dense_row + t] = -INFINITY;
			p.dense_begin[dense_row + t] = -1;
		}
}

}  // namespace

extern "C" int convasr_ctc_keyword_search_max_labels(void) { return CONVASR_KWS_MAX_LABELS; }
extern "C" int convasr_ctc_keyword_search_phrases_per_block(void) { return KWS_WAVES; }
extern "C" int convasr_ctc_keyword_search_staged_classes(void) { return KWS_STAGE_MAX_C; }
extern "C" int convasr_ctc_keyword_search_tile_frames(int C) {
	if (C < 2 || C > CONVASR_KWS_MAX_CLASSES) return convasr_fail(CONVASR_EUNSUPPORTED, "ctc_keyword_search_tile_frames: %d classes, 2 to %d supported", C, CONVASR_KWS_MAX_CLASSES);
	return kws_tile_frames(C);
}

#define KWS_CHECK_ENVELOPE(cond, ...) do { if (!(cond)) return convasr_fail(CONVASR_EUNSUPPORTED, __VA_ARGS__); } while (0)

extern "C" int convasr_ctc_keyword_search(const float* log_probs, const int64_t* lengths, const int32_t* tokens, const int32_t* token_lengths,
                                          const float* thresholds, int32_t* count, float* hit_score, int32_t* hit_begin, int32_t* hit_end,
                                          float* dense_score, int32_t* dense_begin, int B, int T, int C, int K, int L_max, int H, int blank, int min_gap,
                                          void* stream) {
	CONVASR_CHECK_ARG(log_probs && tokens && token_lengths && thresholds && count && hit_score && hit_begin && hit_end, "ctc_keyword_search: NULL pointer");
	CONVASR_CHECK_ARG((dense_score == nullptr) == (dense_begin == nullptr), "ctc_keyword_search: dense_score and dense_begin come together");
	CONVASR_CHECK_ARG(H >= 1, "ctc_keyword_search: a capacity of %d hits, at least 1 expected", H);
	CONVASR_CHECK_ARG(min_gap >= 0, "ctc_keyword_search: min_gap %d < 0", min_gap);
	KWS_CHECK_ENVELOPE(B >= 1 && B <= 65535, "ctc_keyword_search: %d utterances, 1 to 65535 supported", B);
	KWS_CHECK_ENVELOPE(K >= 1 && K <= 65535, "ctc_keyword_search: %d phrases, 1 to 65535 supported", K);
	KWS_CHECK_ENVELOPE(T >= 1 && T <= CONVASR_KWS_MAX_FRAMES, "ctc_keyword_search: %d frames, 1 to %d supported", T, CONVASR_KWS_MAX_FRAMES);
	KWS_CHECK_ENVELOPE(C >= 2 && C <= CONVASR_KWS_MAX_CLASSES, "ctc_keyword_search: %d classes, 2 to %d supported", C, CONVASR_KWS_MAX_CLASSES);
	KWS_CHECK_ENVELOPE(L_max >= 1 && L_max <= CONVASR_KWS_MAX_LABELS, "ctc_keyword_search: phrases of up to %d labels, 1 to %d supported", L_max, CONVASR_KWS_MAX_LABELS);
	CONVASR_CHECK_ARG(blank >= 0 && blank < C, "ctc_keyword_search: blank %d outside [0, %d)", blank, C);
	KwsArgs p;
	p.lp = log_probs; p.lengths = lengths; p.tokens = tokens; p.token_lengths = token_lengths; p.thresholds = thresholds;
	p.count = count; p.hit_score = hit_score; p.hit_begin = hit_begin; p.hit_end = hit_end; p.dense_score = dense_score; p.dense_begin = dense_begin;
	p.T = T; p.C = C; p.K = K; p.L_max = L_max; p.H = H; p.blank = blank; p.min_gap = min_gap;
	const dim3 grid((unsigned)((K + KWS_WAVES - 1) / KWS_WAVES), (unsigned)B);
	if (dense_score) hipLaunchKernelGGL(kws_kernel<true>, grid, dim3(KWS_THREADS), 0, (hipStream_t)stream, p);
	else hipLaunchKernelGGL(kws_kernel<false>, grid, dim3(KWS_THREADS), 0, (hipStream_t)stream, p);
	CONVASR_CHECK_LAUNCH("ctc_keyword_search");
	return 0;
}
