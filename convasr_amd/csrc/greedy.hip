// convasr_ctc_greedy_segments: GreedyCTCGenerator.generate's collapse WITH the frame of every token and the word segments, as a
// flag + prefix-sum + compaction over frames.  The rule is normative in include/convasr_hip.h and restated in numpy by
// tests/_greedy_ref.py; the host loop (GreedyCTCGenerator.generate_host) is the oracle of both.
//
// Whether a frame emits depends on its class, the class of the previous non-blank frame and the number of blanks between them, so
// every frame is decided on its own.  An utterance is cut into chunks of GS_CHUNK = 256 frames, one wave (a 64-thread workgroup) per
// (utterance, chunk), a flat grid of N = B x ceil(T / 256) workgroups: the path is 8 bytes per frame, the passes are bound by
// latency and not by bytes, and a wave needs no LDS and no barrier.  An hour (180,000 frames) is 704 workgroups, the 64 x 753 batch 192.
// Five plain launches in stream order, no workgroup waits on another one:
//   1. summary  (N workgroups): per chunk, the last non-blank frame below the length and the first frame that is neither eps nor space.
//   2. carry    (one wave):     over the N chunks in (utterance, chunk) order: the last non-blank frame BEFORE every chunk (exclusive
//                               prefix maximum, however many silent chunks back it lies) and the utterance's first non-silent frame
//                               up to the chunk (inclusive prefix maximum of the mirrored frame).
//   3. count    (N workgroups): the emission rule per frame; per chunk the tokens, the segments and the last frame emitted from the path.
//   4. offsets  (one wave):     exclusive prefix sums of both counts (packed over the batch) and the last path emission before every chunk.
//   5. write    (N workgroups): the rule again; tokens, frames and segments go to their packed places.
// What the scans carry are FLAT frames b * T + t (B * T < 2^31), -1 for none: a flat frame of an earlier utterance is below b * T, so one
// unsegmented prefix maximum over all chunks serves every utterance; the first non-silent frame is carried as b * T + (T - 1 - t).
// Inside a tile of 64 frames the previous non-blank frame comes from a ballot (the highest set bit below the lane) and its class from
// one shuffle; the compaction ranks are mbcnt over ballots; the two scan kernels are DPP scans across the wave (row shifts and the two
// row broadcasts, as the edit distance's prefix minimum in metrics.hip), 64 chunks per step.
#include "common.h"

namespace {

constexpr int GS_THREADS = 64;
constexpr int GS_TILES = 4;
constexpr int GS_CHUNK = GS_THREADS * GS_TILES;
constexpr int GS_WS_ARRAYS = 10;

__device__ __forceinline__ int gs_top(uint64_t mask) { return 63 - __clzll((long long)mask); }  // highest set bit, mask != 0

// the workspace: GS_WS_ARRAYS arrays of `stride` ints
struct GsWorkspace {
	int *last_nb, *first_ns;          // summary: flat last non-blank frame of the chunk; flat mirrored first non-silent frame
	int *carry_nb, *start;            // carry: flat last non-blank frame before the chunk; flat mirrored first non-silent frame up to it
	int *ntok, *nseg, *last_pe;       // count: tokens and segments of the chunk, flat frame of its last path emission
	int *tok_off, *seg_off, *carry_pe;  // offsets: N + 1 packed exclusive sums each (tokens modulo 2^32), flat last path emission before the chunk
};
inline int64_t gs_stride(int64_t N) { return (N + 1 + 3) & ~(int64_t)3; }
inline GsWorkspace gs_carve(void* ws, int64_t N) {
	int* p = (int*)ws;
	const int64_t s = gs_stride(N);
	GsWorkspace w;
	w.last_nb = p; w.first_ns = p + s; w.carry_nb = p + 2 * s; w.start = p + 3 * s; w.ntok = p + 4 * s; w.nseg = p + 5 * s; w.last_pe = p + 6 * s;
	w.tok_off = p + 7 * s; w.seg_off = p + 8 * s; w.carry_pe = p + 9 * s;
	return w;
}

__global__ __launch_bounds__(GS_THREADS) void gs_summary_kernel(const int64_t* __restrict__ path, const int64_t* __restrict__ lengths,
                                                                int* __restrict__ last_nb, int* __restrict__ first_ns, int T, int nch,
                                                                int64_t eps, int64_t space) {
	const int i = blockIdx.x, b = i / nch, c = i - b * nch, lane = threadIdx.x;
	const int64_t* p = path + (int64_t)b * T;
	const int n = clamp_len(lengths[b], T);
	const int64_t base = (int64_t)c * GS_CHUNK;
	int last = -1, first = -1;
#pragma unroll
	for (int k = 0; k < GS_TILES; ++k) {
		const int64_t t = base + k * GS_THREADS + lane;
		const bool valid = t < n;
		const int64_t cls = valid ? p[t] : eps;
		const uint64_t nb = __ballot(valid && cls != eps), ns = __ballot(valid && cls != eps && cls != space);
		if (nb) last = (int)base + k * GS_THREADS + gs_top(nb);
		if (ns && first < 0) first = (int)base + k * GS_THREADS + __ffsll((long long)ns) - 1;
	}
	if (lane == 0) {
		last_nb[i] = last < 0 ? -1 : b * T + last;
		first_ns[i] = first < 0 ? -1 : b * T + (T - 1 - first);
	}
}

__global__ __launch_bounds__(GS_THREADS) void gs_carry_kernel(const int* __restrict__ last_nb, const int* __restrict__ first_ns,
                                                              int* __restrict__ carry_nb, int* __restrict__ start, int N) {
	const int lane = threadIdx.x;
	int run_nb = -1, run_ns = -1;
	for (int64_t base = 0; base < N; base += GS_THREADS) {
		const int64_t i = base + lane;
		const int nb = max(wave_prefix_max(i < N ? last_nb[i] : -1, -1), run_nb);   // (every value is >= -1)
		const int ns = max(wave_prefix_max(i < N ? first_ns[i] : -1, -1), run_ns);
		const int before = wave_dpp<0x138>(run_nb, nb);  // wave_shr:1, lane 0 <- the chunks before this step
		if (i < N) {
			carry_nb[i] = before;
			start[i] = ns;
		}
		run_nb = __builtin_amdgcn_readlane(nb, GS_THREADS - 1);
		run_ns = __builtin_amdgcn_readlane(ns, GS_THREADS - 1);
	}
}

__global__ __launch_bounds__(GS_THREADS) void gs_offsets_kernel(const int* __restrict__ ntok, const int* __restrict__ nseg,
                                                                const int* __restrict__ last_pe, int* __restrict__ tok_off,
                                                                int* __restrict__ seg_off, int* __restrict__ carry_pe, int N) {
	const int lane = threadIdx.x;
	int run_tok = 0, run_seg = 0, run_pe = -1;
	for (int64_t base = 0; base < N; base += GS_THREADS) {
		const int64_t i = base + lane;
		const int nt = i < N ? ntok[i] : 0, ns = i < N ? nseg[i] : 0;
		const int tok = wave_prefix_sum(nt, 0) + run_tok, seg = wave_prefix_sum(ns, 0) + run_seg;
		const int pe = max(wave_prefix_max(i < N ? last_pe[i] : -1, -1), run_pe);
		const int before = wave_dpp<0x138>(run_pe, pe);
		if (i < N) {
			tok_off[i] = tok - nt;
			seg_off[i] = seg - ns;
			carry_pe[i] = before;
		}
		run_tok = __builtin_amdgcn_readlane(tok, GS_THREADS - 1);
		run_seg = __builtin_amdgcn_readlane(seg, GS_THREADS - 1);
		run_pe = __builtin_amdgcn_readlane(pe, GS_THREADS - 1);
	}
	if (lane == 0) {
		tok_off[N] = run_tok;
		seg_off[N] = run_seg;
	}
}

// The emission rule over one chunk.  WRITE false: the chunk's counts.  WRITE true: its tokens and segments at their packed offsets; the
// last chunk of an utterance also writes the utterance's counts and the end frame of its last segment.
template <bool WRITE>
__global__ __launch_bounds__(GS_THREADS) void gs_emit_kernel(const int64_t* __restrict__ path, const int64_t* __restrict__ lengths, GsWorkspace w,
                                                             int64_t* __restrict__ tokens, int32_t* __restrict__ frames,
                                                             int64_t* __restrict__ counts, int64_t* __restrict__ seg_first,
                                                             int32_t* __restrict__ seg_begin, int32_t* __restrict__ seg_end, int B, int T, int nch,
                                                             int64_t eps, int64_t space, int gap, int split) {
	const int i = blockIdx.x, b = i / nch, c = i - b * nch, lane = threadIdx.x;
	const int64_t* p = path + (int64_t)b * T;
	const int n = clamp_len(lengths[b], T);
	const int flat0 = b * T;
	const int64_t base = (int64_t)c * GS_CHUNK;
	const int mirrored = w.start[i];
	const int S = mirrored >= flat0 ? T - 1 - (mirrored - flat0) : -1;  // the utterance's first non-silent frame when it lies in or before this chunk
	const bool live = S >= 0 && base < n && base + GS_CHUNK > S;
	// the walk's carried state, uniform across the wave: the last non-blank frame >= S before the tile and its class, the last frame
	// emitted from the path, the running packed offsets
	int P = -1, PE = -1, seg = 0;
	uint32_t tok = 0;
	int64_t Pc = eps;
	if (live) {
		const int g = w.carry_nb[i];
		if (g >= flat0 + S) {
			P = g - flat0;
			Pc = p[P];
		}
	}
	if (WRITE) {
		const int g = w.carry_pe[i];
		if (g >= flat0) PE = g - flat0;
		tok = (uint32_t)w.tok_off[i];
		seg = w.seg_off[i];
	}
	if (live) {
		int64_t cls_k[GS_TILES];
#pragma unroll
		for (int k = 0; k < GS_TILES; ++k) {
			const int64_t t = base + k * GS_THREADS + lane;
			cls_k[k] = t < n ? p[t] : eps;
		}
		const uint64_t below_lane = (1ull << lane) - 1;
#pragma unroll
		for (int k = 0; k < GS_TILES; ++k) {
			const int tile = (int)base + k * GS_THREADS;
			const int64_t t64 = base + k * GS_THREADS + lane;
			const bool act = t64 < n && t64 >= S;
			const int t = (int)t64;  // (only used where act)
			const int64_t cls = cls_k[k];
			const bool nonblank = act && cls != eps;
			const uint64_t nbm = __ballot(nonblank);
			const uint64_t nb_below = nbm & below_lane;
			const int src = nb_below ? gs_top(nb_below) : 0;
			const int64_t src_cls = __shfl(cls, src);
			const int prev = nb_below ? tile + src : P;
			const int64_t prev_cls = nb_below ? src_cls : Pc;
			const bool first = act && t == S;
			const bool pe = nonblank && (first || (prev_cls == space ? cls != space : (t - prev > 1 || cls != prev_cls)));
			const bool ins = act && cls == eps && prev >= 0 && prev_cls != space && t - prev == gap;
			const bool dbl = pe && split && cls == space;
			const bool open = first || dbl;
			const uint64_t em = __ballot(pe || ins), dm = __ballot(dbl), om = __ballot(open), pem = __ballot(pe);
			if (WRITE) {
				const size_t r = (size_t)tok + lane_rank(em) + lane_rank(dm);
				if (pe || ins) {
					tokens[r] = ins ? space : cls;
					frames[r] = t;
				}
				if (dbl) {
					tokens[r + 1] = cls;
					frames[r + 1] = t;
				}
				if (open) {
					const int s = seg + lane_rank(om);
					seg_first[s] = (int64_t)r;
					seg_begin[s] = t;
					if (!first) {  // a space from the path closes the segment before it, at the last frame emitted from the path
						const uint64_t pe_below = pem & below_lane;
						seg_end[s - 1] = pe_below ? tile + gs_top(pe_below) : PE;
					}
				}
			}
			tok += __popcll(em) + __popcll(dm);
			seg += __popcll(om);
			if (pem) PE = tile + gs_top(pem);
			if (nbm) {
				P = tile + gs_top(nbm);
				Pc = __shfl(cls, gs_top(nbm));
			}
		}
	}
	if (lane != 0) return;
	if (!WRITE) {
		w.ntok[i] = (int)tok;
		w.nseg[i] = seg;
		w.last_pe[i] = PE < 0 ? -1 : flat0 + PE;
	} else if (c == nch - 1) {
		const int i0 = b * nch;
		const int nseg = w.seg_off[i0 + nch] - w.seg_off[i0];
		counts[b] = (int64_t)((uint32_t)w.tok_off[i0 + nch] - (uint32_t)w.tok_off[i0]);
		counts[B + b] = nseg;
		if (nseg > 0) seg_end[w.seg_off[i0 + nch] - 1] = PE;
	}
}

inline int64_t gs_chunks(int T) { return ((int64_t)T + GS_CHUNK - 1) / GS_CHUNK; }

}  // namespace

extern "C" int convasr_ctc_greedy_segments_chunk_frames(void) { return GS_CHUNK; }

extern "C" int64_t convasr_ctc_greedy_segments_workspace_bytes(int B, int T) {
	if (B < 1 || T < 1 || (int64_t)B * T >= (1ll << 31)) {
		convasr_fail(CONVASR_EINVAL, "ctc_greedy_segments_workspace_bytes: B %d and T %d must be >= 1 and B * T below 2^31", B, T);
		return -1;
	}
	return GS_WS_ARRAYS * gs_stride((int64_t)B * gs_chunks(T)) * (int64_t)sizeof(int);
}

extern "C" int convasr_ctc_greedy_segments(const int64_t* path, const int64_t* lengths, int64_t* tokens, int32_t* frames, int64_t* counts,
                                           int64_t* seg_first, int32_t* seg_begin, int32_t* seg_end, void* workspace, int64_t workspace_bytes,
                                           int B, int T, int eps, int space, int blank_amount_to_space, int split_words, void* stream) {
	CONVASR_CHECK_ARG(path && lengths && tokens && frames && counts && seg_first && seg_begin && seg_end && workspace, "ctc_greedy_segments: NULL pointer");
	CONVASR_CHECK_ARG(B >= 1 && T >= 1, "ctc_greedy_segments: B %d and T %d must be >= 1", B, T);
	CONVASR_CHECK_ARG((int64_t)B * T < (1ll << 31), "ctc_greedy_segments: B * T = %lld, at most 2^31 - 1", (long long)B * T);
	CONVASR_CHECK_ARG(eps >= 0 && space >= 0 && eps != space, "ctc_greedy_segments: eps %d and space %d must be distinct and >= 0", eps, space);
	CONVASR_CHECK_ARG(blank_amount_to_space >= 0, "ctc_greedy_segments: blank_amount_to_space %d < 0", blank_amount_to_space);
	const int nch = (int)gs_chunks(T);
	const int64_t N = (int64_t)B * nch;
	const int64_t need = GS_WS_ARRAYS * gs_stride(N) * (int64_t)sizeof(int);
	CONVASR_CHECK_ARG(workspace_bytes >= need, "ctc_greedy_segments: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
	const GsWorkspace w = gs_carve(workspace, N);
	hipStream_t s = (hipStream_t)stream;
	const int gap = blank_amount_to_space > 1 ? blank_amount_to_space : 1;
	hipLaunchKernelGGL(gs_summary_kernel, dim3((unsigned)N), dim3(GS_THREADS), 0, s, path, lengths, w.last_nb, w.first_ns, T, nch, (int64_t)eps, (int64_t)space);
	CONVASR_CHECK_LAUNCH("ctc_greedy_segments (summary)");
	hipLaunchKernelGGL(gs_carry_kernel, dim3(1), dim3(GS_THREADS), 0, s, w.last_nb, w.first_ns, w.carry_nb, w.start, (int)N);
	CONVASR_CHECK_LAUNCH("ctc_greedy_segments (carry)");
	hipLaunchKernelGGL(gs_emit_kernel<false>, dim3((unsigned)N), dim3(GS_THREADS), 0, s, path, lengths, w, tokens, frames, counts, seg_first, seg_begin,
	                   seg_end, B, T, nch, (int64_t)eps, (int64_t)space, gap, split_words != 0);
	CONVASR_CHECK_LAUNCH("ctc_greedy_segments (count)");
	hipLaunchKernelGGL(gs_offsets_kernel, dim3(1), dim3(GS_THREADS), 0, s, w.ntok, w.nseg, w.last_pe, w.tok_off, w.seg_off, w.carry_pe, (int)N);
	CONVASR_CHECK_LAUNCH("ctc_greedy_segments (offsets)");
	hipLaunchKernelGGL(gs_emit_kernel<true>, dim3((unsigned)N), dim3(GS_THREADS), 0, s, path, lengths, w, tokens, frames, counts, seg_first, seg_begin,
	                   seg_end, B, T, nch, (int64_t)eps, (int64_t)space, gap, split_words != 0);
	CONVASR_CHECK_LAUNCH("ctc_greedy_segments (write)");
	return 0;
}
