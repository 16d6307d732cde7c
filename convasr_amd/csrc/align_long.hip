// ctc.alignment (ctc.py:7-75) of a whole recording against its transcript (transcribe.py:176 without segmentation) on many CUs:
// convasr_ctc_alignment_long.  The two kernels of csrc/next.hip run one wave / one workgroup per utterance and stop at 8,191 labels; an
// hour of telephone audio is ~180,000 frames against ~48,000 labels = ~96,000 states.
//
// State s at frame t depends on states s, s-1, s-2 at frame t-1 only.  The lattice is cut into tiles of ALL_SB consecutive states (a
// "block") x `chunk` consecutive frames; a tile depends on the tile below it in time (the carried column), the tile to its left in state
// and the tile diagonally below-left (the last two states of the left block at the frame before).  Tiles with chunk + block = k are
// independent: launch k of a plain sequence of launches runs them, one wave per tile.  Every byte a tile reads from another tile was
// written by an earlier launch; nothing waits, spins or polls inside a launch.
//
// Sweep: lane l owns states s0 + l*NS .. s0 + l*NS + NS-1 of its block like ctc_alignment_kernel<NS>; neighbours inside the block come
// by __shfl_up, lane 0 takes its two from neigh[b][block-1][t-1] (published by the left block for EVERY frame: no ring, no overwrite
// hazard).  The arithmetic per state is that of the two kernels in next.hip, so the three give the same path bit for bit.
// Back-pointers: 2 bits per state, 16 consecutive states per dword, [B][T][ceil((2 S_max + 1) / 16)].
// A state with s > 2t + 1 is unreachable and its value is exactly AL_ZERO, its back-pointer 0: tiles wholly inside that region are not
// launched, and every read of the carried column / the published neighbours / the back-pointers substitutes those constants under the
// same per-state test, so a result never depends on how the lattice was cut.
//
// Walk: one wave per utterance.  Over F frames the path descends at most 2F states, so the F x (2F/16 + 2) back-pointer dwords around
// it are loaded into LDS by the whole wave and lane 0 walks inside LDS -- no dependent global load per frame.
#include "common.h"

#define AL_ZERO (-3.4028234663852886e38f)  // finfo(float32).min, the reference's "log zero" (as in next.hip)

#define ALL_NS 4                      // states per lane (a divisor of 16, >= 2)
#define ALL_SB (64 * ALL_NS)          // states per block
#define ALL_CHUNK_DEFAULT 256         // frames per chunk
#define ALL_CHUNK_MIN 16
#define ALL_CHUNK_MAX 4096
#define ALL_MAX_LABELS 131071
#define ALL_MAX_FRAMES (1 << 20)
#define ALL_MAX_BATCH 65535           // grid.y
#define ALL_WALK_F 128                // frames per window of the walk
#define ALL_WALK_W (2 * ALL_WALK_F / 16 + 2)

template <int NS>
__global__ __launch_bounds__(64) void ctc_alignment_long_sweep_kernel(const float* __restrict__ lp, const int64_t* __restrict__ targets, const int64_t* __restrict__ in_len,
                                                                      const int64_t* __restrict__ tgt_len, unsigned* __restrict__ bp, float* __restrict__ col,
                                                                      float2* __restrict__ neigh, int T, int C, int S_max, int blank, int chunk, int nblocks, int pitch,
                                                                      int diag, int j_lo) {
	constexpr int G = 16 / NS;  // lanes per back-pointer dword
	const int j = j_lo + (int)blockIdx.x, c = diag - j, b = blockIdx.y, lane = threadIdx.x;
	const int S = (int)tgt_len[b], Tb = (int)in_len[b], L = 2 * S + 1;
	if (S <= 0 || Tb <= 0 || Tb > T) return;
	const int s0 = j * (64 * NS);
	if (s0 >= L) return;  // every state of the block is past the utterance's last: all AL_ZERO, and no block that is read reads from it
	const int t_begin = c * chunk, t_end = min(T, t_begin + chunk);
	const int64_t* tg = targets + (int64_t)b * S_max;
	const float* lpb = lp + (int64_t)b * T * C;
	unsigned* bpb = bp + (int64_t)b * T * pitch;
	float* colp = col + ((int64_t)b * nblocks + j) * (64 * NS) + lane * NS;
	float2* pub = neigh + ((int64_t)b * nblocks + j) * T;
	const float2* left = neigh + ((int64_t)b * nblocks + (j - 1)) * T;  // (not dereferenced for j == 0)
	const int word = (s0 + lane * NS) >> 4;

	int cls[NS];
	bool allow2[NS], valid[NS];
	float a[NS], r[NS];
	int t;
#pragma unroll
	for (int i = 0; i < NS; ++i) {
		const int s = s0 + lane * NS + i;
		valid[i] = s < L;
		const bool lab = (s & 1) && valid[i];
		cls[i] = lab ? (int)tg[s >> 1] : blank;
		allow2[i] = lab && s >= 3 && tg[s >> 1] != tg[(s >> 1) - 1];  // blanks never take the s-2 move (equal to the blank two states back)
	}
	if (c == 0) {
#pragma unroll
		for (int i = 0; i < NS; ++i) a[i] = (valid[i] && s0 + lane * NS + i < 2) ? lpb[cls[i]] : AL_ZERO;
		if (lane == 63) pub[0] = make_float2(a[NS - 2], a[NS - 1]);
		t = 1;
	} else {
#pragma unroll
		for (int i = 0; i < NS; ++i) a[i] = (int64_t)(s0 + lane * NS + i) > 2 * (int64_t)(t_begin - 1) + 1 ? AL_ZERO : colp[i];
		t = t_begin;
	}
	if (t < t_end) {
		const float* row = lpb + (int64_t)t * C;
#pragma unroll
		for (int i = 0; i < NS; ++i) r[i] = row[cls[i]];
	}
	for (int base = t; base < t_end; base += 64) {
		// lane l fetches what lane 0 needs at frame base + l: the last two states of the left block at frame base + l - 1
		float q1 = AL_ZERO, q2 = AL_ZERO;
		const int64_t tp = (int64_t)base + lane - 1;
		if (j > 0 && base + lane < t_end && (int64_t)s0 - 2 <= 2 * tp + 1) {
			const float2 v = left[tp];
			q2 = v.x;
			q1 = (int64_t)s0 - 1 <= 2 * tp + 1 ? v.y : AL_ZERO;
		}
		const int n_here = min(64, t_end - base);
		for (int ii = 0; ii < n_here; ++ii, ++t) {
			float rn[NS];  // the next frame's log-probs, in flight while this frame is computed
			const float* row = lpb + (int64_t)min(t + 1, T - 1) * C;
#pragma unroll
			for (int i = 0; i < NS; ++i) rn[i] = row[cls[i]];
			float p1 = __shfl_up(a[NS - 1], 1, 64), p2 = __shfl_up(a[NS - 2], 1, 64);
			const float l1 = __shfl(q1, ii, 64), l2 = __shfl(q2, ii, 64);
			if (lane == 0) { p1 = l1; p2 = l2; }
			float n[NS];
			unsigned bits = 0;
#pragma unroll
			for (int i = NS - 1; i >= 0; --i) {
				const float stay = a[i];
				const float one = i >= 1 ? a[i - 1] : p1;
				const float two = allow2[i] ? (i >= 2 ? a[i - 2] : (i == 1 ? p1 : p2)) : AL_ZERO;
				unsigned k = 0;
				float best = stay;
				if (one > best) { k = 1; best = one; }
				if (two > best) { k = 2; best = two; }
				bits |= k << (2 * i);
				n[i] = valid[i] ? r[i] + (best + logf(expf(stay - best) + expf(one - best) + expf(two - best))) : AL_ZERO;
			}
			bits <<= 2 * NS * (lane % G);
#pragma unroll
			for (int o = 1; o < G; o <<= 1) bits |= __shfl_xor(bits, o, 64);
			if (lane % G == 0 && word < pitch) bpb[(int64_t)t * pitch + word] = bits;
#pragma unroll
			for (int i = 0; i < NS; ++i) { a[i] = n[i]; r[i] = rn[i]; }
			if (lane == 63) pub[t] = make_float2(a[NS - 2], a[NS - 1]);
		}
	}
#pragma unroll
	for (int i = 0; i < NS; ++i) colp[i] = a[i];
}

__global__ __launch_bounds__(64) void ctc_alignment_long_walk_kernel(const int64_t* __restrict__ in_len, const int64_t* __restrict__ tgt_len, int64_t* __restrict__ out,
                                                                     const unsigned* __restrict__ bp, const float* __restrict__ col, int T, int S_max, int nblocks, int pitch) {
	__shared__ unsigned win[ALL_WALK_F * ALL_WALK_W];
	const int b = blockIdx.x, lane = threadIdx.x;
	const int S = (int)tgt_len[b], Tb = (int)in_len[b];
	int64_t* ob = out + (int64_t)b * S_max;
	for (int j = lane; j < S_max; j += 64) ob[j] = 0;
	if (S <= 0 || Tb <= 0 || Tb > T) return;
	const unsigned* bpb = bp + (int64_t)b * T * pitch;
	const float* fin = col + (int64_t)b * nblocks * ALL_SB;  // the column at T-1, indexed by state
	const int64_t t_last = (int64_t)T - 1;
	const float f1 = 2 * (int64_t)S - 1 > 2 * t_last + 1 ? AL_ZERO : fin[2 * S - 1], f2 = 2 * (int64_t)S > 2 * t_last + 1 ? AL_ZERO : fin[2 * S];
	int s = 2 * S - 1 + (f2 > f1 ? 1 : 0);
	int seen = -1;
	for (int t_hi = Tb - 1; t_hi >= 1; t_hi -= ALL_WALK_F) {  // (frame 0 would record 0 into the zeroed output: nothing to do there)
		const int t_lo = max(1, t_hi - ALL_WALK_F + 1), nf = t_hi - t_lo + 1;
		const int w_hi = s >> 4, w_lo = max(0, w_hi - (ALL_WALK_W - 1)), nw = w_hi - w_lo + 1;
		for (int idx = lane; idx < nf * ALL_WALK_W; idx += 64) {
			const int f = idx / ALL_WALK_W, w = idx - f * ALL_WALK_W;
			if (w < nw) win[idx] = bpb[(int64_t)(t_lo + f) * pitch + w_lo + w];
		}
		__syncthreads();
		if (lane == 0) {
			for (int t = t_hi; t >= t_lo; --t) {
				if (s != seen) { if (s & 1) ob[s >> 1] = t; seen = s; }
				if (s <= 2 * t + 1) s -= (int)((win[(t - t_lo) * ALL_WALK_W + (s >> 4) - w_lo] >> (2 * (s & 15))) & 3u);  // (unreachable states point at themselves)
			}
		}
		s = __shfl(s, 0, 64);
		seen = __shfl(seen, 0, 64);
		__syncthreads();
	}
}

static int all_chunk(int chunk_frames) { return chunk_frames == 0 ? ALL_CHUNK_DEFAULT : chunk_frames; }

struct AllLayout { int nblocks, pitch; int64_t bp_off, col_off, neigh_off, bytes; };
static AllLayout all_layout(int B, int T, int S_max) {
	AllLayout y;
	const int64_t Lmax = 2 * (int64_t)S_max + 1;
	y.nblocks = (int)ceil_div64(Lmax, ALL_SB);
	y.pitch = (int)ceil_div64(Lmax, 16);
	const auto up = [](int64_t n) { return (n + 255) & ~(int64_t)255; };
	y.bp_off = 0;
	y.col_off = up((int64_t)B * T * y.pitch * 4);
	y.neigh_off = y.col_off + up((int64_t)B * y.nblocks * ALL_SB * 4);
	y.bytes = y.neigh_off + up((int64_t)B * y.nblocks * T * 8);
	return y;
}

static int all_check(int B, int T, int S_max) {
	if (B <= 0 || T <= 0 || S_max <= 0) return convasr_fail(CONVASR_EINVAL, "ctc_alignment_long: bad arguments (B %d T %d S_max %d)", B, T, S_max);
	if (S_max > ALL_MAX_LABELS) return convasr_fail(CONVASR_EUNSUPPORTED, "ctc_alignment_long: target length %d > %d", S_max, ALL_MAX_LABELS);
	if (T > ALL_MAX_FRAMES) return convasr_fail(CONVASR_EUNSUPPORTED, "ctc_alignment_long: %d frames > %d", T, ALL_MAX_FRAMES);
	if (B > ALL_MAX_BATCH) return convasr_fail(CONVASR_EUNSUPPORTED, "ctc_alignment_long: batch %d > %d", B, ALL_MAX_BATCH);
	return 0;
}

extern "C" int convasr_ctc_alignment_long_states_per_block(void) { return ALL_SB; }
extern "C" int convasr_ctc_alignment_long_chunk_frames(void) { return ALL_CHUNK_DEFAULT; }

extern "C" int64_t convasr_ctc_alignment_long_workspace_bytes(int B, int T, int S_max) {
	if (all_check(B, T, S_max) != 0) return -1;
	return all_layout(B, T, S_max).bytes;
}

// parts: 1 = the sweep, 2 = the walk over a workspace that a sweep with the same arguments filled, 3 = both (measurements time the two apart)
extern "C" int convasr_ctc_alignment_long_parts(const float* log_probs, const int64_t* targets, const int64_t* input_lengths, const int64_t* target_lengths, int64_t* alignment,
                                                void* workspace, int64_t workspace_bytes, int B, int T, int C, int S_max, int blank, int chunk_frames, int parts, void* stream) {
	CONVASR_CHECK_ARG(parts >= 1 && parts <= 3, "ctc_alignment_long: parts %d is not 1 (sweep), 2 (walk) or 3 (both)", parts);
	CONVASR_CHECK_ARG(log_probs && targets && input_lengths && target_lengths && alignment && workspace && C > 1 && blank >= 0 && blank < C, "ctc_alignment_long: bad arguments");
	if (const int e = all_check(B, T, S_max)) return e;
	CONVASR_CHECK_ARG(chunk_frames == 0 || (chunk_frames >= ALL_CHUNK_MIN && chunk_frames <= ALL_CHUNK_MAX), "ctc_alignment_long: chunk_frames %d is neither 0 nor in [%d, %d]", chunk_frames, ALL_CHUNK_MIN, ALL_CHUNK_MAX);
	const AllLayout y = all_layout(B, T, S_max);
	CONVASR_CHECK_ARG(workspace_bytes >= y.bytes, "ctc_alignment_long: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)y.bytes);
	CONVASR_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "ctc_alignment_long: the workspace must be 16-byte aligned");
	hipStream_t s = (hipStream_t)stream;
	unsigned* bp = (unsigned*)((char*)workspace + y.bp_off);
	float* col = (float*)((char*)workspace + y.col_off);
	float2* neigh = (float2*)((char*)workspace + y.neigh_off);
	const int64_t chunk = all_chunk(chunk_frames), nchunks = ceil_div64(T, chunk);
	for (int64_t k = 0; (parts & 1) && k < nchunks + y.nblocks - 1; ++k) {
		const int64_t j_lo = k - nchunks + 1 > 0 ? k - nchunks + 1 : 0;
		int64_t j_hi = k < y.nblocks - 1 ? k : y.nblocks - 1;
		// tile (chunk k - j, block j) lies wholly in s > 2t + 1 when j * ALL_SB > 2 * ((k - j + 1) * chunk - 1) + 1: true from some j on
		const int64_t j_reach = (2 * (k + 1) * chunk - 1) / (ALL_SB + 2 * chunk);
		if (j_reach < j_hi) j_hi = j_reach;
		if (j_hi < j_lo) continue;
		hipLaunchKernelGGL((ctc_alignment_long_sweep_kernel<ALL_NS>), dim3((unsigned)(j_hi - j_lo + 1), (unsigned)B), dim3(64), 0, s, log_probs, targets, input_lengths, target_lengths,
		                   bp, col, neigh, T, C, S_max, blank, (int)chunk, y.nblocks, y.pitch, (int)k, (int)j_lo);
	}
	CONVASR_CHECK_LAUNCH("ctc_alignment_long (sweep)");
	if (parts & 2) hipLaunchKernelGGL(ctc_alignment_long_walk_kernel, dim3(B), dim3(64), 0, s, input_lengths, target_lengths, alignment, bp, col, T, S_max, y.nblocks, y.pitch);
	CONVASR_CHECK_LAUNCH("ctc_alignment_long (walk)");
	return 0;
}

extern "C" int convasr_ctc_alignment_long(const float* log_probs, const int64_t* targets, const int64_t* input_lengths, const int64_t* target_lengths, int64_t* alignment,
                                          void* workspace, int64_t workspace_bytes, int B, int T, int C, int S_max, int blank, int chunk_frames, void* stream) {
	return convasr_ctc_alignment_long_parts(log_probs, targets, input_lengths, target_lengths, alignment, workspace, workspace_bytes, B, T, C, S_max, blank, chunk_frames, 3, stream);
}
