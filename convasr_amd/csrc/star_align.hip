// The best path through the star-token CTC lattice at the size of whole recordings: convasr_star_alignment (include/convasr_hip.h has
// the rule, next to convasr_star_ctc_loss whose units, states and arc costs it shares).  True max-plus Viterbi in fp32: one rounded
// addition per arc, a maximum, one rounded addition of the emission; the back-pointer is the smallest arc that attains the maximum.
//
// Scheme of csrc/align_long.hip: the lattice is cut into tiles of SAL_SB consecutive states (a "block") x `chunk` consecutive frames;
// tiles with chunk + block = k are independent and launch k of a plain sequence of launches runs them, one wave per tile.  Every byte a
// tile reads from another tile was written by an earlier launch; nothing waits, spins or polls inside a launch.
//
// What differs from align_long.hip:
//   Arcs reach back four states.  A block publishes its last four states at every frame (one float4, no ring, no overwrite hazard);
//   blocks begin on an even state, so only the units -- the odd states -- have the long arcs and lane 0 consumes three of the four.
//   Back-pointers: a blank has two arcs (1 bit), a unit five (3 bits): 4 bits per PAIR of states (blank 2i, unit 2i + 1), 8 pairs = 16
//   states per dword, [B][T][ceil((2 N_max + 1) / 16)] -- the traffic of align_long's 2 bits per state.
//   A state with s > 4t + 3 is unreachable (start states 0..3, at most four states per frame): its value is exactly -inf and its
//   back-pointer 0.  Tiles wholly inside that region are not launched, and every read of the carried column / the published neighbours
//   substitutes -inf under the same per-state test, so a result never depends on how the lattice was cut.
//   Frames t >= Tb are neither read nor computed: a block's carried column stays frozen at frame Tb - 1, where the walk reads it.
//
// Walk: one wave per utterance.  Over F frames the path descends at most 4F states, so the F x (4F/16 + 2) back-pointer dwords around it
// and the 2F + 2 units it can meet are loaded into LDS by the whole wave and lane 0 walks inside LDS -- no dependent global load per
// frame.  The walk initialises all four outputs itself.
#include "common.h"

#define SAL_NS 4                      // states per lane: blank, unit, blank, unit
#define SAL_SB (64 * SAL_NS)          // states per block
#define SAL_CHUNK_DEFAULT 256         // frames per chunk
#define SAL_CHUNK_MIN 16
#define SAL_CHUNK_MAX 4096
#define SAL_MAX_LABELS 131071
#define SAL_MAX_UNITS (2 * SAL_MAX_LABELS + 1)
#define SAL_MAX_FRAMES (1 << 20)
#define SAL_MAX_BATCH 65535           // grid.y
#define SAL_WALK_F 128                // frames per window of the walk
#define SAL_WALK_W (4 * SAL_WALK_F / 16 + 2)
#define SAL_WALK_U (2 * SAL_WALK_F + 2)
#define SAL_WALK_UNROLL 17            // 128 x 34 dwords = 4 rounds of 64 lanes x 17 loads
#define SAL_NEG (-INFINITY)

// unit table entries: a class >= 0, -1 for a label outside [0, C) (emits -inf), -(gap + 2) for a star
__device__ static inline bool sal_is_star(int u) { return u <= -2; }

__global__ __launch_bounds__(64) void star_align_sweep_kernel(const float* __restrict__ lp, const int* __restrict__ units, const int* __restrict__ n_units,
                                                              const int64_t* __restrict__ in_len, unsigned* __restrict__ bp, float* __restrict__ col,
                                                              float4* __restrict__ neigh, int T, int C, int N_max, int blank, float pen, float ent, int chunk,
                                                              int nblocks, int pitch, int diag, int j_lo) {
	const int j = j_lo + (int)blockIdx.x, c = diag - j, b = blockIdx.y, lane = threadIdx.x;
	const int64_t Tb64 = in_len[b];
	const int n = n_units[b];
	if (Tb64 <= 0 || Tb64 > T || n < 0 || n > N_max) return;
	const int Tb = (int)Tb64, L = 2 * n + 1;
	const int s0 = j * SAL_SB;
	if (s0 >= L) return;  // every state of the block is past the utterance's last: all -inf, and no block that is read reads from it
	const int t_begin = c * chunk, t_end = min(Tb, t_begin + chunk);
	if (t_begin >= t_end) return;  // past the utterance's last frame: the carried column stays as frame Tb - 1 left it
	const int* ut = units + (int64_t)b * N_max;
	const float* lpb = lp + (int64_t)b * T * C;
	unsigned* bpb = bp + (int64_t)b * T * pitch;
	float* colp = col + ((int64_t)b * nblocks + j) * SAL_SB + lane * SAL_NS;
	float4* pub = neigh + ((int64_t)b * nblocks + j) * T;
	const float4* left = neigh + ((int64_t)b * nblocks + (j - 1)) * T;  // (not dereferenced for j == 0)
	const int sl = s0 + lane * SAL_NS;  // this lane's first state: the blank before unit sl / 2
	const int word = sl >> 4;

	// the lane's two units X = 0, 1 (states sl + 1, sl + 3) and the arcs into them
	int cidx[2];
	float konst[2], c1[2], c2[2], c3[2], c4[2];
	bool uvalid[2], bvalid[2];
#pragma unroll
	for (int x = 0; x < 2; ++x) {
		const int ix = (sl >> 1) + x;
		bvalid[x] = ix <= n;
		uvalid[x] = ix < n;
		const int u0 = uvalid[x] ? ut[ix] : -1;
		const int um1 = (uvalid[x] && ix >= 1) ? ut[ix - 1] : -1, um2 = (uvalid[x] && ix >= 2) ? ut[ix - 2] : -1;
		const bool star0 = uvalid[x] && sal_is_star(u0);
		cidx[x] = (uvalid[x] && u0 >= 0 && u0 < C) ? u0 : -1;
		konst[x] = star0 ? pen : SAL_NEG;
		c1[x] = star0 ? ent : 0.f;
		c2[x] = (uvalid[x] && ix >= 1 && u0 != um1) ? c1[x] : SAL_NEG;              // the unit before differs (a star differs from every label)
		c3[x] = (uvalid[x] && ix >= 1 && sal_is_star(um1)) ? 0.f : SAL_NEG;         // the blank before the star that is skipped
		c4[x] = (c3[x] == 0.f && ix >= 2 && um2 != u0) ? 0.f : SAL_NEG;             // the unit before that star, when it differs
	}

	float a[SAL_NS];   // a[0] blank, a[1] unit 0, a[2] blank, a[3] unit 1
	float rb, ru[2];   // emissions of the frame being computed: the blank, the two units
	int t;
	const float* row = lpb + (int64_t)t_begin * C;
	rb = row[blank];
#pragma unroll
	for (int x = 0; x < 2; ++x) ru[x] = cidx[x] >= 0 ? row[cidx[x]] : konst[x];
	if (c == 0) {
#pragma unroll
		for (int i = 0; i < SAL_NS; ++i) a[i] = SAL_NEG;
		if (sl == 0) {  // start states: 0, 1 (into a star: star_enter) and, when unit 0 is a star that is skipped, 3
			a[0] = 0.f + rb;
			if (uvalid[0]) a[1] = c1[0] + ru[0];
			if (uvalid[1] && c3[1] == 0.f) a[3] = 0.f + ru[1];
		}
		if (lane == 63) pub[0] = make_float4(a[0], a[1], a[2], a[3]);
		t = 1;
		if (t < t_end) {
			row = lpb + (int64_t)t * C;
			rb = row[blank];
#pragma unroll
			for (int x = 0; x < 2; ++x) ru[x] = cidx[x] >= 0 ? row[cidx[x]] : konst[x];
		}
	} else {
#pragma unroll
		for (int i = 0; i < SAL_NS; ++i) a[i] = (int64_t)(sl + i) > 4 * (int64_t)(t_begin - 1) + 3 ? SAL_NEG : colp[i];
		t = t_begin;
	}
	for (int base = t; base < t_end; base += 64) {
		// lane l fetches what lane 0 needs at frame base + l: the last states of the left block at frame base + l - 1
		float q1 = SAL_NEG, q2 = SAL_NEG, q3 = SAL_NEG;
		const int64_t tp = (int64_t)base + lane - 1, reach = 4 * tp + 3;
		if (j > 0 && base + lane < t_end && (int64_t)s0 - 3 <= reach) {
			const float4 v = left[tp];
			q3 = v.y;
			q2 = (int64_t)s0 - 2 <= reach ? v.z : SAL_NEG;
			q1 = (int64_t)s0 - 1 <= reach ? v.w : SAL_NEG;
		}
		const int n_here = min(64, t_end - base);
		for (int ii = 0; ii < n_here; ++ii, ++t) {
			// the next frame's log-probs, in flight while this frame is computed
			const float* rown = lpb + (int64_t)min(t + 1, Tb - 1) * C;
			const float rbn = rown[blank];
			float run[2];
#pragma unroll
			for (int x = 0; x < 2; ++x) run[x] = cidx[x] >= 0 ? rown[cidx[x]] : konst[x];
			float p1 = __shfl_up(a[3], 1, 64), p2 = __shfl_up(a[2], 1, 64), p3 = __shfl_up(a[1], 1, 64);
			const float l1 = __shfl(q1, ii, 64), l2 = __shfl(q2, ii, 64), l3 = __shfl(q3, ii, 64);
			if (lane == 0) { p1 = l1; p2 = l2; p3 = l3; }
			float nv[SAL_NS];
			unsigned bits = 0;
			// blanks: s, s - 1
			{
				float best = a[0] + 0.f;
				unsigned k = 0;
				const float one = p1 + 0.f;
				if (one > best) { best = one; k = 1; }
				nv[0] = bvalid[0] ? rb + best : SAL_NEG;
				bits |= k;
				best = a[2] + 0.f;
				k = 0;
				const float one2 = a[1] + 0.f;
				if (one2 > best) { best = one2; k = 1; }
				nv[2] = bvalid[1] ? rb + best : SAL_NEG;
				bits |= k << 4;
			}
			// units: s, s - 1, s - 2, s - 3, s - 4 -- the smallest arc that attains the maximum
			{
				float best = a[1] + 0.f, v;
				unsigned k = 0;
				v = a[0] + c1[0]; if (v > best) { best = v; k = 1; }
				v = p1 + c2[0];   if (v > best) { best = v; k = 2; }
				v = p2 + c3[0];   if (v > best) { best = v; k = 3; }
				v = p3 + c4[0];   if (v > best) { best = v; k = 4; }
				nv[1] = uvalid[0] ? ru[0] + best : SAL_NEG;
				bits |= k << 1;
				best = a[3] + 0.f;
				k = 0;
				v = a[2] + c1[1]; if (v > best) { best = v; k = 1; }
				v = a[1] + c2[1]; if (v > best) { best = v; k = 2; }
				v = a[0] + c3[1]; if (v > best) { best = v; k = 3; }
				v = p1 + c4[1];   if (v > best) { best = v; k = 4; }
				nv[3] = uvalid[1] ? ru[1] + best : SAL_NEG;
				bits |= k << 5;
			}
			bits <<= 8 * (lane & 3);
			bits |= __shfl_xor(bits, 1, 64);
			bits |= __shfl_xor(bits, 2, 64);
			if ((lane & 3) == 0 && word < pitch) bpb[(int64_t)t * pitch + word] = bits;
#pragma unroll
			for (int i = 0; i < SAL_NS; ++i) a[i] = nv[i];
			rb = rbn; ru[0] = run[0]; ru[1] = run[1];
			if (lane == 63) pub[t] = make_float4(a[0], a[1], a[2], a[3]);
		}
	}
#pragma unroll
	for (int i = 0; i < SAL_NS; ++i) colp[i] = a[i];
}

__global__ __launch_bounds__(64) void star_align_walk_kernel(const int* __restrict__ units, const int* __restrict__ n_units, const int64_t* __restrict__ in_len,
                                                             const int64_t* __restrict__ tgt_len, int64_t* __restrict__ out, int64_t* __restrict__ star_begin,
                                                             int64_t* __restrict__ star_frames, float* __restrict__ score, const unsigned* __restrict__ bp,
                                                             const float* __restrict__ col, int T, int S_max, int N_max, int nblocks, int pitch) {
	__shared__ unsigned win[SAL_WALK_F * SAL_WALK_W];
	__shared__ int uwin[SAL_WALK_U];
	const int b = blockIdx.x, lane = threadIdx.x;
	int64_t* ob = out + (int64_t)b * S_max;
	int64_t* sb = star_begin + (int64_t)b * (S_max + 1);
	int64_t* sf = star_frames + (int64_t)b * (S_max + 1);
	for (int i = lane; i < S_max; i += 64) ob[i] = 0;
	for (int i = lane; i <= S_max; i += 64) { sb[i] = -1; sf[i] = 0; }
	if (lane == 0) score[b] = SAL_NEG;
	const int64_t Tb64 = in_len[b], S64 = tgt_len[b];
	const int n = n_units[b];
	if (Tb64 <= 0 || Tb64 > T || n < 0 || n > N_max) return;
	const int Tb = (int)Tb64, L = 2 * n + 1;
	const int* ut = units + (int64_t)b * N_max;
	const unsigned* bpb = bp + (int64_t)b * T * pitch;
	const float* fin = col + (int64_t)b * nblocks * SAL_SB;  // the column at Tb - 1, indexed by state
	// the end state: the smallest s that attains the maximum over 2n, 2n - 1 and, behind a last star, 2n - 2, 2n - 3
	const int n_end = (n >= 1 && sal_is_star(ut[n - 1])) ? 4 : 2;
	const int64_t reach = 4 * ((int64_t)Tb - 1) + 3;
	float best = SAL_NEG;
	int s = -1;
	for (int e = max(0, L - n_end); e < L; ++e) {
		const float v = e > reach ? SAL_NEG : fin[e] + 0.f;
		if (v > best) { best = v; s = e; }
	}
	if (s < 0) return;  // no path
	// the outputs this wave zeroed above must be in memory before lane 0 overwrites some of them
	__syncthreads();
	if (lane == 0) score[b] = best;
	int lab = (int)(S64 < 0 ? 0 : (S64 > S_max ? S_max : S64));  // labels not yet met, walking backwards
	int seen = -1, gap = -1, cnt = 0, first = 0;
	for (int t_hi = Tb - 1; t_hi >= 0; t_hi -= SAL_WALK_F) {
		const int t_lo = max(0, t_hi - SAL_WALK_F + 1), nf = t_hi - t_lo + 1;
		const int w_hi = s >> 4, w_lo = max(0, w_hi - (SAL_WALK_W - 1)), nw = w_hi - w_lo + 1;
		const int u_hi = s >> 1, u_lo = max(0, u_hi - (SAL_WALK_U - 1));
		for (int base = 0; base < nf * SAL_WALK_W; base += 64 * SAL_WALK_UNROLL) {  // SAL_WALK_UNROLL loads in flight per lane: the window is latency-bound
			unsigned v[SAL_WALK_UNROLL];
#pragma unroll
			for (int k = 0; k < SAL_WALK_UNROLL; ++k) {
				const int idx = base + k * 64 + lane, f = idx / SAL_WALK_W, w = idx - f * SAL_WALK_W;
				v[k] = (idx < nf * SAL_WALK_W && w < nw && t_lo + f >= 1) ? bpb[(int64_t)(t_lo + f) * pitch + w_lo + w] : 0u;  // (frame 0 has no back-pointers)
			}
#pragma unroll
			for (int k = 0; k < SAL_WALK_UNROLL; ++k) {
				const int idx = base + k * 64 + lane;
				if (idx < nf * SAL_WALK_W) win[idx] = v[k];
			}
		}
		for (int i = lane; i < SAL_WALK_U; i += 64) uwin[i] = u_lo + i < n ? ut[u_lo + i] : -1;
		__syncthreads();
		if (lane == 0) {
			for (int t = t_hi; t >= t_lo; --t) {
				if (s != seen) {
					if (gap >= 0) { sb[gap] = first; sf[gap] = cnt; gap = -1; }
					seen = s;
					if (s & 1) {
						const int u = uwin[(s >> 1) - u_lo];
						if (sal_is_star(u)) {
							const int g = -(u + 2);
							if (g <= S_max) { gap = g; cnt = 0; }
						} else if (--lab >= 0) ob[lab] = t;
					}
				}
				if (gap >= 0) { ++cnt; first = t; }
				if (t >= 1 && s <= 4 * (int64_t)t + 3) {  // (unreachable states point at themselves)
					const unsigned nib = (win[(t - t_lo) * SAL_WALK_W + (s >> 4) - w_lo] >> (4 * ((s >> 1) & 7))) & 15u;
					s -= (int)((s & 1) ? nib >> 1 : nib & 1u);
				}
			}
		}
		s = __shfl(s, 0, 64);
		__syncthreads();
	}
	if (lane == 0 && gap >= 0) { sb[gap] = first; sf[gap] = cnt; }
}

static int sal_chunk(int chunk_frames) { return chunk_frames == 0 ? SAL_CHUNK_DEFAULT : chunk_frames; }

struct SalLayout { int nblocks, pitch; int64_t bp_off, col_off, neigh_off, bytes; };
static SalLayout sal_layout(int B, int T, int N_max) {
	SalLayout y;
	const int64_t Lmax = 2 * (int64_t)N_max + 1;
	y.nblocks = (int)ceil_div64(Lmax, SAL_SB);
	y.pitch = (int)ceil_div64(Lmax, 16);
	const auto up = [](int64_t n) { return (n + 255) & ~(int64_t)255; };
	y.bp_off = 0;
	y.col_off = up((int64_t)B * T * y.pitch * 4);
	y.neigh_off = y.col_off + up((int64_t)B * y.nblocks * SAL_SB * 4);
	y.bytes = y.neigh_off + up((int64_t)B * y.nblocks * T * 16);
	return y;
}

static int sal_check(int B, int T, int N_max) {
	if (B <= 0 || T <= 0 || N_max <= 0) return convasr_fail(CONVASR_EINVAL, "star_alignment: bad arguments (B %d T %d N_max %d)", B, T, N_max);
	if (N_max > SAL_MAX_UNITS) return convasr_fail(CONVASR_EUNSUPPORTED, "star_alignment: %d units > %d (%d labels with every gap starred)", N_max, SAL_MAX_UNITS, SAL_MAX_LABELS);
	if (T > SAL_MAX_FRAMES) return convasr_fail(CONVASR_EUNSUPPORTED, "star_alignment: %d frames > %d", T, SAL_MAX_FRAMES);
	if (B > SAL_MAX_BATCH) return convasr_fail(CONVASR_EUNSUPPORTED, "star_alignment: batch %d > %d", B, SAL_MAX_BATCH);
	return 0;
}

extern "C" int convasr_star_alignment_states_per_block(void) { return SAL_SB; }
extern "C" int convasr_star_alignment_chunk_frames(void) { return SAL_CHUNK_DEFAULT; }

extern "C" int64_t convasr_star_alignment_workspace_bytes(int B, int T, int N_max) {
	if (sal_check(B, T, N_max) != 0) return -1;
	return sal_layout(B, T, N_max).bytes;
}

// parts: 1 = the sweep, 2 = the walk over a workspace that a sweep with the same arguments filled, 3 = both (measurements time the two apart)
extern "C" int convasr_star_alignment_parts(const float* log_probs, const int32_t* units, const int32_t* n_units, const int64_t* input_lengths, const int64_t* target_lengths,
                                            float star_penalty, float star_enter, int64_t* alignment, int64_t* star_begin, int64_t* star_frames, float* score,
                                            void* workspace, int64_t workspace_bytes, int B, int T, int C, int S_max, int N_max, int blank, int chunk_frames, int parts, void* stream) {
	CONVASR_CHECK_ARG(parts >= 1 && parts <= 3, "star_alignment: parts %d is not 1 (sweep), 2 (walk) or 3 (both)", parts);
	CONVASR_CHECK_ARG(log_probs && units && n_units && input_lengths && target_lengths && (alignment || S_max == 0) && star_begin && star_frames && score && workspace && C > 1 && blank >= 0 && blank < C && S_max >= 0,
	                  "star_alignment: bad arguments");
	CONVASR_CHECK_ARG(star_penalty <= 0.f && star_enter <= 0.f && star_penalty > -INFINITY && star_enter > -INFINITY, "star_alignment: star_penalty %g and star_enter %g must be finite and <= 0 (natural-log costs)", (double)star_penalty, (double)star_enter);
	if (S_max > SAL_MAX_LABELS) return convasr_fail(CONVASR_EUNSUPPORTED, "star_alignment: target length %d > %d", S_max, SAL_MAX_LABELS);
	if (const int e = sal_check(B, T, N_max)) return e;
	CONVASR_CHECK_ARG(chunk_frames == 0 || (chunk_frames >= SAL_CHUNK_MIN && chunk_frames <= SAL_CHUNK_MAX), "star_alignment: chunk_frames %d is neither 0 nor in [%d, %d]", chunk_frames, SAL_CHUNK_MIN, SAL_CHUNK_MAX);
	const SalLayout y = sal_layout(B, T, N_max);
	CONVASR_CHECK_ARG(workspace_bytes >= y.bytes, "star_alignment: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)y.bytes);
	CONVASR_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "star_alignment: the workspace must be 16-byte aligned");
	hipStream_t s = (hipStream_t)stream;
	unsigned* bp = (unsigned*)((char*)workspace + y.bp_off);
	float* col = (float*)((char*)workspace + y.col_off);
	float4* neigh = (float4*)((char*)workspace + y.neigh_off);
	const int64_t chunk = sal_chunk(chunk_frames), nchunks = ceil_div64(T, chunk);
	for (int64_t k = 0; (parts & 1) && k < nchunks + y.nblocks - 1; ++k) {
		const int64_t j_lo = k - nchunks + 1 > 0 ? k - nchunks + 1 : 0;
		int64_t j_hi = k < y.nblocks - 1 ? k : y.nblocks - 1;
		// tile (chunk k - j, block j) lies wholly in s > 4t + 3 when j * SAL_SB > 4 * ((k - j + 1) * chunk - 1) + 3: true from some j on
		const int64_t j_reach = (4 * (k + 1) * chunk - 1) / (SAL_SB + 4 * chunk);
		if (j_reach < j_hi) j_hi = j_reach;
		if (j_hi < j_lo) continue;
		hipLaunchKernelGGL(star_align_sweep_kernel, dim3((unsigned)(j_hi - j_lo + 1), (unsigned)B), dim3(64), 0, s, log_probs, units, n_units, input_lengths, bp, col, neigh,
		                   T, C, N_max, blank, star_penalty, star_enter, (int)chunk, y.nblocks, y.pitch, (int)k, (int)j_lo);
	}
	CONVASR_CHECK_LAUNCH("star_alignment (sweep)");
	if (parts & 2) hipLaunchKernelGGL(star_align_walk_kernel, dim3(B), dim3(64), 0, s, units, n_units, input_lengths, target_lengths, alignment, star_begin, star_frames, score,
	                                  bp, col, T, S_max, N_max, y.nblocks, y.pitch);
	CONVASR_CHECK_LAUNCH("star_alignment (walk)");
	return 0;
}

extern "C" int convasr_star_alignment(const float* log_probs, const int32_t* units, const int32_t* n_units, const int64_t* input_lengths, const int64_t* target_lengths,
                                      float star_penalty, float star_enter, int64_t* alignment, int64_t* star_begin, int64_t* star_frames, float* score,
                                      void* workspace, int64_t workspace_bytes, int B, int T, int C, int S_max, int N_max, int blank, int chunk_frames, void* stream) {
	return convasr_star_alignment_parts(log_probs, units, n_units, input_lengths, target_lengths, star_penalty, star_enter, alignment, star_begin, star_frames, score,
	                                    workspace, workspace_bytes, B, T, C, S_max, N_max, blank, chunk_frames, 3, stream);
}
