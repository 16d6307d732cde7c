// CTC prefix beam search without a language model: decoders.BeamSearchDecoder (decoders.py:19-55, ctcdecode.CTCBeamDecoder with
// lm_path = None), train.py --decoder BeamSearchDecoder / --decoder-topk / --beam-width.  The semantics are normative in
// include/convasr_hip.h and restated in float64 by tests/_ctc_beam_ref.py.
//
// One workgroup per utterance; the frame loop runs inside the kernel.  Per frame:
//   1. P_t: radix select of the top-N classes (key = (descending lp, class)); sorted and cut only when cutoff_prob < 1.
//   2. The current beams go into an LDS hash table keyed by their 64-bit prefix hash; every beam looks up its parent prefix there.
//      When the parent is a current beam i and last(l_j) is in P_t, the extension l_i + last(l_j) is folded into l_j's own
//      candidate and its bit in i's fold mask is set, so it is not a candidate of its own.
//   3. Candidates (beam i, own or position p in P_t) are never materialised: a radix select over the 64-bit key of the candidate's
//      score finds the W-th best (score recomputed each pass: one fp64 add, or the stored own score), then the exact ties at the
//      boundary are resolved by the candidate key (rank << 14 | c + 1).  The selected ones (<= W) are compacted and bitonic-sorted
//      by (score, key): that order is the next frame's ranking.
//   4. A selected extension creates a node in the global arena (parent node, token); node id = t * W + rank, so the frame of a token
//      is node / W.  The best topk beams are walked back once at the end.
// Beam scores are fp64 (the log-probs are read as fp32): the selection boundary of a wide beam over hundreds of frames sits among
// tens of thousands of candidates, and fp32 accumulation would reorder near-ties that the float64 restatement keeps apart.
//
// With an n-gram LM (convasr_ctc_beam_search_lm; tables built by convasr_amd/lm.py, restated by tests/_ctc_beam_lm_ref.py) the same body
// runs as bs_body<true>.  Each beam also keeps in LDS its vocabulary-trie node (the current word), its LM state (the entry id of the
// longest listed suffix of its word history), the mask of the classes it may be extended by (the trie node's children, plus the space
// when the current word is a word of V), and the fp64 LM term of a space extension.  All four are set once when the beam is created
// (step 4: one trie step, and for a word that ends there the n-gram lookups of its score), so the frame loop only tests mask bits and
// adds the cached term.  bs_body<false, *> is the LM-free kernel: every LM statement sits under `if constexpr (LM)`.
//
// The wide form (convasr_ctc_beam_search_wide / _lm_wide, W <= 8192) is bs_body<LM, true>: the same body, with the per-beam arrays in
// the utterance's region of the workspace instead of LDS (bs_wide_layout).  LDS keeps the sort buffer and the per-frame
// class arrays.  A thread makes up to W / 1024 beams in step 4, so the beam state is double-buffered there, and the tie pass of the radix
// select covers the 27-bit candidate key.  Every difference sits under `if constexpr (WIDE)`: the LDS kernels are unchanged.
//
// With hot phrases (convasr_ctc_beam_search_hot / _lm_hot and their wide forms; tables built by convasr_amd/hotwords.py, restated by
// tests/_ctc_beam_hot_ref.py) the body runs as bs_body<LM, WIDE, true>.  Each beam also keeps the node of the phrase trie it has matched up
// to (or DEAD), the number of labels matched since the last completed phrase, and that node's child mask; a candidate's score gets +w when
// its class continues the match and gives the pending labels' bonus back when it does not (the header states the rule).  Every hot
// statement sits under `if constexpr (HOT)`: the four kernels above are bs_body<*, *, false> and compile as before.
#include <cmath>

#include "common.h"

#define BS_MAX_W 1024
#define BS_WIDE_MAX_W 8192
#define BS_MAX_N 128
#define BS_MAX_C 8192
#define BS_KEY_C_BITS 14  // candidate key = rank << 14 | (c + 1): c + 1 <= 8192 < 2^14, rank < 1024 -> 24 bits (wide form: rank < 8192 -> 27 bits)
#define BS_LM_MAX_C 256
#define BS_LM_MAX_ORDER 6
#define BS_LM_EMPTY_KEY (-2)

// The LM tables (convasr_amd/lm.py documents them); MW = ceil(C / 32) mask words per trie node.
struct BsLm {
	const unsigned* node_mask;  // (n_nodes, MW)
	const int* node_child;      // (n_nodes,)
	const int* node_word;       // (n_nodes,)
	const double2* ent_pb;      // (n_ent,): (log10 p, log10 bow)
	const int2* ent_sl;         // (n_ent,): (longest listed proper suffix, order)
	const int4* slots;          // (n_slots,): (context entry, word, entry, 0)
	int n_slots, space, order, start;
	double alpha, beta;
};

// The hot-phrase trie (convasr_amd/hotwords.py documents it; the header states the rule); MW mask words per node as above.
#define BS_HOT_DEAD (-1)
struct BsHot {
	const unsigned* mask;  // (n_nodes, MW)
	const int* child;      // (n_nodes,)
	const int* term;       // (n_nodes,): 1 when a phrase ends at the node
	int n_nodes, space;
	double w;
};

__host__ __device__ static inline int bs_pow2(int x) { int p = 1; while (p < x) p <<= 1; return p; }

struct BsSel {
	uint64_t P, M;       // resolved high bits of the boundary key / their mask
	unsigned KP, KM;     // the same over the candidate key, among exact score ties
	int need, full, all, tie;
	int bucket, before, cnt;
	int n, np, m, cut;   // beams, |P_t|, selected, cutoff length
};

struct BsLayout {
	int W, NW, C, S, TB;        // beams, fold words per beam, classes, sort size, hash table size
	size_t lpb, lpnb, tot, own_nb, own_nnb, own_s, hash, phash, su, plp;  // 8-byte arrays
	size_t sel;                                                              // the selection state (BsSel)
	size_t last, node, len, fold, sk, htab, pc, hist, pos;                   // 4- / 2-byte arrays
	size_t lmsp, lnode, lstate, lmask;                                       // LM only: fp64 term, trie node, LM state, MW mask words
	int MW;
	size_t hu, hk, hmask, hroot;                                             // hot phrases only: trie node, pending count, HMW mask words; the root's mask (always LDS)
	int HMW;
	size_t bytes;               // LDS
	size_t dbl, gbytes;         // wide form: the distance between the two copies of the beam state / the workspace bytes per utterance
};

__host__ __device__ static inline BsLayout bs_layout(int W, int N, int C, bool lm = false, bool hot = false) {
	BsLayout L;
	L.W = W; L.NW = (N + 31) / 32; L.C = C;
	L.S = bs_pow2(W > BS_MAX_N ? W : BS_MAX_N);
	L.TB = bs_pow2(2 * W > 64 ? 2 * W : 64);
	size_t o = 0;
	L.lpb = o; o += 8 * (size_t)W;
	L.lpnb = o; o += 8 * (size_t)W;
	L.tot = o; o += 8 * (size_t)W;
	L.own_nb = o; o += 8 * (size_t)W;
	L.own_nnb = o; o += 8 * (size_t)W;
	L.own_s = o; o += 8 * (size_t)W;
	L.hash = o; o += 8 * (size_t)W;
	L.phash = o; o += 8 * (size_t)W;
	L.su = o; o += 8 * (size_t)L.S;
	L.plp = o; o += 8 * (size_t)BS_MAX_N;
	L.sel = o; o += (sizeof(BsSel) + 15) & ~(size_t)15;
	L.last = o; o += 4 * (size_t)W;
	L.node = o; o += 4 * (size_t)W;
	L.len = o; o += 4 * (size_t)W;
	L.fold = o; o += 4 * (size_t)W * L.NW;
	L.sk = o; o += 4 * (size_t)L.S;
	L.htab = o; o += 4 * (size_t)L.TB;
	L.pc = o; o += 4 * (size_t)BS_MAX_N;
	L.hist = o; o += 4 * 256;
	L.pos = o; o += 2 * (size_t)C;
	L.MW = 0; L.lmsp = L.lnode = L.lstate = L.lmask = 0;
	if (lm) {
		L.MW = (C + 31) / 32;
		o = (o + 7) & ~(size_t)7;
		L.lmsp = o; o += 8 * (size_t)W;
		L.lnode = o; o += 4 * (size_t)W;
		L.lstate = o; o += 4 * (size_t)W;
		L.lmask = o; o += 4 * (size_t)W * L.MW;
	}
	L.HMW = 0; L.hu = L.hk = L.hmask = L.hroot = 0;
	if (hot) {
		L.HMW = (C + 31) / 32;
		o = (o + 3) & ~(size_t)3;
		L.hu = o; o += 4 * (size_t)W;
		L.hk = o; o += 4 * (size_t)W;
		L.hmask = o; o += 4 * (size_t)W * L.HMW;
		L.hroot = o; o += 4 * (size_t)L.HMW;
	}
	L.bytes = (o + 15) & ~(size_t)15;
	L.dbl = L.gbytes = 0;
	return L;
}

// The wide form.  LDS: the sort buffer (pow2(W) entries), the selection state and the per-frame class arrays, 117,328 bytes at most
// (W = 8192, C = 8192).  Workspace, per utterance, at offsets from its region: the beam state written in step 4, twice (copy 1 at +dbl),
// then own_*, fold and the hash table, rebuilt every frame.
__host__ __device__ static inline BsLayout bs_wide_layout(int W, int N, int C, bool lm = false, bool hot = false) {
	BsLayout L;
	L.W = W; L.NW = (N + 31) / 32; L.C = C;
	L.S = bs_pow2(W > BS_MAX_N ? W : BS_MAX_N);
	L.TB = bs_pow2(2 * W > 64 ? 2 * W : 64);
	L.MW = lm ? (C + 31) / 32 : 0;
	size_t o = 0;
	L.su = o; o += 8 * (size_t)L.S;
	L.plp = o; o += 8 * (size_t)BS_MAX_N;
	L.sel = o; o += (sizeof(BsSel) + 15) & ~(size_t)15;
	L.sk = o; o += 4 * (size_t)L.S;
	L.pc = o; o += 4 * (size_t)BS_MAX_N;
	L.hist = o; o += 4 * 256;
	L.pos = o; o += 2 * (size_t)C;
	L.HMW = 0; L.hu = L.hk = L.hmask = L.hroot = 0;
	if (hot) {
		L.HMW = (C + 31) / 32;
		o = (o + 3) & ~(size_t)3;
		L.hroot = o; o += 4 * (size_t)L.HMW;
	}
	L.bytes = (o + 15) & ~(size_t)15;
	o = 0;
	L.lpb = o; o += 8 * (size_t)W;
	L.lpnb = o; o += 8 * (size_t)W;
	L.tot = o; o += 8 * (size_t)W;
	L.hash = o; o += 8 * (size_t)W;
	L.phash = o; o += 8 * (size_t)W;
	L.lmsp = o; if (lm) o += 8 * (size_t)W;
	L.last = o; o += 4 * (size_t)W;
	L.node = o; o += 4 * (size_t)W;
	L.len = o; o += 4 * (size_t)W;
	L.lnode = o; if (lm) o += 4 * (size_t)W;
	L.lstate = o; if (lm) o += 4 * (size_t)W;
	L.lmask = o; o += 4 * (size_t)W * L.MW;
	if (!lm) L.lmsp = L.lnode = L.lstate = L.lmask = 0;
	if (hot) {
		L.hu = o; o += 4 * (size_t)W;
		L.hk = o; o += 4 * (size_t)W;
		L.hmask = o; o += 4 * (size_t)W * L.HMW;
	}
	L.dbl = (o + 15) & ~(size_t)15;
	o = 2 * L.dbl;
	L.own_nb = o; o += 8 * (size_t)W;
	L.own_nnb = o; o += 8 * (size_t)W;
	L.own_s = o; o += 8 * (size_t)W;
	L.fold = o; o += 4 * (size_t)W * L.NW;
	L.htab = o; o += 4 * (size_t)L.TB;
	L.gbytes = (o + 255) & ~(size_t)255;
	return L;
}

// numpy's npy_logaddexp, so that the kernel and the float64 restatement round the same way
__device__ __forceinline__ double bs_lae(double x, double y) {
	if (x == y) return x + 0.69314718055994530942;
	const double d = x - y;
	if (d > 0) return x + log1p(exp(-d));
	if (d <= 0) return y + log1p(exp(d));
	return d;  // NaN
}

// ascending key of a DEscending score (smaller key = better); -0.0 is folded onto +0.0
__device__ __forceinline__ uint64_t bs_desc64(double x) {
	const uint64_t b = (uint64_t)__double_as_longlong(x + 0.0);
	const uint64_t o = (b >> 63) ? ~b : (b | (1ull << 63));
	return ~o;
}
__device__ __forceinline__ double bs_undesc64(uint64_t u) {
	const uint64_t o = ~u;
	return __longlong_as_double((long long)((o >> 63) ? (o & ~(1ull << 63)) : ~o));
}
__device__ __forceinline__ uint32_t bs_desc32(float x) {
	const uint32_t b = __float_as_uint(x + 0.f);
	const uint32_t o = (b >> 31) ? ~b : (b | 0x80000000u);
	return ~o;
}

__device__ __forceinline__ uint64_t bs_extend_hash(uint64_t h, int c) { return convasr_mix_seed(h ^ ((uint64_t)(c + 1) * 0x9E3779B97F4A7C15ull)); }
#define BS_EMPTY_HASH 0x243F6A8885A308D3ull


// hist[bin] += 1 for every calling lane (bin >= 0).  In the first passes nearly every candidate of a frame falls into one or two bins (the
// scores share sign and exponent), and 64 lanes adding to one LDS word are serialised: the lanes of the wave's two most common bins
// among the callers are counted with a ballot and added by one lane each; the rest add one by one.  Callable from divergent code.
// Only in the 1,024-thread workgroups (W > 256): with 16 waves contending the aggregation took W = 1024 from 106.7 to 86.9 ms
// (64 x 750 frames), with 4 waves the extra ballots cost more than they saved (W = 64: 19.6 -> 21.5 ms).
__device__ __forceinline__ void bs_hist_add(int* hist, int bin) {
	const int lane = threadIdx.x & 63;
	if (blockDim.x <= 256) {
		if (bin >= 0) atomicAdd(&hist[bin], 1);
		return;
	}
#pragma unroll
	for (int r = 0; r < 2; ++r) {
		const uint64_t act = __ballot(bin >= 0);
		if (!act) return;
		const int lead = __shfl(bin, __ffsll((long long)act) - 1, 64);  // (the source lane is active and holds a bin)
		const uint64_t same = __ballot(bin == lead);
		if (bin == lead) {
			if (lane == __ffsll((long long)same) - 1) atomicAdd(&hist[lead], __popcll(same));
			bin = -1;
		}
	}
	if (bin >= 0) atomicAdd(&hist[bin], 1);
}

// Wave 0: the bucket of `hist` where the running count reaches `need`; `all` when the whole histogram holds fewer.
__device__ __forceinline__ void bs_pick(const int* hist, BsSel* s) {
	const int lane = threadIdx.x;
	const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
	const int sum = h0 + h1 + h2 + h3;
	int incl = sum;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const int v = __shfl_up(incl, o, 64);
		if (lane >= o) incl += v;
	}
	const int excl = incl - sum, need = s->need;
	if (excl < need && need <= incl) {
		int b = 4 * lane, before = excl, h = h0;
		while (before + h < need) { before += h; h = hist[++b]; }
		s->bucket = b; s->before = before; s->cnt = h;
	}
	if (lane == 63 && incl < need) s->all = 1;
}

// Radix select of the k best (smallest (u, key)) among the candidates `enumerate` visits; afterwards bs_selected() tells them apart.
// Every thread of the workgroup calls it.  The tie passes cover key bits 0-23, or 0-31 in the wide form (keys of 27 bits).
template <bool WIDE, class E>
__device__ void bs_radix_select(E enumerate, int k, int* hist, BsSel* s) {
	const int tid = threadIdx.x, nth = blockDim.x;
	if (tid == 0) { s->P = 0; s->M = 0; s->KP = 0; s->KM = 0; s->need = k; s->full = 0; s->all = 0; s->tie = 0; }
	__syncthreads();
	for (int shift = 56; shift >= 0; shift -= 8) {
		for (int i = tid; i < 256; i += nth) hist[i] = 0;
		__syncthreads();
		const uint64_t P = s->P, M = s->M;
		enumerate([&](uint64_t u, unsigned) { bs_hist_add(hist, (u & M) == P ? (int)((u >> shift) & 255) : -1); });
		__syncthreads();
		if (tid < 64) bs_pick(hist, s);
		__syncthreads();
		if (s->all) return;
		if (tid == 0) {
			s->P |= (uint64_t)s->bucket << shift; s->M |= 255ull << shift; s->need -= s->before;
			if (s->cnt == s->need) s->full = 1;
		}
		__syncthreads();
		if (s->full) return;
	}
	// more candidates than needed share the boundary score exactly: the smallest keys among them
	if (tid == 0) s->tie = 1;
	for (int shift = WIDE ? 24 : 16; shift >= 0; shift -= 8) {
		for (int i = tid; i < 256; i += nth) hist[i] = 0;
		__syncthreads();
		const uint64_t P = s->P;
		const unsigned KP = s->KP, KM = s->KM;
		enumerate([&](uint64_t u, unsigned key) { bs_hist_add(hist, u == P && (key & KM) == KP ? (int)((key >> shift) & 255) : -1); });
		__syncthreads();
		if (tid < 64) bs_pick(hist, s);
		__syncthreads();
		if (tid == 0) {
			s->KP |= (unsigned)s->bucket << shift; s->KM |= 255u << shift; s->need -= s->before;
			if (s->cnt == s->need) s->full = 1;
		}
		__syncthreads();
		if (s->full) return;
	}
}

__device__ __forceinline__ bool bs_selected(const BsSel& s, uint64_t u, unsigned key) {
	if (s.all || u < s.P) return true;
	if ((u & s.M) != s.P) return false;
	if (!s.tie) return true;
	return key < s.KP || (key & s.KM) == s.KP;
}

// ascending bitonic sort of (su, sk) pairs, S a power of two
__device__ void bs_sort(uint64_t* su, int* sk, int S) {
	const int tid = threadIdx.x, nth = blockDim.x;
	for (int k = 2; k <= S; k <<= 1)
		for (int j = k >> 1; j > 0; j >>= 1) {
			for (int i = tid; i < S; i += nth) {
				const int l = i ^ j;
				if (l > i) {
					const uint64_t a = su[i], b = su[l];
					const int ka = sk[i], kb = sk[l];
					const bool gt = a > b || (a == b && ka > kb);
					if (gt == ((i & k) == 0)) { su[i] = b; su[l] = a; sk[i] = kb; sk[l] = ka; }
				}
			}
			__syncthreads();
		}
}

// ---- LM lookups (lm.py: _hash, NgramLM.log10_cond); every loop is bounded even over tables that break lm.py's invariants
__device__ __forceinline__ unsigned bs_lm_hash(int ctx, int word) {
	unsigned h = ((unsigned)ctx * 0x9E3779B1u) ^ ((unsigned)word * 0x85EBCA77u);
	h ^= h >> 15;
	h *= 0x2C1B3C6Du;
	h ^= h >> 12;
	return h;
}

// the entry (ctx, word) of order >= 2, -1 when the model does not list it; ctx = -1: the unigram entry, which is the word id
__device__ __forceinline__ int bs_lm_find(const BsLm& lm, int ctx, int word) {
	if (ctx < 0) return word;
	unsigned slot = bs_lm_hash(ctx, word) & (unsigned)(lm.n_slots - 1);
	for (int probe = 0; probe < lm.n_slots; ++probe, slot = (slot + 1) & (unsigned)(lm.n_slots - 1)) {
		const int4 v = lm.slots[slot];
		if (v.x == ctx && v.y == word) return v.z;
		if (v.x == BS_LM_EMPTY_KEY) return -1;
	}
	return -1;
}

// log10 P(word | state) by the backoff rule: the first listed (suffix, word), plus the backoff weights of the longer suffixes
__device__ double bs_lm_log10(const BsLm& lm, int s, int word) {
	double acc = 0.0;
	for (int it = 0; it <= BS_LM_MAX_ORDER; ++it) {
		const int e = bs_lm_find(lm, s, word);
		if (e >= 0) return acc + lm.ent_pb[e].x;
		acc += lm.ent_pb[s].y;
		s = lm.ent_sl[s].x;
	}
	return acc + lm.ent_pb[word].x;
}

// the state after `word` follows state s: the longest listed (suffix of s of at most order - 2 words, word)
__device__ int bs_lm_advance(const BsLm& lm, int s, int word) {
	if (lm.order == 1) return -1;
	if (s >= 0 && lm.ent_sl[s].y > lm.order - 2) s = lm.ent_sl[s].x;
	for (int it = 0; it <= BS_LM_MAX_ORDER; ++it) {
		const int e = bs_lm_find(lm, s, word);
		if (e >= 0) return e;
		s = lm.ent_sl[s].x;
	}
	return word;
}

// ---- hot phrases: the state (node, pending) of l + c from that of l (the header's rule).  pmask: the MW mask words cached for l's node
// (zero for a DEAD one), hroot: the root's.  The child index is checked against n_nodes, so a table that breaks hotwords.py's invariants
// gives a wrong state, not a read outside the tables; there is no loop over the tables.
__device__ __forceinline__ void bs_hot_step(const BsHot& hot, const unsigned* pmask, const unsigned* hroot, int MW, int pu, int pk, int plast, int c, int& nu, int& nk) {
	const unsigned* m = nullptr;
	int base = 0;
	nk = 0;
	if ((pmask[c >> 5] >> (c & 31)) & 1u) { m = pmask; base = pu; nk = pk + 1; }
	else if (plast == hot.space && ((hroot[c >> 5] >> (c & 31)) & 1u)) { m = hroot; base = 0; nk = 1; }
	if (m == nullptr) { nu = c == hot.space ? 0 : BS_HOT_DEAD; return; }
	int below = 0;
#pragma unroll
	for (int k = 0; k < BS_LM_MAX_C / 32; ++k)
		if (k < MW) {
			const unsigned bits = m[k];
			if (32 * k + 32 <= c) below += __popc(bits);
			else if (32 * k <= c) below += __popc(bits & ((1u << (c & 31)) - 1u));
		}
	const int v = hot.child[base] + below;
	if ((unsigned)v >= (unsigned)hot.n_nodes) { nu = BS_HOT_DEAD; nk = 0; return; }
	nu = v;
	if (hot.term[v]) nk = 0;
}

template <bool LM, bool WIDE, bool HOT>
__device__ __forceinline__ void bs_body(const float* __restrict__ log_probs, const int64_t* __restrict__ lengths, int64_t* __restrict__ out_tokens,
                                        int* __restrict__ out_offsets, int64_t* __restrict__ out_lengths, void* __restrict__ out_logp,
                                        int2* __restrict__ arena_all, unsigned char* __restrict__ state_all, int T, int C, int blank, int W, int N,
                                        float cutoff_prob, int topk, const BsLm& lm, const BsHot& hot) {
	extern __shared__ __align__(16) unsigned char bs_smem[];
	const BsLayout Ly = WIDE ? bs_wide_layout(W, N, C, LM, HOT) : bs_layout(W, N, C, LM, HOT);
	unsigned char* bm = bs_smem;  // the per-beam arrays: LDS, or in the wide form the utterance's region of the workspace
	if constexpr (WIDE) bm = state_all + (int64_t)blockIdx.x * Ly.gbytes;
	BsSel& s = *(BsSel*)(bs_smem + Ly.sel);  // (dynamic: static LDS would stop the 160 KiB opt-in)
	double* lpb = (double*)(bm + Ly.lpb);
	double* lpnb = (double*)(bm + Ly.lpnb);
	double* tot = (double*)(bm + Ly.tot);
	double* own_nb = (double*)(bm + Ly.own_nb);
	double* own_nnb = (double*)(bm + Ly.own_nnb);
	double* own_s = (double*)(bm + Ly.own_s);
	uint64_t* hash = (uint64_t*)(bm + Ly.hash);
	uint64_t* phash = (uint64_t*)(bm + Ly.phash);
	uint64_t* su = (uint64_t*)(bs_smem + Ly.su);
	double* plp = (double*)(bs_smem + Ly.plp);
	int* last = (int*)(bm + Ly.last);
	int* node = (int*)(bm + Ly.node);
	int* len = (int*)(bm + Ly.len);
	unsigned* fold = (unsigned*)(bm + Ly.fold);
	int* sk = (int*)(bs_smem + Ly.sk);
	int* htab = (int*)(bm + Ly.htab);
	int* pc = (int*)(bs_smem + Ly.pc);
	int* hist = (int*)(bs_smem + Ly.hist);
	short* pos = (short*)(bs_smem + Ly.pos);
	double* lmsp = (double*)(bm + Ly.lmsp);
	int* lnode = (int*)(bm + Ly.lnode);
	int* lstate = (int*)(bm + Ly.lstate);
	unsigned* lmask = (unsigned*)(bm + Ly.lmask);
	int* hu = (int*)(bm + Ly.hu);
	int* hk = (int*)(bm + Ly.hk);
	unsigned* hmask = (unsigned*)(bm + Ly.hmask);
	unsigned* hroot = (unsigned*)(bs_smem + Ly.hroot);
	const int HMW = HOT ? Ly.HMW : 0;
	// delta(l_i, c) of the header: +w on a match; otherwise the pending labels give their bonus back, and a match restarts at a word start
	auto hot_delta = [&](int i, int c) -> double {
		if ((hmask[i * HMW + (c >> 5)] >> (c & 31)) & 1u) return hot.w;
		const double back = -__dmul_rn(hot.w, (double)hk[i]);
		if (last[i] == hot.space && ((hroot[c >> 5] >> (c & 31)) & 1u)) return __dadd_rn(back, hot.w);
		return back;
	};
	int64_t dbl = (int64_t)Ly.dbl;  // wide form: from the copy of the beam state being read to the one step 4 writes
	const int MW = LM ? Ly.MW : 0;
	const int space = LM ? lm.space : -1;
	const double LN10 = 2.302585092994045684;
	const int NW = Ly.NW, TB = Ly.TB;
	const int tid = threadIdx.x, nth = blockDim.x, b = blockIdx.x;
	int64_t Lb = lengths[b];
	Lb = Lb < 0 ? 0 : (Lb > T ? T : Lb);
	int2* arena = arena_all + (int64_t)b * T * W;
	const double NEG = -INFINITY;

	for (int c = tid; c < C; c += nth) pos[c] = -1;
	if (tid == 0) {
		lpb[0] = 0.0; lpnb[0] = NEG; tot[0] = 0.0; hash[0] = BS_EMPTY_HASH; phash[0] = 0; last[0] = -1; node[0] = -1; len[0] = 0;
		s.n = 1; s.np = 0;
	}
	if constexpr (LM) {
		if (tid == 0) { lmsp[0] = 0.0; lnode[0] = 0; lstate[0] = lm.start; }
		for (int k = tid; k < MW; k += nth) lmask[k] = lm.node_mask[k];  // the root's children; the space is not allowed
	}
	if constexpr (HOT) {
		if (tid == 0) { hu[0] = 0; hk[0] = 0; }
		for (int k = tid; k < HMW; k += nth) { const unsigned bits = hot.mask[k]; hmask[k] = bits; hroot[k] = bits; }
	}
	__syncthreads();

	for (int t = 0; t < (int)Lb; ++t) {
		const float* row = log_probs + ((int64_t)b * T + t) * C;
		// ---- 1. P_t
		for (int p = tid; p < s.np; p += nth) pos[pc[p]] = -1;
		if (tid == 0) s.m = 0;
		__syncthreads();
		int np;
		if (N >= C) {
			for (int c = tid; c < C; c += nth) pc[c] = c;
			np = C;
		} else {
			auto classes = [&](auto&& fn) { for (int c = tid; c < C; c += nth) fn(((uint64_t)bs_desc32(row[c]) << 32) | (unsigned)c, 0u); };
			bs_radix_select<WIDE>(classes, N, hist, &s);
			const BsSel sel = s;
			for (int c = tid; c < C; c += nth)
				if (bs_selected(sel, ((uint64_t)bs_desc32(row[c]) << 32) | (unsigned)c, 0u)) pc[atomicAdd(&s.m, 1)] = c;
			np = N;
		}
		__syncthreads();
		if (cutoff_prob < 1.f) {  // the shortest leading run of the sorted P_t whose probability reaches cutoff_prob
			for (int i = tid; i < BS_MAX_N; i += nth) {
				su[i] = i < np ? (((uint64_t)bs_desc32(row[pc[i]]) << 32) | (unsigned)pc[i]) : ~0ull;
				sk[i] = 0;
			}
			__syncthreads();
			bs_sort(su, sk, BS_MAX_N);
			if (tid < 64) {
				const int p0 = 2 * tid, p1 = 2 * tid + 1;
				const int c0 = (int)(su[p0] & 0xffffffffu), c1 = (int)(su[p1] & 0xffffffffu);
				const double v0 = p0 < np ? exp((double)row[c0]) : 0.0, v1 = p1 < np ? exp((double)row[c1]) : 0.0;
				double incl = v0 + v1;
#pragma unroll
				for (int o = 1; o < 64; o <<= 1) {
					const double v = __shfl_up(incl, o, 64);
					if (tid >= o) incl += v;
				}
				const double excl = incl - (v0 + v1);
				const double cum0 = excl + v0, cum1 = excl + v0 + v1;
				const uint64_t hit = __ballot((p0 < np && cum0 >= (double)cutoff_prob) || (p1 < np && cum1 >= (double)cutoff_prob));
				if (tid == 0) s.cut = np;
				if (hit) {
					const int first = __ffsll((long long)hit) - 1;
					if (tid == first) s.cut = (p0 < np && cum0 >= (double)cutoff_prob) ? p0 + 1 : p1 + 1;
				}
				if (p0 < np) pc[p0] = c0;
				if (p1 < np) pc[p1] = c1;
			}
			__syncthreads();
			np = s.cut;
		}
		for (int p = tid; p < np; p += nth) { plp[p] = (double)row[pc[p]]; pos[pc[p]] = (short)p; }
		if (tid == 0) s.np = np;
		// ---- 2. hash table of the current beams, fold masks cleared
		const int n = s.n;
		for (int i = tid; i < TB; i += nth) htab[i] = 0;
		for (int i = tid; i < n * NW; i += nth) fold[i] = 0;
		if (tid == 0) s.m = 0;
		__syncthreads();
		for (int j = tid; j < n; j += nth) {
			const uint64_t h = hash[j];
			int slot = (int)((h ^ (h >> 32)) & (uint64_t)(TB - 1));
			while (atomicCAS(&htab[slot], 0, j + 1) != 0) slot = (slot + 1) & (TB - 1);
		}
		__syncthreads();
		// ---- own candidates (and the folds of extensions into existing beams)
		const int pb = pos[blank];
		for (int j = tid; j < n; j += nth) {
			double nb = NEG, nnb = NEG;
			if (pb >= 0) nb = plp[pb] + tot[j];
			const int lj = last[j];
			const int pl = lj >= 0 ? pos[lj] : -1;
			if (pl >= 0) {
				nnb = plp[pl] + lpnb[j];
				const uint64_t h = phash[j];
				int slot = (int)((h ^ (h >> 32)) & (uint64_t)(TB - 1)), i = -1;
				for (int e; (e = htab[slot]) != 0; slot = (slot + 1) & (TB - 1))
					if (hash[e - 1] == h) { i = e - 1; break; }
				if constexpr (LM)
					if (i >= 0 && !((lmask[i * MW + (lj >> 5)] >> (lj & 31)) & 1u)) i = -1;  // (l_j exists, so l_i + last(l_j) is allowed: never taken)
				if (i >= 0) {
					double e = plp[pl] + (last[i] == lj ? lpb[i] : tot[i]);
					if constexpr (LM)
						if (lj == space) e += lmsp[i];
					if constexpr (HOT) e = __dadd_rn(e, hot_delta(i, lj));
					nnb = bs_lae(nnb, e);
					atomicOr(&fold[i * NW + (pl >> 5)], 1u << (pl & 31));
				}
			}
			own_nb[j] = nb; own_nnb[j] = nnb; own_s[j] = bs_lae(nb, nnb);
		}
		__syncthreads();
		// ---- 3. top W of the candidates (beam i, q): q = 0 its own, q = p + 1 its extension by pc[p]
		const int S = np + 1, total = n * S;
		auto candidates = [&](auto&& fn) {
			int i = tid / S, q = tid % S;
			const int di = nth / S, dq = nth % S;
			for (int e = tid; e < total; e += nth) {
				double sc;
				unsigned key = (unsigned)i << BS_KEY_C_BITS;
				bool ok;
				if (q == 0) { sc = own_s[i]; ok = true; }
				else {
					const int p = q - 1, c = pc[p];
					if constexpr (LM) ok = ((lmask[i * MW + (c >> 5)] >> (c & 31)) & 1u) && !((fold[i * NW + (p >> 5)] >> (p & 31)) & 1u);  // (never the blank)
					else ok = c != blank && !((fold[i * NW + (p >> 5)] >> (p & 31)) & 1u);
					sc = plp[p] + (c == last[i] ? lpb[i] : tot[i]);
					if constexpr (LM)
						if (c == space) sc += lmsp[i];
					if constexpr (HOT) sc = __dadd_rn(sc, hot_delta(i, c));
					key |= (unsigned)(c + 1);
				}
				if (ok && sc > NEG) fn(bs_desc64(sc), key);
				q += dq; i += di;
				if (q >= S) { q -= S; ++i; }
			}
		};
		bs_radix_select<WIDE>(candidates, W, hist, &s);
		{
			const BsSel sel = s;
			candidates([&](uint64_t u, unsigned key) {
				if (bs_selected(sel, u, key)) { const int r = atomicAdd(&s.m, 1); su[r] = u; sk[r] = (int)key; }
			});
		}
		__syncthreads();
		const int m = s.m, Sm = bs_pow2(m);
		for (int r = m + tid; r < Sm; r += nth) { su[r] = ~0ull; sk[r] = 0x7fffffff; }
		__syncthreads();
		bs_sort(su, sk, Sm);
		// ---- 4. the next beams, in rank order.  The LDS form makes one per thread (nth >= W >= m); the wide form up to W / nth per thread, and
		// a beam made there may be the parent another thread still reads: it writes the other copy of the beam state, then swaps.
		if constexpr (WIDE) {
			auto nx = [&](auto* p) { return (decltype(p))((unsigned char*)p + dbl); };
			for (int r = tid; r < m; r += nth) {
				double nlpb = 0, nlpnb = 0, ntot = 0;
				uint64_t nh = 0, nph = 0;
				int nlast = 0, nnode = 0, nlen = 0;
				double nlmsp = 0.0;
				int nlnode = 0, nlstate = 0;
				unsigned nmask[BS_LM_MAX_C / 32];
				int nhu = 0, nhk = 0;
				unsigned nhmask[BS_LM_MAX_C / 32];
				const unsigned key = (unsigned)sk[r];
				const int i = (int)(key >> BS_KEY_C_BITS), c = (int)(key & ((1u << BS_KEY_C_BITS) - 1)) - 1;
				ntot = bs_undesc64(su[r]);
				if (c < 0) {
					nlpb = own_nb[i]; nlpnb = own_nnb[i]; nh = hash[i]; nph = phash[i]; nlast = last[i]; nnode = node[i]; nlen = len[i];
					if constexpr (LM) {
						nlmsp = lmsp[i]; nlnode = lnode[i]; nlstate = lstate[i];
#pragma unroll
						for (int k = 0; k < BS_LM_MAX_C / 32; ++k) nmask[k] = k < MW ? lmask[i * MW + k] : 0u;
					}
					if constexpr (HOT) {
						nhu = hu[i]; nhk = hk[i];
#pragma unroll
						for (int k = 0; k < BS_LM_MAX_C / 32; ++k) nhmask[k] = k < HMW ? hmask[i * HMW + k] : 0u;
					}
				} else {
					nlpb = NEG; nlpnb = ntot; nh = bs_extend_hash(hash[i], c); nph = hash[i]; nlast = c; nlen = len[i] + 1;
					nnode = t * W + r;
					arena[nnode] = make_int2(node[i], c);
					if constexpr (HOT) {
						bs_hot_step(hot, hmask + i * HMW, hroot, HMW, hu[i], hk[i], last[i], c, nhu, nhk);
#pragma unroll
						for (int k = 0; k < BS_LM_MAX_C / 32; ++k) nhmask[k] = (k < HMW && nhu >= 0) ? hot.mask[(int64_t)nhu * HMW + k] : 0u;
					}
					if constexpr (LM) {
						nlstate = lstate[i];
						int word;
						if (c == space) {  // the current word ends: the next one starts at the root, in the state after it
							word = lm.node_word[lnode[i]];
							nlstate = bs_lm_advance(lm, nlstate, word);
							nlnode = 0;
							word = -1;
						} else {  // one trie step: the child's index among its siblings = the parent's children below c
							const int pn = lnode[i];
							int below = 0;
#pragma unroll
							for (int k = 0; k < BS_LM_MAX_C / 32; ++k)
								if (k < MW) {
									unsigned bits = lm.node_mask[(int64_t)pn * MW + k];
									if (32 * k + 32 <= c) below += __popc(bits);
									else if (32 * k <= c) below += __popc(bits & ((1u << (c & 31)) - 1u));
								}
							nlnode = lm.node_child[pn] + below;
							word = lm.node_word[nlnode];
						}
#pragma unroll
						for (int k = 0; k < BS_LM_MAX_C / 32; ++k) nmask[k] = k < MW ? lm.node_mask[(int64_t)nlnode * MW + k] : 0u;
						nlmsp = 0.0;
						if (word >= 0) {  // the current word is in V: the space may follow, with this LM term
							nlmsp = lm.alpha * (bs_lm_log10(lm, nlstate, word) * LN10) + lm.beta;
#pragma unroll
							for (int k = 0; k < BS_LM_MAX_C / 32; ++k)
								if (k == (space >> 5)) nmask[k] |= 1u << (space & 31);
						}
					}
				}
				nx(lpb)[r] = nlpb; nx(lpnb)[r] = nlpnb; nx(tot)[r] = ntot; nx(hash)[r] = nh; nx(phash)[r] = nph; nx(last)[r] = nlast; nx(node)[r] = nnode; nx(len)[r] = nlen;
				if constexpr (LM) {
					nx(lmsp)[r] = nlmsp; nx(lnode)[r] = nlnode; nx(lstate)[r] = nlstate;
#pragma unroll
					for (int k = 0; k < BS_LM_MAX_C / 32; ++k)
						if (k < MW) nx(lmask)[r * MW + k] = nmask[k];
				}
				if constexpr (HOT) {
					nx(hu)[r] = nhu; nx(hk)[r] = nhk;
#pragma unroll
					for (int k = 0; k < BS_LM_MAX_C / 32; ++k)
						if (k < HMW) nx(hmask)[r * HMW + k] = nhmask[k];
				}
			}
			lpb = nx(lpb); lpnb = nx(lpnb); tot = nx(tot); hash = nx(hash); phash = nx(phash); last = nx(last); node = nx(node); len = nx(len);
			if constexpr (LM) { lmsp = nx(lmsp); lnode = nx(lnode); lstate = nx(lstate); lmask = nx(lmask); }
			if constexpr (HOT) { hu = nx(hu); hk = nx(hk); hmask = nx(hmask); }
			dbl = -dbl;
		} else {
			double nlpb = 0, nlpnb = 0, ntot = 0;
			uint64_t nh = 0, nph = 0;
			int nlast = 0, nnode = 0, nlen = 0;
			double nlmsp = 0.0;
			int nlnode = 0, nlstate = 0;
			unsigned nmask[BS_LM_MAX_C / 32];
			int nhu = 0, nhk = 0;
			unsigned nhmask[BS_LM_MAX_C / 32];
			if (tid < m) {
				const unsigned key = (unsigned)sk[tid];
				const int i = (int)(key >> BS_KEY_C_BITS), c = (int)(key & ((1u << BS_KEY_C_BITS) - 1)) - 1;
				ntot = bs_undesc64(su[tid]);
				if (c < 0) {
					nlpb = own_nb[i]; nlpnb = own_nnb[i]; nh = hash[i]; nph = phash[i]; nlast = last[i]; nnode = node[i]; nlen = len[i];
					if constexpr (LM) {
						nlmsp = lmsp[i]; nlnode = lnode[i]; nlstate = lstate[i];
#pragma unroll
						for (int k = 0; k < BS_LM_MAX_C / 32; ++k) nmask[k] = k < MW ? lmask[i * MW + k] : 0u;
					}
					if constexpr (HOT) {
						nhu = hu[i]; nhk = hk[i];
#pragma unroll
						for (int k = 0; k < BS_LM_MAX_C / 32; ++k) nhmask[k] = k < HMW ? hmask[i * HMW + k] : 0u;
					}
				} else {
					nlpb = NEG; nlpnb = ntot; nh = bs_extend_hash(hash[i], c); nph = hash[i]; nlast = c; nlen = len[i] + 1;
					nnode = t * W + tid;
					arena[nnode] = make_int2(node[i], c);
					if constexpr (HOT) {
						bs_hot_step(hot, hmask + i * HMW, hroot, HMW, hu[i], hk[i], last[i], c, nhu, nhk);
#pragma unroll
						for (int k = 0; k < BS_LM_MAX_C / 32; ++k) nhmask[k] = (k < HMW && nhu >= 0) ? hot.mask[(int64_t)nhu * HMW + k] : 0u;
					}
					if constexpr (LM) {
						nlstate = lstate[i];
						int word;
						if (c == space) {  // the current word ends: the next one starts at the root, in the state after it
							word = lm.node_word[lnode[i]];
							nlstate = bs_lm_advance(lm, nlstate, word);
							nlnode = 0;
							word = -1;
						} else {  // one trie step: the child's index among its siblings = the parent's children below c
							const int pn = lnode[i];
							int below = 0;
#pragma unroll
							for (int k = 0; k < BS_LM_MAX_C / 32; ++k)
								if (k < MW) {
									unsigned bits = lm.node_mask[(int64_t)pn * MW + k];
									if (32 * k + 32 <= c) below += __popc(bits);
									else if (32 * k <= c) below += __popc(bits & ((1u << (c & 31)) - 1u));
								}
							nlnode = lm.node_child[pn] + below;
							word = lm.node_word[nlnode];
						}
#pragma unroll
						for (int k = 0; k < BS_LM_MAX_C / 32; ++k) nmask[k] = k < MW ? lm.node_mask[(int64_t)nlnode * MW + k] : 0u;
						nlmsp = 0.0;
						if (word >= 0) {  // the current word is in V: the space may follow, with this LM term
							nlmsp = lm.alpha * (bs_lm_log10(lm, nlstate, word) * LN10) + lm.beta;
#pragma unroll
							for (int k = 0; k < BS_LM_MAX_C / 32; ++k)
								if (k == (space >> 5)) nmask[k] |= 1u << (space & 31);
						}
					}
				}
			}
			__syncthreads();
			if (tid < m) { lpb[tid] = nlpb; lpnb[tid] = nlpnb; tot[tid] = ntot; hash[tid] = nh; phash[tid] = nph; last[tid] = nlast; node[tid] = nnode; len[tid] = nlen; }
			if constexpr (LM) {
				if (tid < m) {
					lmsp[tid] = nlmsp; lnode[tid] = nlnode; lstate[tid] = nlstate;
#pragma unroll
					for (int k = 0; k < BS_LM_MAX_C / 32; ++k)
						if (k < MW) lmask[tid * MW + k] = nmask[k];
				}
			}
			if constexpr (HOT) {
				if (tid < m) {
					hu[tid] = nhu; hk[tid] = nhk;
#pragma unroll
					for (int k = 0; k < BS_LM_MAX_C / 32; ++k)
						if (k < HMW) hmask[tid * HMW + k] = nhmask[k];
				}
			}
		}
		if (tid == 0) s.n = m;
		__syncthreads();
	}

	// ---- results: the best topk beams, walked back through the arena
	const int n = s.n;
	if constexpr (LM || HOT) {  // the end-of-utterance terms, then the beams re-ranked by the result (ties: rank): the LM's F(l), and with hot phrases
		// F_hot(l) = -(w * k), a pending match giving its bonus back; su[] = the returned score
		const double oov = LM ? lm.alpha * -1000.0 + lm.beta : 0.0;
		const int Sn = bs_pow2(n);
		for (int r = tid; r < Sn; r += nth) {
			if (r < n) {
				double fs = tot[r];
				if constexpr (LM) {
					const bool in_v = (lmask[r * MW + (space >> 5)] >> (space & 31)) & 1u;
					const double F = (len[r] == 0 || last[r] == space) ? 0.0 : (in_v ? lmsp[r] : oov);
					fs = fs + F;
				}
				if constexpr (HOT) fs = __dadd_rn(fs, -__dmul_rn(hot.w, (double)hk[r]));
				su[r] = bs_desc64(fs); sk[r] = r;
			} else {
				su[r] = ~0ull; sk[r] = 0x7fffffff;
			}
		}
		__syncthreads();
		bs_sort(su, sk, Sn);
	}
	int64_t* tok_b = out_tokens + (int64_t)b * topk * T;
	int* off_b = out_offsets + (int64_t)b * topk * T;
	for (int64_t e = tid; e < (int64_t)topk * T; e += nth) {
		const int k = (int)(e / T), p = (int)(e % T);
		if (p >= (k < n ? len[(LM || HOT) ? sk[k] : k] : 0)) { tok_b[e] = 0; off_b[e] = 0; }
	}
	for (int k = tid; k < topk; k += nth) {
		if (k < n) {
			const int r = (LM || HOT) ? sk[k] : k;
			int p = len[r] - 1;
			for (int nd = node[r]; nd >= 0 && p >= 0; --p) {
				const int2 v = arena[nd];
				tok_b[(int64_t)k * T + p] = v.y;
				off_b[(int64_t)k * T + p] = nd / W;
				nd = v.x;
			}
			out_lengths[(int64_t)b * topk + k] = len[r];
			if constexpr (LM || HOT) ((double*)out_logp)[(int64_t)b * topk + k] = bs_undesc64(su[k]);
			else ((float*)out_logp)[(int64_t)b * topk + k] = (float)tot[k];
		} else {
			out_lengths[(int64_t)b * topk + k] = 0;
			if constexpr (LM || HOT) ((double*)out_logp)[(int64_t)b * topk + k] = -INFINITY;
			else ((float*)out_logp)[(int64_t)b * topk + k] = -INFINITY;
		}
	}
}

__global__ __launch_bounds__(1024) void ctc_beam_search_kernel(const float* __restrict__ log_probs, const int64_t* __restrict__ lengths,
                                                                int64_t* __restrict__ out_tokens, int* __restrict__ out_offsets,
                                                                int64_t* __restrict__ out_lengths, float* __restrict__ out_logp,
                                                                int2* __restrict__ arena_all, int T, int C, int blank, int W, int N,
                                                                float cutoff_prob, int topk) {
	const BsLm none{};
	const BsHot cold{};
	bs_body<false, false, false>(log_probs, lengths, out_tokens, out_offsets, out_lengths, out_logp, arena_all, nullptr, T, C, blank, W, N, cutoff_prob, topk, none, cold);
}

__global__ __launch_bounds__(1024) void ctc_beam_search_lm_kernel(const float* __restrict__ log_probs, const int64_t* __restrict__ lengths,
                                                                   int64_t* __restrict__ out_tokens, int* __restrict__ out_offsets,
                                                                   int64_t* __restrict__ out_lengths, double* __restrict__ out_logp,
                                                                   int2* __restrict__ arena_all, int T, int C, int blank, int W, int N,
                                                                   float cutoff_prob, int topk, BsLm lm) {
	const BsHot cold{};
	bs_body<true, false, false>(log_probs, lengths, out_tokens, out_offsets, out_lengths, out_logp, arena_all, nullptr, T, C, blank, W, N, cutoff_prob, topk, lm, cold);
}

__global__ __launch_bounds__(1024) void ctc_beam_search_wide_kernel(const float* __restrict__ log_probs, const int64_t* __restrict__ lengths,
                                                                     int64_t* __restrict__ out_tokens, int* __restrict__ out_offsets,
                                                                     int64_t* __restrict__ out_lengths, float* __restrict__ out_logp,
                                                                     int2* __restrict__ arena_all, unsigned char* __restrict__ state_all, int T, int C,
                                                                     int blank, int W, int N, float cutoff_prob, int topk) {
	const BsLm none{};
	const BsHot cold{};
	bs_body<false, true, false>(log_probs, lengths, out_tokens, out_offsets, out_lengths, out_logp, arena_all, state_all, T, C, blank, W, N, cutoff_prob, topk, none, cold);
}

__global__ __launch_bounds__(1024) void ctc_beam_search_lm_wide_kernel(const float* __restrict__ log_probs, const int64_t* __restrict__ lengths,
                                                                        int64_t* __restrict__ out_tokens, int* __restrict__ out_offsets,
                                                                        int64_t* __restrict__ out_lengths, double* __restrict__ out_logp,
                                                                        int2* __restrict__ arena_all, unsigned char* __restrict__ state_all, int T,
                                                                        int C, int blank, int W, int N, float cutoff_prob, int topk, BsLm lm) {
	const BsHot cold{};
	bs_body<true, true, false>(log_probs, lengths, out_tokens, out_offsets, out_lengths, out_logp, arena_all, state_all, T, C, blank, W, N, cutoff_prob, topk, lm, cold);
}

static const char* bs_envelope(int B, int T, int C, int W, int N, int topk, int* code, bool wide = false) {
	*code = CONVASR_EINVAL;
	if (B < 1 || T < 1) return "B and T must be >= 1";
	if (W < 1) return "beam width must be >= 1";
	if (C < 2) return "C must be >= 2";
	if (N < 1 || N > C) return "cutoff_top_n must be in [1, C]";
	if (topk < 1 || topk > W) return "topk must be in [1, beam width]";
	*code = CONVASR_EUNSUPPORTED;
	if (!wide && W > BS_MAX_W) return "beam width > 1024 is outside the supported envelope";
	if (wide && W > BS_WIDE_MAX_W) return "beam width > 8192 is outside the supported envelope";
	if (N > BS_MAX_N) return "cutoff_top_n > 128 is outside the supported envelope";
	if (C > BS_MAX_C) return "C > 8192 is outside the supported envelope";
	if ((int64_t)B * T * W >= (1ll << 31)) return "B * T * beam width >= 2^31 (workspace arena)";
	if ((int64_t)B * topk * T >= (1ll << 31)) return "B * topk * T >= 2^31 (outputs)";
	return nullptr;
}

extern "C" int64_t convasr_ctc_beam_search_workspace_bytes(int B, int T, int C, int W, int N, int topk) {
	int code;
	if (const char* why = bs_envelope(B, T, C, W, N, topk, &code)) return convasr_fail(code, "ctc_beam_search: %s (B %d T %d C %d W %d N %d topk %d)", why, B, T, C, W, N, topk);
	return (int64_t)B * T * W * (int64_t)sizeof(int2);
}

extern "C" int convasr_ctc_beam_search(const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths,
                                       float* log_prob, void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob,
                                       int topk, void* stream) {
	CONVASR_CHECK_ARG(log_probs && lengths && tokens && offsets && out_lengths && log_prob && workspace, "ctc_beam_search: NULL pointer");
	int code;
	if (const char* why = bs_envelope(B, T, C, W, N, topk, &code)) return convasr_fail(code, "ctc_beam_search: %s (B %d T %d C %d W %d N %d topk %d)", why, B, T, C, W, N, topk);
	CONVASR_CHECK_ARG(blank >= 0 && blank < C, "ctc_beam_search: blank %d outside [0, %d)", blank, C);
	CONVASR_CHECK_ARG(cutoff_prob > 0.f && cutoff_prob <= 1.f, "ctc_beam_search: cutoff_prob must be in (0, 1]");
	const BsLayout Ly = bs_layout(W, N, C);
	if (Ly.bytes > 160 * 1024) return convasr_fail(CONVASR_EUNSUPPORTED, "ctc_beam_search: %zu bytes of LDS (W %d N %d C %d)", Ly.bytes, W, N, C);
	const int threads = W <= 256 ? 256 : 1024;
	static unsigned long long set = 0;
	convasr_allow_160k_lds(reinterpret_cast<const void*>(ctc_beam_search_kernel), set);
	hipLaunchKernelGGL(ctc_beam_search_kernel, dim3(B), dim3(threads), Ly.bytes, (hipStream_t)stream, log_probs, lengths, tokens, offsets, out_lengths,
	                   log_prob, (int2*)workspace, T, C, blank, W, N, cutoff_prob, topk);
	CONVASR_CHECK_LAUNCH("ctc_beam_search");
	return 0;
}

// ---- with an n-gram LM
static const char* bs_lm_envelope(int B, int T, int C, int W, int N, int topk, int* code) {
	if (const char* why = bs_envelope(B, T, C, W, N, topk, code)) return why;
	*code = CONVASR_EUNSUPPORTED;
	if (C > BS_LM_MAX_C) return "C > 256 is outside the envelope of the LM search";
	const BsLayout Ly = bs_layout(W, N, C, true);
	if (Ly.bytes > 160 * 1024) return "the beam state exceeds 160 KiB of LDS (LM search: see the header for the largest beam width per C and N)";
	return nullptr;
}

// the LM entry points' checks after the envelope; fills *lm
static int bs_lm_args(const char* fn, int C, int blank, float cutoff_prob, const uint32_t* node_mask, const int32_t* node_child, const int32_t* node_word,
                      int n_nodes, const double* ent_pb, const int32_t* ent_sl, int n_ent, const int32_t* slots, int n_slots, int space, int order,
                      int start_state, double alpha, double beta, BsLm* lm) {
	CONVASR_CHECK_ARG(blank >= 0 && blank < C, "%s: blank %d outside [0, %d)", fn, blank, C);
	CONVASR_CHECK_ARG(cutoff_prob > 0.f && cutoff_prob <= 1.f, "%s: cutoff_prob must be in (0, 1]", fn);
	CONVASR_CHECK_ARG(space >= 0 && space < C && space != blank, "%s: space class %d must be in [0, %d) and differ from the blank %d", fn, space, C, blank);
	CONVASR_CHECK_ARG(order >= 1 && order <= BS_LM_MAX_ORDER, "%s: LM order %d outside [1, %d]", fn, order, BS_LM_MAX_ORDER);
	CONVASR_CHECK_ARG(std::isfinite(alpha) && std::isfinite(beta), "%s: alpha and beta must be finite", fn);
	CONVASR_CHECK_ARG(n_nodes >= 1 && n_ent >= 1, "%s: empty LM tables (%d trie nodes, %d n-gram entries)", fn, n_nodes, n_ent);
	CONVASR_CHECK_ARG(n_slots >= 1 && (n_slots & (n_slots - 1)) == 0, "%s: n_slots %d is not a power of two", fn, n_slots);
	CONVASR_CHECK_ARG(start_state >= -1 && start_state < n_ent, "%s: start state %d outside [-1, %d)", fn, start_state, n_ent);
	lm->node_mask = node_mask; lm->node_child = node_child; lm->node_word = node_word;
	lm->ent_pb = (const double2*)ent_pb; lm->ent_sl = (const int2*)ent_sl; lm->slots = (const int4*)slots;
	lm->n_slots = n_slots; lm->space = space; lm->order = order; lm->start = start_state; lm->alpha = alpha; lm->beta = beta;
	return 0;
}

extern "C" int64_t convasr_ctc_beam_search_lm_workspace_bytes(int B, int T, int C, int W, int N, int topk) {
	int code;
	if (const char* why = bs_lm_envelope(B, T, C, W, N, topk, &code))
		return convasr_fail(code, "ctc_beam_search_lm: %s (B %d T %d C %d W %d N %d topk %d; %zu bytes of LDS)", why, B, T, C, W, N, topk, bs_layout(W, N, C, true).bytes);
	return (int64_t)B * T * W * (int64_t)sizeof(int2);
}

extern "C" int convasr_ctc_beam_search_lm(const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths,
                                          double* log_prob, void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob, int topk,
                                          const uint32_t* node_mask, const int32_t* node_child, const int32_t* node_word, int n_nodes,
                                          const double* ent_pb, const int32_t* ent_sl, int n_ent, const int32_t* slots, int n_slots,
                                          int space, int order, int start_state, double alpha, double beta, void* stream) {
	CONVASR_CHECK_ARG(log_probs && lengths && tokens && offsets && out_lengths && log_prob && workspace, "ctc_beam_search_lm: NULL pointer");
	CONVASR_CHECK_ARG(node_mask && node_child && node_word && ent_pb && ent_sl && slots, "ctc_beam_search_lm: NULL LM table");
	int code;
	if (const char* why = bs_lm_envelope(B, T, C, W, N, topk, &code))
		return convasr_fail(code, "ctc_beam_search_lm: %s (B %d T %d C %d W %d N %d topk %d; %zu bytes of LDS)", why, B, T, C, W, N, topk, bs_layout(W, N, C, true).bytes);
	BsLm lm;
	if (int rc = bs_lm_args("ctc_beam_search_lm", C, blank, cutoff_prob, node_mask, node_child, node_word, n_nodes, ent_pb, ent_sl, n_ent, slots, n_slots, space, order,
	                        start_state, alpha, beta, &lm))
		return rc;
	const BsLayout Ly = bs_layout(W, N, C, true);
	const int threads = W <= 256 ? 256 : 1024;
	static unsigned long long set = 0;
	convasr_allow_160k_lds(reinterpret_cast<const void*>(ctc_beam_search_lm_kernel), set);
	hipLaunchKernelGGL(ctc_beam_search_lm_kernel, dim3(B), dim3(threads), Ly.bytes, (hipStream_t)stream, log_probs, lengths, tokens, offsets, out_lengths,
	                   log_prob, (int2*)workspace, T, C, blank, W, N, cutoff_prob, topk, lm);
	CONVASR_CHECK_LAUNCH("ctc_beam_search_lm");
	return 0;
}

// ---- the wide form: W <= 8192, the beam state in the workspace (bs_wide_layout)
static const char* bs_wide_envelope(int B, int T, int C, int W, int N, int topk, bool lm, int* code) {
	if (const char* why = bs_envelope(B, T, C, W, N, topk, code, true)) return why;
	*code = CONVASR_EUNSUPPORTED;
	if (lm && C > BS_LM_MAX_C) return "C > 256 is outside the envelope of the LM search";
	if (bs_wide_layout(W, N, C, lm).bytes > 160 * 1024) return "the sort buffer and class arrays exceed 160 KiB of LDS";  // (never within the checks above)
	return nullptr;
}

// the arena (B * T * W nodes), rounded up to 256 bytes, then B regions of beam state
static int64_t bs_wide_arena_bytes(int B, int T, int W) { return ((int64_t)B * T * W * (int64_t)sizeof(int2) + 255) & ~(int64_t)255; }
static int64_t bs_wide_workspace(int B, int T, int C, int W, int N, bool lm) { return bs_wide_arena_bytes(B, T, W) + (int64_t)B * (int64_t)bs_wide_layout(W, N, C, lm).gbytes; }

extern "C" int64_t convasr_ctc_beam_search_wide_workspace_bytes(int B, int T, int C, int W, int N, int topk) {
	int code;
	if (const char* why = bs_wide_envelope(B, T, C, W, N, topk, false, &code))
		return convasr_fail(code, "ctc_beam_search_wide: %s (B %d T %d C %d W %d N %d topk %d)", why, B, T, C, W, N, topk);
	return bs_wide_workspace(B, T, C, W, N, false);
}

extern "C" int convasr_ctc_beam_search_wide(const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths,
                                            float* log_prob, void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob,
                                            int topk, void* stream) {
	CONVASR_CHECK_ARG(log_probs && lengths && tokens && offsets && out_lengths && log_prob && workspace, "ctc_beam_search_wide: NULL pointer");
	int code;
	if (const char* why = bs_wide_envelope(B, T, C, W, N, topk, false, &code))
		return convasr_fail(code, "ctc_beam_search_wide: %s (B %d T %d C %d W %d N %d topk %d)", why, B, T, C, W, N, topk);
	CONVASR_CHECK_ARG(blank >= 0 && blank < C, "ctc_beam_search_wide: blank %d outside [0, %d)", blank, C);
	CONVASR_CHECK_ARG(cutoff_prob > 0.f && cutoff_prob <= 1.f, "ctc_beam_search_wide: cutoff_prob must be in (0, 1]");
	const BsLayout Ly = bs_wide_layout(W, N, C);
	const int threads = W <= 256 ? 256 : 1024;
	static unsigned long long set = 0;
	convasr_allow_160k_lds(reinterpret_cast<const void*>(ctc_beam_search_wide_kernel), set);
	unsigned char* state = (unsigned char*)workspace + bs_wide_arena_bytes(B, T, W);
	hipLaunchKernelGGL(ctc_beam_search_wide_kernel, dim3(B), dim3(threads), Ly.bytes, (hipStream_t)stream, log_probs, lengths, tokens, offsets, out_lengths,
	                   log_prob, (int2*)workspace, state, T, C, blank, W, N, cutoff_prob, topk);
	CONVASR_CHECK_LAUNCH("ctc_beam_search_wide");
	return 0;
}

extern "C" int64_t convasr_ctc_beam_search_lm_wide_workspace_bytes(int B, int T, int C, int W, int N, int topk) {
	int code;
	if (const char* why = bs_wide_envelope(B, T, C, W, N, topk, true, &code))
		return convasr_fail(code, "ctc_beam_search_lm_wide: %s (B %d T %d C %d W %d N %d topk %d)", why, B, T, C, W, N, topk);
	return bs_wide_workspace(B, T, C, W, N, true);
}

extern "C" int convasr_ctc_beam_search_lm_wide(const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths,
                                               double* log_prob, void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob, int topk,
                                               const uint32_t* node_mask, const int32_t* node_child, const int32_t* node_word, int n_nodes,
                                               const double* ent_pb, const int32_t* ent_sl, int n_ent, const int32_t* slots, int n_slots,
                                               int space, int order, int start_state, double alpha, double beta, void* stream) {
	CONVASR_CHECK_ARG(log_probs && lengths && tokens && offsets && out_lengths && log_prob && workspace, "ctc_beam_search_lm_wide: NULL pointer");
	CONVASR_CHECK_ARG(node_mask && node_child && node_word && ent_pb && ent_sl && slots, "ctc_beam_search_lm_wide: NULL LM table");
	int code;
	if (const char* why = bs_wide_envelope(B, T, C, W, N, topk, true, &code))
		return convasr_fail(code, "ctc_beam_search_lm_wide: %s (B %d T %d C %d W %d N %d topk %d)", why, B, T, C, W, N, topk);
	BsLm lm;
	if (int rc = bs_lm_args("ctc_beam_search_lm_wide", C, blank, cutoff_prob, node_mask, node_child, node_word, n_nodes, ent_pb, ent_sl, n_ent, slots, n_slots,
	                        space, order, start_state, alpha, beta, &lm))
		return rc;
	const BsLayout Ly = bs_wide_layout(W, N, C, true);
	const int threads = W <= 256 ? 256 : 1024;
	static unsigned long long set = 0;
	convasr_allow_160k_lds(reinterpret_cast<const void*>(ctc_beam_search_lm_wide_kernel), set);
	unsigned char* state = (unsigned char*)workspace + bs_wide_arena_bytes(B, T, W);
	hipLaunchKernelGGL(ctc_beam_search_lm_wide_kernel, dim3(B), dim3(threads), Ly.bytes, (hipStream_t)stream, log_probs, lengths, tokens, offsets, out_lengths,
	                   log_prob, (int2*)workspace, state, T, C, blank, W, N, cutoff_prob, topk, lm);
	CONVASR_CHECK_LAUNCH("ctc_beam_search_lm_wide");
	return 0;
}

// ---- with hot phrases: bs_body<LM, WIDE, true>, the score fp64 on all four
template <bool LM, bool WIDE>
__global__ __launch_bounds__(1024) void ctc_beam_search_hot_kernel(const float* __restrict__ log_probs, const int64_t* __restrict__ lengths,
                                                                    int64_t* __restrict__ out_tokens, int* __restrict__ out_offsets,
                                                                    int64_t* __restrict__ out_lengths, double* __restrict__ out_logp,
                                                                    int2* __restrict__ arena_all, unsigned char* __restrict__ state_all, int T, int C,
                                                                    int blank, int W, int N, float cutoff_prob, int topk, BsLm lm, BsHot hot) {
	bs_body<LM, WIDE, true>(log_probs, lengths, out_tokens, out_offsets, out_lengths, out_logp, arena_all, state_all, T, C, blank, W, N, cutoff_prob, topk, lm, hot);
}

static const char* bs_hot_envelope(int B, int T, int C, int W, int N, int topk, bool lm, bool wide, int* code) {
	if (const char* why = bs_envelope(B, T, C, W, N, topk, code, wide)) return why;
	*code = CONVASR_EUNSUPPORTED;
	if (C > BS_LM_MAX_C) return "C > 256 is outside the envelope of the hot-phrase search";
	if (wide) {
		if (bs_wide_layout(W, N, C, lm, true).bytes > 160 * 1024) return "the sort buffer and class arrays exceed 160 KiB of LDS";  // (never within the checks above)
	} else if (bs_layout(W, N, C, lm, true).bytes > 160 * 1024)
		return "the beam state exceeds 160 KiB of LDS (hot-phrase search: see the header for the largest beam width per C and N)";
	return nullptr;
}

static int64_t bs_hot_workspace(const char* fn, int B, int T, int C, int W, int N, int topk, bool lm, bool wide) {
	int code;
	if (const char* why = bs_hot_envelope(B, T, C, W, N, topk, lm, wide, &code))
		return convasr_fail(code, "%s: %s (B %d T %d C %d W %d N %d topk %d)", fn, why, B, T, C, W, N, topk);
	if (wide) return bs_wide_arena_bytes(B, T, W) + (int64_t)B * (int64_t)bs_wide_layout(W, N, C, lm, true).gbytes;
	return (int64_t)B * T * W * (int64_t)sizeof(int2);
}

// the hot entry points' checks after the envelope; fills *hot
static int bs_hot_args(const char* fn, int C, int blank, int space, const uint32_t* hot_mask, const int32_t* hot_child, const int32_t* hot_term, int n_hot_nodes,
                       int hot_mask_words, double weight, BsHot* hot) {
	CONVASR_CHECK_ARG(hot_mask && hot_child && hot_term, "%s: NULL hot-phrase table", fn);
	CONVASR_CHECK_ARG(blank >= 0 && blank < C, "%s: blank %d outside [0, %d)", fn, blank, C);
	CONVASR_CHECK_ARG(space >= 0 && space < C && space != blank, "%s: space class %d must be in [0, %d) and differ from the blank %d", fn, space, C, blank);
	CONVASR_CHECK_ARG(n_hot_nodes >= 1, "%s: empty hot-phrase tables (%d trie nodes; the root alone is 1)", fn, n_hot_nodes);
	CONVASR_CHECK_ARG(hot_mask_words == (C + 31) / 32, "%s: %d mask words per hot-phrase node, %d classes need %d", fn, hot_mask_words, C, (C + 31) / 32);
	CONVASR_CHECK_ARG(std::isfinite(weight) && weight >= 0.0, "%s: the hot-phrase weight must be finite and >= 0", fn);
	hot->mask = hot_mask; hot->child = hot_child; hot->term = hot_term; hot->n_nodes = n_hot_nodes; hot->space = space; hot->w = weight;
	return 0;
}

template <bool LM, bool WIDE>
static int bs_hot_launch(const char* fn, const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths, double* log_prob,
                         void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob, int topk, const BsLm& lm, const BsHot& hot, void* stream) {
	const BsLayout Ly = WIDE ? bs_wide_layout(W, N, C, LM, true) : bs_layout(W, N, C, LM, true);
	const int threads = W <= 256 ? 256 : 1024;
	static unsigned long long set = 0;
	convasr_allow_160k_lds(reinterpret_cast<const void*>(ctc_beam_search_hot_kernel<LM, WIDE>), set);
	unsigned char* state = WIDE ? (unsigned char*)workspace + bs_wide_arena_bytes(B, T, W) : nullptr;
	hipLaunchKernelGGL((ctc_beam_search_hot_kernel<LM, WIDE>), dim3(B), dim3(threads), Ly.bytes, (hipStream_t)stream, log_probs, lengths, tokens, offsets, out_lengths,
	                   log_prob, (int2*)workspace, state, T, C, blank, W, N, cutoff_prob, topk, lm, hot);
	CONVASR_CHECK_LAUNCH(fn);
	return 0;
}

template <bool WIDE>
static int bs_hot_call(const char* fn, const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths, double* log_prob,
                       void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob, int topk, const uint32_t* hot_mask,
                       const int32_t* hot_child, const int32_t* hot_term, int n_hot_nodes, int hot_mask_words, int space, double weight, void* stream) {
	CONVASR_CHECK_ARG(log_probs && lengths && tokens && offsets && out_lengths && log_prob && workspace, "%s: NULL pointer", fn);
	if (const int64_t rc = bs_hot_workspace(fn, B, T, C, W, N, topk, false, WIDE); rc < 0) return (int)rc;
	CONVASR_CHECK_ARG(cutoff_prob > 0.f && cutoff_prob <= 1.f, "%s: cutoff_prob must be in (0, 1]", fn);
	BsHot hot;
	if (int rc = bs_hot_args(fn, C, blank, space, hot_mask, hot_child, hot_term, n_hot_nodes, hot_mask_words, weight, &hot)) return rc;
	const BsLm none{};
	return bs_hot_launch<false, WIDE>(fn, log_probs, lengths, tokens, offsets, out_lengths, log_prob, workspace, B, T, C, blank, W, N, cutoff_prob, topk, none, hot, stream);
}

template <bool WIDE>
static int bs_lm_hot_call(const char* fn, const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths, double* log_prob,
                          void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob, int topk, const uint32_t* node_mask,
                          const int32_t* node_child, const int32_t* node_word, int n_nodes, const double* ent_pb, const int32_t* ent_sl, int n_ent,
                          const int32_t* slots, int n_slots, int space, int order, int start_state, double alpha, double beta, const uint32_t* hot_mask,
                          const int32_t* hot_child, const int32_t* hot_term, int n_hot_nodes, int hot_mask_words, double weight, void* stream) {
	CONVASR_CHECK_ARG(log_probs && lengths && tokens && offsets && out_lengths && log_prob && workspace, "%s: NULL pointer", fn);
	CONVASR_CHECK_ARG(node_mask && node_child && node_word && ent_pb && ent_sl && slots, "%s: NULL LM table", fn);
	if (const int64_t rc = bs_hot_workspace(fn, B, T, C, W, N, topk, true, WIDE); rc < 0) return (int)rc;
	BsLm lm;
	if (int rc = bs_lm_args(fn, C, blank, cutoff_prob, node_mask, node_child, node_word, n_nodes, ent_pb, ent_sl, n_ent, slots, n_slots, space, order, start_state,
	                        alpha, beta, &lm))
		return rc;
	BsHot hot;
	if (int rc = bs_hot_args(fn, C, blank, space, hot_mask, hot_child, hot_term, n_hot_nodes, hot_mask_words, weight, &hot)) return rc;
	return bs_hot_launch<true, WIDE>(fn, log_probs, lengths, tokens, offsets, out_lengths, log_prob, workspace, B, T, C, blank, W, N, cutoff_prob, topk, lm, hot, stream);
}

extern "C" int64_t convasr_ctc_beam_search_hot_workspace_bytes(int B, int T, int C, int W, int N, int topk) {
	return bs_hot_workspace("ctc_beam_search_hot", B, T, C, W, N, topk, false, false);
}
extern "C" int64_t convasr_ctc_beam_search_hot_wide_workspace_bytes(int B, int T, int C, int W, int N, int topk) {
	return bs_hot_workspace("ctc_beam_search_hot_wide", B, T, C, W, N, topk, false, true);
}
extern "C" int64_t convasr_ctc_beam_search_lm_hot_workspace_bytes(int B, int T, int C, int W, int N, int topk) {
	return bs_hot_workspace("ctc_beam_search_lm_hot", B, T, C, W, N, topk, true, false);
}
extern "C" int64_t convasr_ctc_beam_search_lm_hot_wide_workspace_bytes(int B, int T, int C, int W, int N, int topk) {
	return bs_hot_workspace("ctc_beam_search_lm_hot_wide", B, T, C, W, N, topk, true, true);
}

extern "C" int convasr_ctc_beam_search_hot(const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths,
                                           double* log_prob, void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob, int topk,
                                           const uint32_t* hot_mask, const int32_t* hot_child, const int32_t* hot_term, int n_hot_nodes, int hot_mask_words,
                                           int space, double weight, void* stream) {
	return bs_hot_call<false>("ctc_beam_search_hot", log_probs, lengths, tokens, offsets, out_lengths, log_prob, workspace, B, T, C, blank, W, N, cutoff_prob, topk,
	                          hot_mask, hot_child, hot_term, n_hot_nodes, hot_mask_words, space, weight, stream);
}

extern "C" int convasr_ctc_beam_search_hot_wide(const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths,
                                                double* log_prob, void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob, int topk,
                                                const uint32_t* hot_mask, const int32_t* hot_child, const int32_t* hot_term, int n_hot_nodes,
                                                int hot_mask_words, int space, double weight, void* stream) {
	return bs_hot_call<true>("ctc_beam_search_hot_wide", log_probs, lengths, tokens, offsets, out_lengths, log_prob, workspace, B, T, C, blank, W, N, cutoff_prob, topk,
	                         hot_mask, hot_child, hot_term, n_hot_nodes, hot_mask_words, space, weight, stream);
}

extern "C" int convasr_ctc_beam_search_lm_hot(const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths,
                                              double* log_prob, void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob, int topk,
                                              const uint32_t* node_mask, const int32_t* node_child, const int32_t* node_word, int n_nodes,
                                              const double* ent_pb, const int32_t* ent_sl, int n_ent, const int32_t* slots, int n_slots,
                                              int space, int order, int start_state, double alpha, double beta, const uint32_t* hot_mask,
                                              const int32_t* hot_child, const int32_t* hot_term, int n_hot_nodes, int hot_mask_words, double weight,
                                              void* stream) {
	return bs_lm_hot_call<false>("ctc_beam_search_lm_hot", log_probs, lengths, tokens, offsets, out_lengths, log_prob, workspace, B, T, C, blank, W, N, cutoff_prob,
	                             topk, node_mask, node_child, node_word, n_nodes, ent_pb, ent_sl, n_ent, slots, n_slots, space, order, start_state, alpha, beta,
	                             hot_mask, hot_child, hot_term, n_hot_nodes, hot_mask_words, weight, stream);
}

extern "C" int convasr_ctc_beam_search_lm_hot_wide(const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths,
                                                   double* log_prob, void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob,
                                                   int topk, const uint32_t* node_mask, const int32_t* node_child, const int32_t* node_word, int n_nodes,
                                                   const double* ent_pb, const int32_t* ent_sl, int n_ent, const int32_t* slots, int n_slots,
                                                   int space, int order, int start_state, double alpha, double beta, const uint32_t* hot_mask,
                                                   const int32_t* hot_child, const int32_t* hot_term, int n_hot_nodes, int hot_mask_words, double weight,
                                                   void* stream) {
	return bs_lm_hot_call<true>("ctc_beam_search_lm_hot_wide", log_probs, lengths, tokens, offsets, out_lengths, log_prob, workspace, B, T, C, blank, W, N,
	                            cutoff_prob, topk, node_mask, node_child, node_word, n_nodes, ent_pb, ent_sl, n_ent, slots, n_slots, space, order, start_state, alpha,
	                            beta, hot_mask, hot_child, hot_term, n_hot_nodes, hot_mask_words, weight, stream);
}
