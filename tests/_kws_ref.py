"""numpy restatement of the keyword search that include/convasr_hip.h defines (convasr_ctc_keyword_search), and a brute force by definition.

`search_dense` / `pick` / `search` restate the rule in float32 with the kernel's operation order -- one subtraction per frame score, one
addition per step -- so the kernel is held to them bit for bit (tests/test_keyword_search_gpu.py).  `brute_force` is the definition itself in
float64: from every start frame a Viterbi over label / blank / label ... with no outer blanks, the maximum per end frame, the earliest start
on ties; tests/test_kws_ref.py holds the restatement against it on inputs whose sums are exact in both precisions.  Shares no code with the
package."""
import types

import numpy as np

NEG = np.float32(-np.inf)


def frame_scores(lp, dtype = np.float32):
	"""d (T, C): lp[t, c] - m_t with m_t the largest entry of the frame, NaNs ignored; a NaN result counts as -inf."""
	lp = np.asarray(lp, dtype = dtype)
	with np.errstate(invalid = 'ignore'):
		m = np.fmax.reduce(lp, axis = 1, keepdims = True)
		d = lp - m
	d[np.isnan(d)] = -np.inf
	return d


def better(s1, b1, s2, b2):
	"""Elementwise: the larger score, among equal scores the smaller begin (-inf always carries -1, so two of them are the same value)."""
	first = (s1 > s2) | ((s1 == s2) & (b1 <= b2))
	return np.where(first, s1, s2), np.where(first, b1, b2)


def plus(s, b, x):
	"""(s, b) + x: one float32 addition; -inf resets begin to -1."""
	s = (s + x).astype(np.float32)
	return s, np.where(s == NEG, -1, b).astype(np.int32)


def search_dense(lp, n, phrase, blank):
	"""E(t) of one utterance and phrase: (score (T,) float32, begin (T,) int32), (-inf, -1) at the frames t >= n."""
	T = lp.shape[0]
	y = np.asarray(phrase, dtype = np.int64)
	L = len(y)
	d = frame_scores(lp[:n])
	A, Ab = np.full(L, NEG), np.full(L, -1, dtype = np.int32)
	Z, Zb = A.copy(), Ab.copy()
	differs = y[1:] != y[:-1]
	score, begin = np.full(T, NEG), np.full(T, -1, dtype = np.int32)
	for t in range(n):
		dy, db = d[t, y], d[t, blank]
		# what may enter label i: for i = 0 a span that opens here; for i > 0 the blank before it, and the label before it unless it is the same label
		es, eb = np.concatenate([[np.float32(0)], Z[:-1]]), np.concatenate([[np.int32(t)], Zb[:-1]]).astype(np.int32)
		cs, cb = better(A, Ab, es, eb)
		if L > 1:
			ps, pb = better(cs[1:], cb[1:], A[:-1], Ab[:-1])
			cs[1:], cb[1:] = np.where(differs, ps, cs[1:]), np.where(differs, pb, cb[1:])
		zs, zb = better(Z, Zb, A, Ab)
		A, Ab = plus(cs, cb, dy)
		Z, Zb = plus(zs, zb, db)
		score[t], begin[t] = A[L - 1], Ab[L - 1]
	return score, begin


def pick(score, begin, n, threshold, min_gap):
	"""The hit picker over E(0 .. n - 1): a list of (score, begin, end)."""
	hits, cand, last_end = [], None, -1
	threshold = np.float32(threshold)
	for t in range(n):
		s, b = score[t], int(begin[t])
		if s >= threshold and b > last_end and (cand is None or s > cand[0] or (s == cand[0] and b == cand[1])):
			cand = (s, b, t)
		if cand is not None and t - cand[2] >= min_gap:
			hits.append(cand)
			last_end, cand = cand[2], None
	if cand is not None:
		hits.append(cand)
	return hits


def search(lp, lengths, phrases, blank, thresholds, min_gap, H, fill = None):
	"""The whole call on lp (B, T, C) float32: count (B, K) int32, score / begin / end (B, K, H) holding the first H hits of a row -- the rest
	keeps `fill` = (score, begin, end) arrays of that shape (what the buffers held before the call) -- and dense_score / dense_begin (B, K, T)."""
	lp = np.asarray(lp, dtype = np.float32)
	B, T, C = lp.shape
	K = len(phrases)
	lengths = [T] * B if lengths is None else [min(max(int(v), 0), T) for v in lengths]
	thresholds = np.broadcast_to(np.asarray(thresholds, dtype = np.float32), (K,))
	count = np.zeros((B, K), dtype = np.int32)
	if fill is None:
		fill = np.full((B, K, H), NEG), np.full((B, K, H), -1, dtype = np.int32), np.full((B, K, H), -1, dtype = np.int32)
	score, begin, end = (a.copy() for a in fill)
	dense_score, dense_begin = np.full((B, K, T), NEG), np.full((B, K, T), -1, dtype = np.int32)
	hits = [[None] * K for _ in range(B)]
	for b in range(B):
		for k, phrase in enumerate(phrases):
			dense_score[b, k], dense_begin[b, k] = search_dense(lp[b], lengths[b], phrase, blank)
			hits[b][k] = pick(dense_score[b, k], dense_begin[b, k], lengths[b], thresholds[k], min_gap)
			count[b, k] = len(hits[b][k])
			for j, (s, bg, e) in enumerate(hits[b][k][:H]):
				score[b, k, j], begin[b, k, j], end[b, k, j] = s, bg, e
	return types.SimpleNamespace(count = count, score = score, begin = begin, end = end, dense_score = dense_score, dense_begin = dense_begin, hits = hits)


def brute_force(lp, phrase, blank):
	"""By definition, in float64: for every start frame s a Viterbi over the states label 0, blank, label 1, ..., label L - 1 that starts IN
	label 0 at frame s; E(t) = the maximum over s of the score of being in label L - 1 at frame t, the earliest s on ties.
	Returns (score (T,) float64, begin (T,) int64), (-inf, -1) where no path ends."""
	d = frame_scores(lp, np.float64)
	T, L = d.shape[0], len(phrase)
	S = 2 * L - 1  # state 2 i: label i, state 2 i + 1: the blank after it
	cls = [phrase[j // 2] if j % 2 == 0 else blank for j in range(S)]
	score, begin = np.full(T, -np.inf), np.full(T, -1, dtype = np.int64)
	for s in range(T):
		v = [-np.inf] * S
		for t in range(s, T):
			if t == s:
				new = [-np.inf] * S
				new[0] = d[t, cls[0]]
			else:
				new = []
				for j in range(S):
					best = v[j]
					if j >= 1:
						best = max(best, v[j - 1])
					if j >= 2 and j % 2 == 0 and cls[j] != cls[j - 2]:
						best = max(best, v[j - 2])
					new.append(best + d[t, cls[j]])
			v = new
			if v[S - 1] > score[t]:  # (strictly: the earliest start stays on ties)
				score[t], begin[t] = v[S - 1], s
	return score, begin
