"""What the star-alignment tests share: a numpy restatement of convasr_star_alignment's rule (include/convasr_hip.h), operation for
operation -- one rounded addition per arc, a maximum with the smallest arc winning ties, one rounded addition of the emission -- so in
float32 it equals the kernel bit for bit; the walk with all four outputs; and a seeded generator of inputs whose best path is known.

The units, states and arc costs are those of tests/_star_ctc_ref.py (units_of, STAR and _shift come from there; `arcs` restates the
table that `lattice` builds inline, and tests/test_star_align_ref.py checks the two against each other through the sum over paths).
dtype = np.float64 serves the brute force of tests/test_star_align_ref.py."""
import types

import numpy as np

import _star_ctc_ref as SR


def arcs(labels, mask, blank, enter, dtype = np.float32):
	"""One utterance: (cls (L,) with SR.STAR for a star, gap of every state's unit or -1, c (5, L): the cost of the arc from s - d into s,
	start (L,), end (L,)); -inf = no such arc / state."""
	ucls, ugap = SR.units_of(labels, mask)
	n = len(ucls)
	L = 2 * n + 1
	cls = np.full(L, blank, dtype = np.int64)
	cls[1::2] = ucls
	gap = np.full(L, -1, dtype = np.int64)
	gap[1::2] = ugap
	is_star = cls == SR.STAR
	enter = dtype(enter)
	c = np.full((5, L), -np.inf, dtype = dtype)
	c[0] = 0
	c[1, 1:] = np.where(is_star[1:], enter, dtype(0))
	for s in range(1, L, 2):
		if s >= 2 and cls[s] != cls[s - 2]:
			c[2, s] = enter if is_star[s] else 0
		if s >= 3 and is_star[s - 2]:
			c[3, s] = 0
			if s >= 4 and cls[s - 4] != cls[s]:
				c[4, s] = 0
	start = np.full(L, -np.inf, dtype = dtype)
	start[0] = 0
	if L > 1:
		start[1] = enter if is_star[1] else 0
	if L > 3 and is_star[1]:
		start[3] = 0
	end = np.full(L, -np.inf, dtype = dtype)
	end[L - 1] = 0
	if L >= 2:
		end[L - 2] = 0
	if n >= 1 and is_star[L - 2]:
		end[L - 3] = 0
		if L >= 4:
			end[L - 4] = 0
	return cls, gap, c, start, end


def align_one(log_probs, labels, mask, input_length, blank, penalty, enter, dtype = np.float32):
	"""log_probs (T, C) -- all frames of the padded batch --, labels (S,), mask (S + 1,) bool.  Returns a namespace: alignment (S,) int64,
	star_begin (S + 1,), star_frames (S + 1,), score (a dtype scalar), path ((Tb,) states, or None without a path)."""
	S, Tb = len(labels), int(input_length)
	out = types.SimpleNamespace(alignment = np.zeros(S, dtype = np.int64), star_begin = np.full(S + 1, -1, dtype = np.int64), star_frames = np.zeros(S + 1, dtype = np.int64),
	                            score = dtype(-np.inf), path = None)
	if Tb <= 0 or Tb > log_probs.shape[0]:
		return out
	lp = np.ascontiguousarray(log_probs[:Tb], dtype = dtype)
	cls, gap, c, start, end = arcs(labels, mask, blank, enter, dtype)
	L = len(cls)
	is_star = cls == SR.STAR
	col = np.where(is_star, 0, cls)
	pen = dtype(penalty)
	em = lambda t: np.where(is_star, pen, lp[t, col]).astype(dtype)
	back = np.zeros((Tb, L), dtype = np.uint8)
	v = start + em(0)
	for t in range(1, Tb):
		best = SR._shift(v, 0) + c[0]
		k = np.zeros(L, dtype = np.uint8)
		for d in range(1, 5):
			cand = SR._shift(v, d) + c[d]
			m = cand > best
			k[m] = d
			best = np.where(m, cand, best)
		back[t] = k
		v = em(t) + best
		assert v.dtype == dtype
	total = v + end
	s = int(np.argmax(total))  # (the first maximum: the smallest state)
	if not np.isfinite(total[s]):
		return out
	out.score = total[s]
	path = np.empty(Tb, dtype = np.int64)
	for t in range(Tb - 1, -1, -1):
		path[t] = s
		if t > 0:
			s -= int(back[t, s])
	out.path = path
	lab = np.cumsum((np.arange(L) % 2 == 1) & ~is_star) - 1  # the label index of a label state
	for t, s in enumerate(path):  # increasing t: the last frame of every label's state stays, the first of every star's
		if s & 1:
			if is_star[s]:
				if out.star_frames[gap[s]] == 0:
					out.star_begin[gap[s]] = t
				out.star_frames[gap[s]] += 1
			else:
				out.alignment[lab[s]] = t
	return out


def align(log_probs_tbc, targets, input_lengths, target_lengths, blank, star_mask, penalty, enter, dtype = np.float32):
	"""The batch form: log_probs (T, B, C), targets (B, S_max), star_mask (B, S_max + 1) -> a namespace of alignment (B, S_max), star_begin,
	star_frames (B, S_max + 1) int64, score (B,) and paths (a list)."""
	lp, targets, star_mask = np.asarray(log_probs_tbc), np.asarray(targets), np.asarray(star_mask).astype(bool)
	B, S_max = targets.shape
	out = types.SimpleNamespace(alignment = np.zeros((B, S_max), dtype = np.int64), star_begin = np.full((B, S_max + 1), -1, dtype = np.int64),
	                            star_frames = np.zeros((B, S_max + 1), dtype = np.int64), score = np.full(B, -np.inf, dtype = dtype), paths = [])
	for b in range(B):
		S = int(target_lengths[b])
		one = align_one(lp[:, b], targets[b, :S], star_mask[b, :S + 1], int(input_lengths[b]), blank, penalty, enter, dtype)
		out.alignment[b, :S], out.star_begin[b, :S + 1], out.star_frames[b, :S + 1], out.score[b] = one.alignment, one.star_begin, one.star_frames, one.score
		out.paths.append(one.path)
	return out


def path_score(log_probs, labels, mask, path, blank, penalty, enter):
	"""The score of a state sequence re-summed in float64 the way the rule adds it up, or None where the sequence is no path of the lattice."""
	cls, gap, c, start, end = arcs(labels, mask, blank, enter, np.float64)
	emit = lambda t, s: float(penalty) if cls[s] == SR.STAR else float(log_probs[t, cls[s]])
	total = start[path[0]] + emit(0, path[0])
	for t in range(1, len(path)):
		d = int(path[t] - path[t - 1])
		if not 0 <= d <= 4:
			return None
		total = emit(t, path[t]) + (total + c[d, path[t]])
	total = total + end[path[-1]]
	return total if np.isfinite(total) else None


def planted(seed, T, labels, C, blank, inserts, boost = 12.0, input_length = None):
	"""Inputs whose best path through the star lattice is known by construction, for star costs well above -boost (a star must beat a frame
	of about -boost and lose to a frame of about 0): label j sits at frame pos[j] with one or two blank frames before it (the layout of
	_ctc_align_ref.planted); inserts = {gap: frames}: before label `gap` (after the last label for gap = len(labels)) stands a run of that
	many frames at which a non-blank class that the transcript does not use (failing that: neither neighbouring label) is boosted, so every transcript label and the blank lie near
	-boost there; every other frame of all T belongs to the blank.  The run has a blank frame on either side.  With a star allowed in every
	gap of `inserts` the best path spends exactly the runs in those stars and no frame in any other; every label sits at pos[j].
	Returns (log_probs (T, C) float32, pos (S,) int64, runs {gap: (begin, frames)})."""
	rng = np.random.RandomState(seed)
	labels = np.asarray(labels, dtype = np.int64)
	S, Tb = len(labels), T if input_length is None else int(input_length)
	cls = np.full(T, blank, dtype = np.int64)
	pos, runs, cur = np.zeros(S, dtype = np.int64), {}, 0
	for j in range(S + 1):
		if j in inserts:
			cur += 1
			near = {blank} | ({int(labels[j - 1])} if j >= 1 else set()) | ({int(labels[j])} if j < S else set())
			# a class the transcript does not use, where there is one: a label of that class a few places on would take the run at ~0 a
			# frame, cheaper than the star, and drag the labels between into it
			foreign = [k for k in range(C) if k != blank and k not in labels] or [k for k in range(C) if k not in near]
			cls[cur:cur + inserts[j]] = foreign[rng.randint(len(foreign))]
			runs[j] = (cur, int(inserts[j]))
			cur += inserts[j]
		if j < S:
			cur += rng.randint(1, 3)
			pos[j] = cur
			cur += 1
	assert cur < Tb, f'the planted path needs {cur + 1} frames, {Tb} given'
	cls[pos] = labels
	logits = rng.standard_normal((T, C)).astype(np.float32)
	logits[np.arange(T), cls] += np.float32(boost)
	x = logits - logits.max(axis = 1, keepdims = True)
	log_probs = x - np.log(np.exp(x).sum(axis = 1, keepdims = True, dtype = np.float32))
	return log_probs.astype(np.float32), pos, runs


def random_labels(seed, S, C, blank):
	"""S labels, any class but the blank, neighbours distinct or not as they fall."""
	labels = np.random.RandomState(seed).randint(0, C - 1, size = S).astype(np.int64)
	labels[labels >= blank] += 1
	return labels
