"""What the forced-alignment tests share: a numpy float32 restatement of the reference's ctc.alignment (ctc.py:7-75), one utterance at a
time, and a seeded generator of inputs whose best path is known in advance.

The restatement keeps one uint8 back-pointer per (frame, state), so 24,000 frames x 18,001 states cost about 0.4 GB, and one numpy
expression per frame over all states, so that case takes seconds (the oracle's torch restatement, one small tensor op after another on
int64 back-pointers, is there for the short cases)."""
import numpy as np

ZERO = np.float32(np.finfo(np.float32).min)  # the reference's "log zero" (ctc.py:14,29): finfo.min, not -inf


def alignment_one(log_probs, targets, input_length, target_length, blank = 0):
	"""log_probs (T, C) float32 -- ALL frames of the padded batch --, targets (S_max,) ints.  Returns (S_max,) int64: the last frame the best
	path spends in every label's state, 0 for padded labels.

	ctc.py:47-50: prev = (stay, s-1, s-2 where the labels differ else zero); alpha[t] = log_probs[t, ext] + logsumexp(prev); back-pointer =
	argmax(prev), the first maximum.  The sweep covers all T frames, the end state (last label or trailing blank, first maximum) is
	chosen from the column at T-1 (ctc.py:56-61), the walk starts at frame input_length - 1 (ctc.py:61-71), and the scatter of frame
	numbers in increasing order leaves the last frame of every state (ctc.py:72-75).  States past 2 * target_length never feed lower ones
	and the walk never visits them, so they are left out."""
	lp = np.ascontiguousarray(log_probs, dtype = np.float32)
	T = lp.shape[0]
	S, Tb, S_max = int(target_length), int(input_length), len(targets)
	out = np.zeros(S_max, dtype = np.int64)
	if S <= 0 or Tb <= 0:
		return out
	L = 2 * S + 1
	ext = np.full(L, blank, dtype = np.int64)
	ext[1::2] = np.asarray(targets[:S], dtype = np.int64)
	allow2 = np.zeros(L, dtype = bool)
	allow2[2:] = ext[2:] != ext[:-2]
	pad = np.full(L + 2, ZERO, dtype = np.float32)  # alpha behind two "log zero" states, like the reference's zero_padding
	alpha = pad[2:]
	alpha[0] = lp[0, blank]
	alpha[1] = lp[0, ext[1]]
	back = np.zeros((T, L), dtype = np.uint8)
	with np.errstate(over = 'ignore', under = 'ignore'):
		for t in range(1, T):
			stay, one, two = pad[2:], pad[1:-1], np.where(allow2, pad[:-2], ZERO)
			k = np.zeros(L, dtype = np.uint8)
			best = stay.copy()
			m = one > best
			k[m] = 1
			best[m] = one[m]
			m = two > best
			k[m] = 2
			best[m] = two[m]
			back[t] = k
			new = lp[t, ext] + (best + np.log(np.exp(stay - best) + np.exp(one - best) + np.exp(two - best)))
			pad[2:] = new
	alpha = pad[2:]
	s = 2 * S - 1 + int(alpha[2 * S] > alpha[2 * S - 1])
	seen = -1
	for t in range(Tb - 1, -1, -1):
		if s != seen:
			if s & 1:
				out[s >> 1] = t
			seen = s
		if t > 0:
			s -= int(back[t, s])
	return out


def alignment(log_probs_tbc, targets, input_lengths, target_lengths, blank = 0):
	"""The batch form: log_probs (T, B, C), targets (B, S_max) -> (B, S_max) int64."""
	lp = np.asarray(log_probs_tbc, dtype = np.float32)
	return np.stack([alignment_one(lp[:, b], np.asarray(targets[b]), int(input_lengths[b]), int(target_lengths[b]), blank) for b in range(lp.shape[1])])


def planted(seed, T, S, C, blank, boost, input_length = None):
	"""Inputs whose best path is planted: label j sits at frame pos[j], pos[0] in {1, 2}, consecutive labels 2 or 3 frames apart (so a blank
	frame separates any two), every other frame of all T belongs to the blank; randn logits get +boost at the planted class of every
	frame before log_softmax.  All labels lie inside input_length (default T), followed by at least one blank frame.
	Returns (log_probs (T, C) float32, targets (S,) int64, pos (S,) int64)."""
	rng = np.random.RandomState(seed)
	Tb = T if input_length is None else int(input_length)
	pos = np.cumsum(rng.randint(2, 4, size = S)).astype(np.int64) - 1
	assert S >= 1 and pos[-1] < Tb - 1, f'{S} labels need {int(pos[-1]) + 2} frames, {Tb} given'
	targets = rng.randint(0, C - 1, size = S).astype(np.int64)
	targets[targets >= blank] += 1  # any class but the blank
	logits = rng.standard_normal((T, C)).astype(np.float32)
	cls = np.full(T, blank, dtype = np.int64)
	cls[pos] = targets
	logits[np.arange(T), cls] += np.float32(boost)
	x = logits - logits.max(axis = 1, keepdims = True)
	log_probs = x - np.log(np.exp(x).sum(axis = 1, keepdims = True, dtype = np.float32))
	return log_probs.astype(np.float32), targets, pos
