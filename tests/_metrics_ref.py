"""A Python restatement of the validation metrics (include/convasr_hip.h: convasr_edit_distance, convasr_ctc_greedy_collapse; the reference's
metrics.cer / metrics.wer), written from their definitions.

Two Levenshtein forms: `levenshtein_loop`, the plain double loop over the DP table, and `levenshtein`, a numpy row DP in which each row's
left-to-right dependency D[i][j] = min(E[j], D[i][j-1] + 1) becomes j + a running minimum of E[k] - k (np.minimum.accumulate).  The loop is
the definition; tests check the numpy form against it and use the numpy form for volume."""
import numpy as np


def levenshtein_loop(a, b):
	"""Edit distance between two sequences of hashable items: unit-cost insertion, deletion and substitution."""
	prev = list(range(len(b) + 1))
	for i in range(1, len(a) + 1):
		cur = [i] + [0] * len(b)
		for j in range(1, len(b) + 1):
			cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
		prev = cur
	return prev[-1]


def levenshtein(a, b):
	"""The same distance by the row-minimum DP over integer sequences (a on the outer axis)."""
	a, b = np.asarray(a, dtype = np.int64), np.asarray(b, dtype = np.int64)
	if len(a) == 0 or len(b) == 0:
		return int(len(a) + len(b))
	k = np.arange(len(b) + 1, dtype = np.int64)
	row = k.copy()
	e = np.empty_like(row)
	for i, ai in enumerate(a, 1):
		e[0] = i
		e[1:] = np.minimum(row[1:] + 1, row[:-1] + (b != ai))
		row = np.minimum.accumulate(e - k) + k
	return int(row[-1])


def char_units(tokens, space):
	"""CHARS mode: the tokens that are not `space` (space < 0: all of them)."""
	return [t for t in tokens if space < 0 or t != space]


def word_units(tokens, space):
	"""WORDS mode: the maximal runs of non-space tokens, each as a tuple."""
	words, cur = [], []
	for t in list(tokens) + [space]:
		if t == space:
			if cur:
				words.append(tuple(cur))
			cur = []
		else:
			cur.append(t)
	return words


def _ids(*seqs):
	table = {}
	return [[table.setdefault(u, len(table)) for u in s] for s in seqs]


def edit_distance(hyp, ref, mode, space, loop = False):
	"""(distance, reference units) of one pair of token lists, mode 0 = CHARS, 1 = WORDS."""
	units = char_units if mode == 0 else word_units
	h, r = _ids(units(list(hyp), space), units(list(ref), space))
	return (levenshtein_loop if loop else levenshtein)(r, h), len(r)


def cer(hyp, ref):
	"""The reference's metrics.cer, restated."""
	if hyp == ref:
		return 0.0
	h, r = hyp.replace(' ', '').lower(), ref.replace(' ', '').lower()
	return levenshtein([ord(c) for c in r], [ord(c) for c in h]) / (len(ref.replace(' ', '')) or 1)


def wer(hyp, ref):
	"""The reference's metrics.wer, restated."""
	if hyp == ref:
		return 0.0
	h, r = _ids(hyp.split(), ref.split())
	return levenshtein(r, h) / (len(ref.split()) or 1)


def greedy_collapse(path, n, eps, space, blank_amount_to_space):
	"""GreedyCTCGenerator.generate's token loop (time_stamps None, silence {eps, space}, word start = space) over path[:n]: the tokens after
	the leading eps."""
	out = []
	last, blanks, repeat_ok, started = eps, 0, False, False
	for c in path[:n]:
		if not started:
			if c in (eps, space):
				continue
			started = True
		if c == eps:
			if last == space:
				continue
			repeat_ok = True
			blanks += 1
			if blanks >= blank_amount_to_space:
				out.append(space)
				last = space
			continue
		if c == last and not repeat_ok:
			continue
		repeat_ok = False
		out.append(c)
		last = c
		blanks = 0
	return out
