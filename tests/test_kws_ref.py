"""The keyword search's rule on the CPU (include/convasr_hip.h: convasr_ctc_keyword_search): the float32 restatement the kernel is held to
(tests/_kws_ref.py) against the float64 brute force by definition, the properties of the hit picker, a planted phrase, and the wiring of the
new entry points.  No GPU needed."""
import ctypes
import os
import re

import numpy as np

import _kws_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['convasr_ctc_keyword_search', 'convasr_ctc_keyword_search_max_labels', 'convasr_ctc_keyword_search_phrases_per_block',
       'convasr_ctc_keyword_search_staged_classes', 'convasr_ctc_keyword_search_tile_frames']
CASES = 240
_DUMMY = ctypes.create_string_buffer(64)  # stands for every pointer of a call that is refused before it reads one


def dyadic_case(seed):
	"""Log-probs that are multiples of 1/16 in [-4, 0] with about 10 % -inf entries and one zero entry per frame: every sum is exact in
	float32 and float64, and ties are frequent.  T 1-14, C 2-6, L 1-5; every fourth case repeats a label, every fifth has L = 1."""
	rng = np.random.RandomState(seed)
	T, C = rng.randint(1, 15), rng.randint(2, 7)
	L = 1 if seed % 5 == 0 else rng.randint(1, 6)
	lp = -rng.randint(0, 65, size = (T, C)).astype(np.float32) / 16
	lp[rng.rand(T, C) < 0.1] = -np.inf
	lp[np.arange(T), rng.randint(0, C, size = T)] = 0.0
	blank = rng.randint(0, C)
	labels = [c for c in range(C) if c != blank]
	phrase = [labels[rng.randint(len(labels))] for _ in range(L)]
	if seed % 4 == 0 and L > 1:
		j = rng.randint(1, L)
		phrase[j] = phrase[j - 1]
	return lp, phrase, blank, rng


def test_restatement_equals_the_brute_force_at_every_frame():
	repeats = singles = finite = ties = 0
	for seed in range(CASES):
		lp, phrase, blank, _ = dyadic_case(seed)
		T = lp.shape[0]
		score, begin = R.search_dense(lp, T, phrase, blank)
		want_score, want_begin = R.brute_force(lp, phrase, blank)
		assert score.dtype == np.float32 and np.array_equal(score.astype(np.float64), want_score), (seed, score, want_score)
		assert np.array_equal(begin, want_begin), (seed, begin, want_begin)
		assert np.all((begin == -1) == np.isinf(score)) and np.all(score <= 0)
		repeats += any(a == b for a, b in zip(phrase, phrase[1:]))
		singles += len(phrase) == 1
		finite += int(np.isfinite(score).sum())
		ties += len(set(score[np.isfinite(score)].tolist())) < int(np.isfinite(score).sum())
	print(f'{CASES} cases: {repeats} with equal neighbours, {singles} of one label, {finite} finite end frames, {ties} cases with tied scores')
	assert CASES >= 200 and repeats >= 20 and singles >= 20 and finite >= 500 and ties >= 50


def test_a_shorter_length_stops_the_recurrence_and_fills_the_rest():
	lp, phrase, blank, _ = dyadic_case(3)
	T = lp.shape[0]
	for n in range(T + 1):
		score, begin = R.search_dense(lp, n, phrase, blank)
		full = R.search_dense(lp[:n], n, phrase, blank)
		assert np.array_equal(score[:n], full[0]) and np.array_equal(begin[:n], full[1])
		assert np.all(score[n:] == -np.inf) and np.all(begin[n:] == -1)


def test_picker_properties():
	hits_seen = 0
	for seed in range(CASES):
		lp, phrase, blank, rng = dyadic_case(seed)
		T = lp.shape[0]
		score, begin = R.search_dense(lp, T, phrase, blank)
		threshold, min_gap = np.float32(-rng.randint(0, 9) * len(phrase) / 4), int(rng.randint(0, 5))
		hits = R.pick(score, begin, T, threshold, min_gap)
		hits_seen += len(hits)
		for s, b, e in hits:
			assert s >= threshold and 0 <= b <= e < T
			assert score[e] == s and begin[e] == b  # a hit is a frame of E
		for (_, _, e0), (_, b1, e1) in zip(hits, hits[1:]):
			assert e0 < b1 and e0 < e1  # disjoint and ordered
		# a frame at or above the threshold whose begin lies past the previous hit is covered: the first hit that ends at or after t - min_gap
		# (the candidate held at t, or the one the chain from t leads to) exists and is better or equal
		for t in range(T):
			earlier = [h for h in hits if h[2] < t]
			if score[t] >= threshold and begin[t] > (earlier[-1][2] if earlier else -1):
				cover = [h for h in hits if h[2] >= t - min_gap]
				assert cover and cover[0][0] >= score[t], (seed, t, hits)
	print(f'{hits_seen} hits over {CASES} cases')
	assert hits_seen >= 100


PLANT_T, PLANT_C, PLANT_BLANK, PLANT_FIRST, PLANT_LAST, BOOST = 753, 38, 0, 300, 334, 6.0
PLANT_PHRASE = [5, 12, 12, 7, 1, 30, 9, 21, 1, 14, 14, 3]  # 12 labels, 1 the space; two pairs of equal neighbours
ABSENT_PHRASE = [17, 4, 26, 33, 1, 8, 19, 2, 11, 36, 23, 29]
# Measured here with the inputs below: the planted phrase scores 0.0 on (300, 334); its best end frame more than 5 frames away from 334 and the
# absent phrase's best frame are the two numbers the test prints and PLANT_MEASURED records (-13.33 and -41.77); PLANT_THRESHOLD = -1.0 per
# label lies above both.
PLANT_THRESHOLD, PLANT_GAP = -12.0, 20
PLANT_MEASURED = dict(best_elsewhere = -13.3340, best_absent = -41.7670)


def planted_logits():
	"""753 speech-like frames x 38 classes: unit normal logits, boosted by 6.0 along a path of runs of 2-4 frames (60 % blank runs, 3 % spaces)
	into which the phrase is planted at frames 300-334: two frames per label and a blank between labels, blanks on the five frames either side."""
	rng = np.random.RandomState(2026)
	path = np.zeros(PLANT_T, dtype = np.int64)
	t = 0
	while t < PLANT_T:
		run = rng.randint(2, 5)
		u = rng.rand()
		path[t:t + run] = PLANT_BLANK if u < 0.6 else 1 if u < 0.63 else rng.randint(2, PLANT_C)
		t += run
	path[PLANT_FIRST - 5:PLANT_LAST + 6] = PLANT_BLANK
	for j, c in enumerate(PLANT_PHRASE):
		path[PLANT_FIRST + 3 * j:PLANT_FIRST + 3 * j + 2] = c
	assert path[PLANT_LAST] == PLANT_PHRASE[-1] and path[PLANT_LAST + 1] == PLANT_BLANK
	logits = rng.randn(PLANT_T, PLANT_C).astype(np.float32)
	logits[np.arange(PLANT_T), path] += np.float32(BOOST)
	span = slice(PLANT_FIRST - 5, PLANT_LAST + 6)
	assert np.array_equal(logits.argmax(1)[span], path[span])  # (the boost carries these frames: the greedy path IS the planted one)
	return logits


def test_planted_phrase_is_found_once_and_an_absent_one_is_not():
	logits = planted_logits()
	score, begin = R.search_dense(logits, PLANT_T, PLANT_PHRASE, PLANT_BLANK)
	assert score[PLANT_LAST] == 0.0 and begin[PLANT_LAST] == PLANT_FIRST
	away = np.abs(np.arange(PLANT_T) - PLANT_LAST) > 5
	best_elsewhere = float(score[away].max())
	absent, _ = R.search_dense(logits, PLANT_T, ABSENT_PHRASE, PLANT_BLANK)
	best_absent = float(absent.max())
	print(f'planted: 0.0 at ({PLANT_FIRST}, {PLANT_LAST}); best end frame more than 5 frames away {best_elsewhere:.4f}; absent phrase at best {best_absent:.4f}; threshold {PLANT_THRESHOLD}')
	assert best_elsewhere < PLANT_THRESHOLD and best_absent < PLANT_THRESHOLD
	assert abs(best_elsewhere - PLANT_MEASURED['best_elsewhere']) < 1e-3 and abs(best_absent - PLANT_MEASURED['best_absent']) < 1e-3
	hits = R.pick(score, begin, PLANT_T, PLANT_THRESHOLD, PLANT_GAP)
	assert hits == [(0.0, PLANT_FIRST, PLANT_LAST)], hits
	assert R.pick(absent, _, PLANT_T, PLANT_THRESHOLD, PLANT_GAP) == []
	# log-probs instead of logits: only differences within a frame matter (not bit for bit: the log-softmax rounds)
	lp = logits - np.log(np.exp(logits.astype(np.float64)).sum(1, keepdims = True)).astype(np.float32)
	hits_lp = R.pick(*R.search_dense(lp, PLANT_T, PLANT_PHRASE, PLANT_BLANK), PLANT_T, PLANT_THRESHOLD, PLANT_GAP)
	assert [(b, e) for _, b, e in hits_lp] == [(PLANT_FIRST, PLANT_LAST)] and hits_lp[0][0] == 0.0


def test_wiring():
	from convasr_amd import _lib
	header = open(os.path.join(ROOT, 'include', 'convasr_hip.h')).read()
	lib = _lib.load()
	for name in NEW:
		assert re.search(r'\b' + name + r'\s*\(', header), name
		assert name in _lib._SIGNATURES and hasattr(lib, name), name
	assert 'CONVASR_ABI_VERSION 11' in header and lib.convasr_abi_version() == 11
	assert lib.convasr_ctc_keyword_search_max_labels() == 64 and lib.convasr_ctc_keyword_search_phrases_per_block() >= 1
	staged = lib.convasr_ctc_keyword_search_staged_classes()
	for C in (2, 38, 64, 65, staged, staged + 1, 8192):
		assert 1 <= lib.convasr_ctc_keyword_search_tile_frames(C) <= 64
	assert lib.convasr_ctc_keyword_search_tile_frames(1) < 0 and lib.convasr_ctc_keyword_search_tile_frames(8193) < 0
	# the envelope is checked before any launch (no GPU is touched: every refusal precedes the first HIP call)
	one = ctypes.cast(_DUMMY, ctypes.c_void_p)
	base = dict(B = 1, T = 8, C = 4, K = 1, L_max = 2, H = 1, blank = 0, min_gap = 0)
	for kw, code in ((dict(L_max = 65), -3), (dict(L_max = 0), -3), (dict(C = 1), -3), (dict(C = 8193), -3), (dict(T = (1 << 20) + 1), -3), (dict(T = 0), -3), (dict(B = 65536), -3), (dict(K = 65536), -3),
	                 (dict(K = 0), -3), (dict(H = 0), -1), (dict(min_gap = -1), -1), (dict(blank = 4), -1)):
		ints = [dict(base, **kw)[k] for k in ('B', 'T', 'C', 'K', 'L_max', 'H', 'blank', 'min_gap')]
		assert lib.convasr_ctc_keyword_search(*([one] * 9 + [None, None] + ints + [None])) == code, kw
		assert b'ctc_keyword_search' in lib.convasr_last_error()
	assert lib.convasr_ctc_keyword_search(*([one] * 9 + [one, None] + list(base.values()) + [None])) == -1  # one dense pointer without the other
