"""Inputs of the hot-phrase beam-search tests, shared by test_ctc_beam_hot_ref.py (which asserts on the CPU that they exercise the
rule) and test_ctc_beam_hot_gpu.py (which compares the kernels on them): utterances that spell hot phrases, truncated hot phrases and
other words over noisy log-probs, and the search of the first seed among six whose restatement has a decision margin above GAP."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ctc_beam_hot_ref as RH  # noqa: E402
import _ctc_beam_lm_ref as RL  # noqa: E402

GAP = 1e-9  # (test_ctc_beam_lm_gpu.GAP, test_ctc_beam_search_gpu.GAP)
ROOT = os.path.dirname(os.path.abspath(__file__))
SMALL = os.path.join(ROOT, 'golden', 'lm_small.arpa')
ALPHA = 'абвгдеёжзийклмнопрстуфхцчшщъыьэюя'
RU_LABELS = ALPHA + '*.2 |'                 # space 36, blank '|' 37
LABELS_MID = ALPHA[:5] + '|' + ALPHA[5:19] + ' ' + ALPHA[19:] + '*.2'  # blank 5, space 20
LM_WORDS = ['да', 'нет', 'кот', 'код', 'дом', 'как', 'так', 'он', 'она', 'я']  # the words of lm_small.arpa these labels spell
# 'он' is a prefix of 'она', 'как дом' and 'дом да нет' have inner spaces, every word is a word of the small LM
LM_PHRASES = ['кот', 'как дом', 'да', 'он', 'она', 'дом да нет']
# without an LM also words it does not list
FREE_PHRASES = LM_PHRASES + ['кошка', 'так себе', 'кода']
FREE_WORDS = LM_WORDS + ['кошки', 'себя', 'тактика', 'ёж', 'дома']


LM_ALPHA, LM_BETA = 0.5, 1.0
WMAX = 1024  # the largest width the hot LDS forms accept at C = 38 (asserted against the workspace queries by the GPU test)
# the searches compared on the GPU, per form: (labels, weight, B, T, W, N, topk, cutoff_prob)
CASES = [
	(RU_LABELS, 0.7, 8, 1, 8, 40, 4, 1.0),
	(RU_LABELS, 3.0, 8, 60, 1, 40, 1, 1.0),
	(RU_LABELS, 0.7, 8, 60, 8, 10, 4, 1.0),
	(RU_LABELS, 3.0, 8, 60, 64, 40, 4, 1.0),
	(RU_LABELS, 0.7, 8, 200, 64, 40, 1, 1.0),
	(RU_LABELS, 3.0, 8, 60, 16, 40, 4, 0.99),
	(LABELS_MID, 0.7, 8, 60, 64, 40, 4, 1.0),
	(RU_LABELS, 0.7, 8, 60, WMAX, 40, 4, 1.0),
	(RU_LABELS, 3.0, 4, 60, 2048, 40, 4, 1.0),  # the wide form
]


def form_case(form, arpa, labels, weight, B, T, W, N, topk, cutoff):
	"""case() of one row of CASES for form 'free' (no LM) or 'lm' (arpa: the small model's lm.Arpa)."""
	blank = labels.index('|')
	if form == 'free':
		return case(B, T, labels, blank, FREE_PHRASES, FREE_WORDS, weight, W, N, topk, cutoff)
	return case(B, T, labels, blank, LM_PHRASES, LM_WORDS, weight, W, N, topk, cutoff, lm = (arpa, LM_ALPHA, LM_BETA))


def lengths_of(B, T):
	"""test_ctc_beam_lm_gpu._lengths: ragged, with the lengths 0 and 1."""
	return np.array([T, 0, 1, max(T // 2, 1), max(T - 7, 1), max(3 * T // 4, 1), min(17, T), T][:B], dtype = np.int64)


def spelled(B, T, labels, blank, phrases, words, seed, sharp = 3.5):
	"""(B, T, C) float32 log-probs: per utterance a sequence of hot phrases, hot phrases cut short and other words, each label held for one
	or two frames with blanks in between, as a bump of `sharp` on unit normal noise."""
	labels = list(labels)
	C = len(labels)
	cls = {}
	for c, ch in enumerate(labels):
		cls.setdefault(ch, c)
	rng = np.random.default_rng(seed)
	x = rng.normal(size = (B, T, C))
	for b in range(B):
		frames = []
		while len(frames) < T:
			kind = int(rng.integers(0, 4))
			if kind == 0:
				s = phrases[int(rng.integers(len(phrases)))]
			elif kind == 1:
				p = phrases[int(rng.integers(len(phrases)))]
				s = p[:int(rng.integers(1, len(p) + 1))].strip()
			elif kind == 2:  # a phrase cut short and carried on with another word's tail
				p, w = phrases[int(rng.integers(len(phrases)))], words[int(rng.integers(len(words)))]
				s = (p[:int(rng.integers(1, len(p) + 1))] + w[1:]).strip()
			else:
				s = words[int(rng.integers(len(words)))]
			for ch in s + ' ':
				frames += [cls[ch]] * int(rng.integers(1, 3))
				if rng.random() < 0.5:
					frames.append(blank)
		x[b, np.arange(T), frames[:T]] += sharp
	return (x - np.logaddexp.reduce(x, axis = -1, keepdims = True)).astype(np.float32)


def case(B, T, labels, blank, phrases, words, weight, W, N, topk, cutoff = 1.0, lm = None, seed0 = 0):
	"""The first seed among six whose restatement has a margin above GAP: (lp, lengths, reference outputs incl. min_gap and events).
	lm: None or (arpa, alpha, beta)."""
	C = len(labels)
	H = RH.Hot(phrases, labels, weight)
	M = None if lm is None else RL.Model(lm[0], labels, blank, lm[1], lm[2])
	lengths = lengths_of(B, T)
	for seed in range(seed0, seed0 + 6):
		lp = spelled(B, T, labels, blank, phrases, words, 1000 * T + 10 * W + seed)
		ref = RH.decode(lp, lengths, blank, H, W, min(N, C), float(np.float32(cutoff)), topk, M)
		if ref[4] > GAP:
			return lp, lengths, ref
	raise AssertionError(f'no seed with a decision margin above {GAP} for T {T} W {W} N {N}')
