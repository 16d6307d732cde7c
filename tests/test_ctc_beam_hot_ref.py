"""The hot-phrase rule on the CPU: the float64 restatement (tests/_ctc_beam_hot_ref.py) against a brute force over every labelling,
against the two existing restatements at weight 0, hotwords.HotWords' tables against the string-prefix definition, and the inputs of
the GPU test (tests/_hot_inputs.py) against the events they have to reach."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ctc_beam_hot_ref as RH  # noqa: E402
import _ctc_beam_lm_ref as RL  # noqa: E402
import _ctc_beam_ref as R  # noqa: E402
import _hot_inputs as I  # noqa: E402

from convasr_amd import hotwords, lm  # noqa: E402


def _forward(lp, labels, blank):
	"""ln p(labels | lp) by the CTC forward recursion in float64."""
	L = len(lp)
	ext = [blank]
	for c in labels:
		ext += [c, blank]
	S = len(ext)
	a = np.full(S, -np.inf)
	a[0] = lp[0, blank]
	if S > 1:
		a[1] = lp[0, ext[1]]
	for t in range(1, L):
		n = np.full(S, -np.inf)
		for s in range(S):
			v = a[s]
			if s >= 1:
				v = np.logaddexp(v, a[s - 1])
			if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2]:
				v = np.logaddexp(v, a[s - 2])
			n[s] = v + lp[t, ext[s]]
		a = n
	return float(np.logaddexp(a[-1], a[-2]) if S > 1 else a[-1])


def _random_lp(T, C, seed):
	x = np.random.default_rng(seed).normal(size = (T, C)) * 1.5
	return x - np.logaddexp.reduce(x, axis = -1, keepdims = True)


def _tiny_arpa():
	uni = {'<unk>': (-1.0, 0.0), '<s>': (-99.0, -0.4), '</s>': (-1.1, 0.0), 'a': (-0.7, -0.3), 'ab': (-1.2, -0.2), 'b': (-0.9, -0.1), 'cab': (-1.5, 0.0),
	       'c': (-1.0, -0.25), 'ba': (-1.3, 0.0)}
	ngrams = {(w,): v for w, v in uni.items()}
	ngrams.update({('<s>', 'a'): (-0.3, -0.1), ('b', 'a'): (-0.2, 0.0), ('a', 'ab'): (-0.6, 0.0), ('c', 'b'): (-0.5, 0.0)})
	return lm.Arpa(2, ngrams, list(uni))


BRUTE = [  # (labels, T, phrases)
	('ab |', 6, ['a', 'ab', 'b a']),
	('| abc', 5, ['ab', 'a', 'cab', 'b a', 'c']),
	('a b|c', 5, ['ba', 'b', 'a b']),
]


@pytest.mark.parametrize('with_lm', [False, True])
@pytest.mark.parametrize('labels,T,phrases', BRUTE)
def test_restatement_against_brute_force(labels, T, phrases, with_lm):
	"""Every labelling's ln p + HotWords.bonus (+ the LM terms, over the labellings the dictionary allows) is the restatement's top-k at a
	width that prunes nothing: tokens exactly, scores within 1e-12."""
	C, blank, space = len(labels), labels.index('|'), labels.index(' ')
	if with_lm:
		phrases = [p for p in phrases if all(w in ('a', 'ab', 'b', 'cab', 'c', 'ba') for w in p.split())]
	for w, seed in ((0.7, 1), (3.0, 2), (0.0, 3)):
		lp = _random_lp(T, C, 100 * T + seed)
		hw = hotwords.HotWords(phrases, labels)
		H = RH.Hot(phrases, labels, w)
		M = RL.Model(_tiny_arpa(), labels, blank, 0.6, 0.4) if with_lm else None
		scored = []
		for n in range(T + 1):
			for lab in itertools.product([c for c in range(C) if c != blank], repeat = n):
				if M is not None and not RL.is_allowed(M, lab):
					continue
				p = _forward(lp, list(lab), blank)
				if p == -np.inf:
					continue
				scored.append((p + hw.bonus(lab, w) + (RL.lm_terms(M, lab) if M is not None else 0.0), lab))
		scored.sort(key = lambda e: -e[0])
		topk = 8
		hyps, gap, ev = RH.decode_one(lp, blank, H, len(scored) + 1, C, 1.0, topk, M)
		assert len(hyps) == topk and gap > 1e-9
		for (toks, _, s), (want, lab) in zip(hyps, scored):
			assert tuple(toks) == lab, (w, toks, lab)
			assert abs(s - want) <= 1e-12 * max(1.0, abs(want)), (w, s, want)
		if w > 0:
			assert ev['completed'] > 0 and ev['revoked'] > 0 and ev['folds'] > 0


def _peaked(B, T, C, seed, sharp = 4.0):
	rng = np.random.default_rng(seed)
	x = rng.normal(size = (B, T, C))
	x[np.arange(B)[:, None], np.arange(T)[None, :], rng.integers(0, C, (B, T))] += sharp
	return (x - np.logaddexp.reduce(x, axis = -1, keepdims = True)).astype(np.float32)


def test_weight_zero_is_the_existing_restatements():
	B, T, C, W, topk = 8, 40, 38, 8, 4
	lengths = I.lengths_of(B, T)
	arpa = lm.read_arpa(I.SMALL)
	for phrases in (I.LM_PHRASES, []):
		H = RH.Hot(phrases, I.RU_LABELS, 0.0)
		lp = _peaked(B, T, C, 7)
		want = R.decode(lp, lengths, 37, W, C, 1.0, topk)
		got = RH.decode(lp, lengths, 37, H, W, C, 1.0, topk)
		for a, b in zip(got[:4], want[:4]):
			assert np.array_equal(a, b)
		assert got[4] == want[4]
		for cutoff in (1.0, 0.99):
			M = RL.Model(arpa, I.RU_LABELS, 37, 0.8, 1.0)
			want = RL.decode(lp, lengths, M, W, C, cutoff, topk)
			got = RH.decode(lp, lengths, 37, H, W, C, cutoff, topk, M)
			for a, b in zip(got[:4], want[:4]):
				assert np.array_equal(a, b)
			assert got[4] == want[4]


def _walk(tables, cs):
	"""The node a class sequence reaches in the tables, None when it leaves the trie."""
	mask, child, term = tables
	u = 0
	for c in cs:
		if not (int(mask[u, c >> 5]) >> (c & 31)) & 1:
			return None
		below = sum(bin(int(mask[u, k]) & (0xffffffff if 32 * k + 32 <= c else (1 << (c & 31)) - 1)).count('1') for k in range(c // 32 + 1))
		u = int(child[u]) + below
	return u


def test_hotwords_tables_against_the_string_prefix_definition():
	rng = np.random.default_rng(5)
	labels = I.RU_LABELS
	letters = list(I.ALPHA[:6])
	for trial in range(20):
		phrases = []
		for _ in range(int(rng.integers(1, 12))):
			words = [''.join(rng.choice(letters, size = int(rng.integers(1, 4)))) for _ in range(int(rng.integers(1, 3)))]
			phrases.append(' '.join(words))
		hw = hotwords.HotWords(['  ' + phrases[0].upper() + ' '] + phrases, labels)  # (a duplicate after normalisation)
		H = RH.Hot(phrases, labels, 1.0)
		tables = hw.tables(37)
		mask, child, term = tables
		assert mask.dtype == np.uint32 and mask.shape == (hw.num_nodes, 2) and child.dtype == np.int32 and term.dtype == np.int32
		assert hw.num_nodes == len(H.prefixes) + 1 and len(hw.phrases) == len(set(phrases))
		seen = {0}
		for pre in H.prefixes:
			u = _walk(tables, pre)
			assert u is not None and u not in seen
			seen.add(u)
			assert bool(term[u]) == (pre in H.phrases)
		for pre in list(H.prefixes) + [()]:
			u = _walk(tables, pre)
			kids = [c for c in range(len(labels)) if pre + (c,) in H.prefixes]
			assert [c for c in range(len(labels)) if (int(mask[u, c >> 5]) >> (c & 31)) & 1] == kids
			assert [_walk(tables, pre + (c,)) for c in kids] == list(range(int(child[u]), int(child[u]) + len(kids)))  # contiguous, in class order
		# bonus = the restatement's deltas + the end term, on random labellings over the phrases' letters and the space
		for _ in range(30):
			toks = [int(c) for c in rng.choice([labels.index(ch) for ch in letters[:3] + [' ']], size = int(rng.integers(0, 12)))]
			state, last, total = ((), 0), -1, 0.0
			for c in toks:
				d, state, _ = H.step(state, last, c)
				total += d * 0.7
				last = c
			assert abs(hw.bonus(toks, 0.7) - (total - 0.7 * state[1])) < 1e-12
	assert hotwords.HotWords([], labels).num_nodes == 1


def test_hotwords_errors():
	labels = I.RU_LABELS
	with pytest.raises(ValueError, match = 'empty phrase'):
		hotwords.HotWords(['кот', '  '], labels)
	with pytest.raises(ValueError, match = 'no label'):
		hotwords.HotWords(['cat'], labels)
	with pytest.raises(ValueError, match = 'blank'):
		hotwords.HotWords(['ко|т'], labels).tables(37)
	with pytest.raises(ValueError, match = 'exactly one space'):
		hotwords.HotWords(['кот'], I.ALPHA + '|')
	with pytest.raises(ValueError, match = 'exactly one space'):
		hotwords.HotWords(['кот'], I.ALPHA + '  |')
	model = lm.NgramLM(I.SMALL, labels)
	with pytest.raises(ValueError, match = 'кошка'):
		hotwords.HotWords(['кот', 'он кошка'], labels).check_vocabulary(model, 37)
	hotwords.HotWords(I.LM_PHRASES, labels).check_vocabulary(model, 37)


@pytest.mark.parametrize('form', ['free', 'lm'])
def test_the_gpu_inputs_reach_every_event(form):
	"""The rows of _hot_inputs.CASES the GPU test runs at W <= 64, T <= 60: each has a seed among six with a margin above GAP, and per
	form every event counter is reached -- so the GPU comparison cannot pass by never leaving the root."""
	arpa = lm.read_arpa(I.SMALL)
	total = dict.fromkeys(RH.EVENTS, 0)
	for row in I.CASES:
		labels, weight, B, T, W, N, topk, cutoff = row
		if W > 64 or T > 60:
			continue
		lp, lengths, ref = I.form_case(form, arpa, *row)
		assert ref[4] > I.GAP
		assert T == 1 or (ref[2][:, 0] > 0).any()  # (with the LM a frame without an allowed class ends an utterance's search: that path is compared too)
		for k in RH.EVENTS:
			total[k] += ref[5][k]
		if T > 1 and W > 1:
			assert ref[5]['completed'] > 0 and ref[5]['folds'] > 0, (row, ref[5])
	assert all(total[k] > 0 for k in RH.EVENTS), total
