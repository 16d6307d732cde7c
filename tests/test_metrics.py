"""Validation metrics without a GPU: the argument envelopes of convasr_edit_distance and convasr_ctc_greedy_collapse (checked before any
launch), the host-side string preparation of metrics.cer_wer, and the Python restatement in tests/_metrics_ref.py on hand-computed cases."""
import ctypes
import random

import numpy as np
import torch

import _metrics_ref as R

P = ctypes.c_void_p(4096)  # any non-NULL value: never dereferenced


def _lib():
	from convasr_amd import _lib
	return _lib.load()


def test_envelope_of_edit_distance():
	lib = _lib()

	def run(B = 2, K = 1, Lh = 10, Lr = 10, mode = 0, space = -1, rs = 10, ls = 1, hyp = P, dist = P):
		return lib.convasr_edit_distance(hyp, P, P, rs, P, ls, dist, P, B, K, Lh, Lr, mode, space, None)

	for bad in (dict(B = 0), dict(K = 0), dict(B = 1024, K = 1024), dict(B = -1), dict(Lh = 16384), dict(Lr = 16384), dict(Lh = -1), dict(Lr = -1),
	            dict(mode = 2), dict(mode = -1), dict(mode = 1, space = -1), dict(rs = -1), dict(ls = -1), dict(hyp = None), dict(dist = None)):
		rc = run(**bad)
		assert rc == -1 and b'edit_distance' in lib.convasr_last_error(), (bad, rc)
	from convasr_amd import _lib as L
	assert (L.METRIC_CHARS, L.METRIC_WORDS, L.METRIC_MAX_LEN) == (0, 1, 16383)


def test_envelope_of_ctc_greedy_collapse():
	lib = _lib()

	def run(B = 2, T = 10, eps = 37, space = 36, bats = 10, path = P, out = P):
		return lib.convasr_ctc_greedy_collapse(path, P, out, P, B, T, eps, space, bats, None)

	for bad in (dict(B = 0), dict(T = 0), dict(B = 1 << 16, T = 1 << 15), dict(eps = 5, space = 5), dict(eps = -1), dict(space = -2),
	            dict(bats = -1), dict(path = None), dict(out = None)):
		rc = run(**bad)
		assert rc == -1 and b'ctc_greedy_collapse' in lib.convasr_last_error(), (bad, rc)


def test_host_string_preparation():
	from convasr_amd import metrics
	h, r, n = metrics.char_units(['Привет Мир', 'İ x', 'a\tb\nc'], ['привет  мир', 'i\tX', ' '])
	assert h[0] == r[0] == [ord(c) for c in 'приветмир']
	assert h[1] == [ord('i'), 0x307, ord('x')]  # 'İ'.lower() is two codepoints; only U+0020 is removed
	assert r[1] == [ord('i'), 9, ord('x')]
	assert h[2] == [ord(c) for c in 'a\tb\nc'] and r[2] == []
	assert n == [9, 3, 1]  # len(ref.replace(' ', '')) or 1, before lowercasing
	assert len('İ'.replace(' ', '')) == 1 and len('İ'.lower()) == 2
	h, r, n = metrics.word_units(['a b\tc', 'x\ny  ', 'A a'], ['a  c', ' \t', 'a'])
	assert h[0] == [0, 1, 2] and r[0] == [0, 2]
	assert len(h[1]) == 2 and r[1] == []
	assert h[2][0] != h[2][1] and h[2][1] == r[2][0]  # WER does not lowercase
	assert n == [2, 1, 1]


def test_restatement_on_hand_computed_cases():
	for f in (R.levenshtein, R.levenshtein_loop):
		assert f([ord(c) for c in 'kitten'], [ord(c) for c in 'sitting']) == 3
		assert f([ord(c) for c in 'sitting'], [ord(c) for c in 'kitten']) == 3
		assert f([], []) == 0 and f([1, 2, 3], []) == 3 and f([], [4, 5]) == 2
		assert f([1, 2, 3], [1, 2, 3]) == 0 and f([1, 2, 3], [3, 2, 1]) == 2
		assert f([ord(c) for c in 'flaw'], [ord(c) for c in 'lawn']) == 2
	assert R.cer('kitten', 'sitting') == 3 / 7 and R.cer('', '') == 0.0 and R.cer('abc', '') == 3.0 and R.cer('', 'a b') == 1.0
	assert R.cer('Hello World', 'hello world') == 0.0 and R.cer('İ', 'i') == 1.0
	assert R.wer('the cat sat', 'the cat sat down') == 0.25 and R.wer('a b', '') == 2.0 and R.wer('A b', 'a b') == 0.5
	assert R.edit_distance([5, 0, 0, 6, 7, 0], [0, 5, 6, 7], 1, 0) == (2, 1)  # words (5) (6 7) against (5 6 7)
	assert R.edit_distance([5, 0, 6, 7], [5, 0, 6, 8, 0, 9], 1, 0) == (2, 3)
	assert R.edit_distance([5, 0, 6], [5, 6], 0, 0) == (0, 2)
	assert R.word_units([0, 0, 1, 2, 0, 0, 3, 0], 0) == [(1, 2), (3, )]


def test_numpy_restatement_equals_the_loop():
	rng = random.Random(5)
	for n in range(300):
		alpha = rng.choice((2, 3, 38))
		a = [rng.randrange(alpha) for _ in range(rng.randrange(0, 40))]
		b = [rng.randrange(alpha) for _ in range(rng.randrange(0, 40))]
		assert R.levenshtein(a, b) == R.levenshtein_loop(a, b), (a, b)
		for mode in (0, 1):
			assert R.edit_distance(a, b, mode, 0) == R.edit_distance(a, b, mode, 0, loop = True)


def test_greedy_restatement_equals_the_host_generator():
	"""GreedyCTCGenerator.generate on CPU log-probs (its host loop) against the restatement the GPU test compares the kernel with."""
	from convasr_amd.transcript_generators import CharTokenizerLegacy, GreedyCTCGenerator
	tok = CharTokenizerLegacy('абвгдеёжзийклмнопрстуфхцчшщъыьэюя')
	C, eps, space = tok.vocab_size, tok.eps_id, tok.space_id
	g = torch.Generator().manual_seed(3)
	B, T = 24, 120
	path = torch.randint(0, C, (B, T), generator = g)
	pick = torch.rand(B, T, generator = g)
	path[pick < 0.45] = eps
	path[(pick >= 0.45) & (pick < 0.6)] = space
	path[:, 1:][pick[:, 1:] > 0.85] = path[:, :-1][pick[:, 1:] > 0.85]
	path[0], path[1] = eps, space
	lengths = torch.randint(1, T + 1, (B,), generator = g)
	lp = torch.nn.functional.one_hot(path, C).permute(0, 2, 1).float()
	for bats in (1, 3, 10):
		out = GreedyCTCGenerator(bats).generate(tok, lp, torch.zeros(B), torch.ones(B), output_lengths = lengths)
		for b in range(B):
			want = tok.decode([R.greedy_collapse(path[b].tolist(), int(lengths[b]), eps, space, bats)])[0]
			got = out[b][0][0]['hyp'] if len(out[b][0]) else ''
			assert got == want, (bats, b)
