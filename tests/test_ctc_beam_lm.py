"""LM-fused CTC prefix beam search without a GPU: the float64 restatement (tests/_ctc_beam_lm_ref.py) against brute force and hand-worked
backoff arithmetic, the ARPA parser and the vocabulary rules of convasr_amd/lm.py, the host tables against the restatement's full-context
backoff, and the argument envelope of convasr_ctc_beam_search_lm (checked before any launch)."""
import ctypes
import itertools
import math
import os
import sys
import time
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ctc_beam_lm_ref as RL  # noqa: E402
import _ctc_beam_ref as R  # noqa: E402
import _lm_synth  # noqa: E402

from convasr_amd import lm  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
SMALL = os.path.join(ROOT, 'golden', 'lm_small.arpa')
RU_LABELS = 'абвгдеёжзийклмнопрстуфхцчшщъыьэюя*.2 |'  # CharTokenizerLegacy: blank '|' = 37, space = 36


def _log_softmax(x):
	return x - np.logaddexp.reduce(x, axis = -1, keepdims = True)


def _write(tmp_path, name, text, mode = 'w'):
	p = tmp_path / name
	if mode == 'wb':
		p.write_bytes(text)
	else:
		p.write_text(text, encoding = 'utf-8')
	return str(p)


TINY_ARPA = """\\data\\
ngram 1=6
ngram 2=3

\\1-grams:
-0.7	<s>	-0.3
-0.9	</s>
-0.5	ab	-0.2
-0.8	a	-0.4
-0.6	ba
-1.1	bb	-0.1

\\2-grams:
-0.2	<s> ab
-0.3	ab a	-0.05
-0.1	a ba

\\end\\
"""


def test_backoff_against_hand_worked_probabilities():
	"""tests/golden/lm_small.arpa, order 3: each value below is worked out by hand from the file."""
	arpa = lm.read_arpa(SMALL)
	assert arpa.order == 3 and len(arpa.words) == 14 and arpa.ngrams[('код',)] == (-2.5, 0.0) and arpa.ngrams[('он', 'кот')] == (-0.5, 0.0)
	M = lm.NgramLM(SMALL, RU_LABELS)
	cases = [  # (completed words, word, log10 P)
		([], 'как', -0.4),              # <s> как
		([], 'нет', -0.5 + -1.6),       # bow(<s>) + нет
		(['как'], 'дом', -0.1),         # <s> как дом
		(['как', 'дом'], 'да', -0.15),  # как дом да
		(['как', 'дом'], 'кот', -0.2 + -0.3 + -2.0),  # bow(как дом) + bow(дом) + кот
		(['он'], 'код', -0.35 + -2.5),  # <s> он код -> (<s> он: no bow) + bow(он) + код
		(['он'], 'кот', -0.5),          # <s> он кот is not listed; <s> он has no bow -> он кот
		(['да', 'нет'], 'так', 0.0 + -0.2 + -1.7),     # bow(да нет) missing = 0
		(['он', 'кот'], 'дом', 0.0 + -0.4 + -1.8),
		(['я', 'я', 'я', 'кот'], 'да', -0.9),           # context truncated to two words: я кот -> bow 0, кот да
	]
	for words, w, want in cases:
		got_ref = RL.log10_cond(arpa.ngrams, arpa.order, words, w)
		got_tab = M.log10_cond(words, w)
		assert abs(got_ref - want) < 1e-12 and abs(got_tab - want) < 1e-12, (words, w, got_ref, got_tab, want)
	mod = RL.Model(arpa, RU_LABELS, 37, 0.5, 1.5)
	assert abs(mod.term(['он'], 'кот') - (0.5 * (-0.5 * math.log(10)) + 1.5)) < 1e-12


def test_restatement_against_brute_force(tmp_path):
	"""W above the number of reachable prefixes and N = C: every labelling the dictionary allows is returned, with ln P_ctc(l) plus its
	LM terms (one per space, F at the end); none that it forbids is."""
	arpa = lm.read_arpa(_write(tmp_path, 'tiny.arpa', TINY_ARPA))
	rng = np.random.default_rng(99)
	for trial in range(24):
		labels, blank = (('ab |', 3), ('|ab ', 0), ('a b|', 3), ('b|a ', 1))[trial % 4]
		alpha, beta = ((0.6, 1.3), (0.0, 0.0), (1.2, -2.0))[trial % 3]
		M = RL.Model(arpa, labels, blank, alpha, beta)
		L = int(rng.integers(1, 6))
		lp = _log_softmax(rng.normal(size = (L, 4)) * 2.0)
		labs = {lab for lab in _labellings(L, 4, blank) if RL.is_allowed(M, lab)}
		hyps, _ = RL.decode_one(lp, M, 4 ** L + 8, 4, 1.0, 4 ** L + 8)
		assert {tuple(h[0]) for h in hyps} == labs, (labels, L)
		for toks, offs, s in hyps:
			want = R.labelling_log_prob(lp, toks, blank) + RL.lm_terms(M, toks)
			assert abs(want - s) <= 1e-11, (labels, toks, want, s)
			assert offs == sorted(offs)
		assert [h[2] for h in hyps] == sorted((h[2] for h in hyps), reverse = True)


def _labellings(L, C, blank):
	out = set()
	for path in itertools.product(range(C), repeat = L):
		lab, prev = [], None
		for c in path:
			if c != blank and c != prev:
				lab.append(c)
			prev = c
		out.add(tuple(lab))
	return out


def test_restatement_edge_cases():
	"""L = 0: one empty hypothesis of score 0; the dictionary forbids a leading space and two spaces in a row; alpha = beta = 0 keeps the
	dictionary (it is not the LM-free search)."""
	arpa = lm.read_arpa(SMALL)
	M = RL.Model(arpa, RU_LABELS, 37, 0.0, 0.0)
	hyps, _ = RL.decode_one(np.zeros((0, 38)), M, 8, 38, 1.0, 3)
	assert hyps == [([], [], 0.0)]
	sp = 36
	assert not M.allowed('')[sp] and M.allowed('кот')[sp] and not M.allowed('ко')[sp] and not M.allowed('кот')[37]
	assert not RL.is_allowed(M, [sp]) and not RL.is_allowed(M, [M.labels.index('к'), M.labels.index('о'), M.labels.index('т'), sp, sp])
	rng = np.random.default_rng(5)
	lp = _log_softmax(rng.normal(size = (20, 38)) * 3.0).astype(np.float32)
	free, _ = R.decode_one(lp, 37, 16, 38, 1.0, 1)
	fused, _ = RL.decode_one(lp, M, 16, 38, 1.0, 1)
	assert RL.is_allowed(M, fused[0][0]) and not RL.is_allowed(M, free[0][0])


def test_arpa_parser_and_malformed_files(tmp_path):
	arpa = lm.read_arpa(_write(tmp_path, 'ok.arpa', TINY_ARPA))
	assert arpa.order == 2 and arpa.ngrams[('ba',)] == (-0.6, 0.0) and arpa.ngrams[('ab', 'a')] == (-0.3, -0.05) and arpa.words[:3] == ['<s>', '</s>', 'ab']
	bad = {
		'no end': TINY_ARPA.replace('\\end\\\n', ''),
		'count': TINY_ARPA.replace('ngram 2=3', 'ngram 2=4'),
		'fields': TINY_ARPA.replace('-0.1\ta ba', '-0.1\ta ba -0.1 7'),
		'number': TINY_ARPA.replace('-0.6\tba', 'x\tba'),
		'context': TINY_ARPA.replace('-0.1\ta ba', '-0.1\tzz ab'),
		'duplicate': TINY_ARPA.replace('-0.1\ta ba', '-0.1\tab a'),
		'nan': TINY_ARPA.replace('-0.6\tba', 'nan\tba'),
		'section': TINY_ARPA.replace('\\2-grams:', '\\3-grams:'),
		'order 7': '\\data\\\n' + ''.join(f'ngram {k}=0\n' for k in range(1, 8)).replace('ngram 1=0', 'ngram 1=1') + '\n\\1-grams:\n-1\ta\n\n' + ''.join(f'\\{k}-grams:\n\n' for k in range(2, 8)) + '\\end\\\n',
		'counts': TINY_ARPA.replace('ngram 2=3', 'ngram two=3'),
	}
	for what, text in bad.items():
		with pytest.raises(ValueError):
			lm.read_arpa(_write(tmp_path, 'bad.arpa', text))
			pytest.fail(what)
	# a file that is not ARPA text at all: NotImplementedError naming the language model and ARPA
	kenlm = _write(tmp_path, 'model.binary', b'mmap lm http://kheafield.com/code format version 5\n\x00\x00\x01\xff\xfe' + bytes(range(256)), mode = 'wb')
	plain = _write(tmp_path, 'plain.txt', 'hello world\n')
	for path in (str(tmp_path / 'missing.arpa'), kenlm, plain):
		with pytest.raises(NotImplementedError, match = 'language-model.*only ARPA'):
			lm.read_arpa(path)


def test_vocabulary_filtering_and_refusals(tmp_path):
	from convasr_amd import decoders
	M = lm.NgramLM(SMALL, RU_LABELS.upper())  # labels are lowercased, as the reference does
	V = M.vocabulary_of(37)
	assert sorted(V) == ['да', 'дом', 'как', 'код', 'кот', 'нет', 'он', 'она', 'так', 'я']  # not <s> </s> <unk>, not 'cat'
	mask, child, word = M.tables(37)
	assert mask.shape[1] == 2 and word[0] == -1 and (word >= 0).sum() == len(V)
	with pytest.raises(ValueError, match = 'space'):
		lm.NgramLM(SMALL, RU_LABELS.replace(' ', '_'))
	with pytest.raises(ValueError, match = 'space'):
		lm.NgramLM(SMALL, RU_LABELS + ' ')
	with pytest.raises(ValueError, match = 'empty'):
		lm.NgramLM(SMALL, 'xyz |').tables(4)
	single = TINY_ARPA.replace('ab', 'c').replace('bb', 'd').replace('ba', 'e')
	with pytest.raises(NotImplementedError, match = 'character'):
		lm.NgramLM(_write(tmp_path, 's.arpa', single), 'acde |').tables(5)
	tok = types.SimpleNamespace(eps_id = 37, idx2char = list(RU_LABELS))
	with pytest.raises(ValueError, match = 'blank'):  # the space is the blank
		decoders.BeamSearchDecoder(types.SimpleNamespace(eps_id = 36, idx2char = list(RU_LABELS)), lm_path = SMALL, beam_width = 8)
	with pytest.raises(ValueError, match = 'finite'):
		decoders.BeamSearchDecoder(tok, lm_path = SMALL, beam_width = 8, beam_alpha = float('nan'))
	with pytest.raises(NotImplementedError, match = 'language-model'):
		decoders.BeamSearchDecoder(tok, lm_path = str(tmp_path / 'missing.arpa'), beam_width = 8)
	d = decoders.BeamSearchDecoder(tok, lm_path = SMALL, beam_width = 8, beam_alpha = 0.4, beam_beta = 2.6)
	shared = decoders.BeamSearchDecoder(tok, lm_path = d.lm, beam_width = 16)
	assert d.lm is shared.lm and d.blank == 37 and (d.alpha, d.beta) == (0.4, 2.6)


def _find(M, ctx, word):
	"""lm.py's slot table probed the way the kernel's bs_lm_find does."""
	if ctx < 0:
		return word
	n = M.slots.shape[0]
	s = int(lm._hash(ctx, word)) & (n - 1)
	for _ in range(n):
		v = M.slots[s]
		if v[0] == ctx and v[1] == word:
			return int(v[2])
		if v[0] == lm.EMPTY_KEY:
			return -1
		s = (s + 1) & (n - 1)
	return -1


def _table_log10(M, state, word):
	"""bs_lm_log10 over the host tables."""
	acc = 0.0
	while True:
		e = _find(M, state, word)
		if e >= 0:
			return acc + float(M.ent_pb[e, 0])
		acc += float(M.ent_pb[state, 1])
		state = int(M.ent_sl[state, 0])


def _table_advance(M, state, word):
	"""bs_lm_advance over the host tables."""
	if M.order == 1:
		return -1
	if state >= 0 and M.ent_sl[state, 1] > M.order - 2:
		state = int(M.ent_sl[state, 0])
	while True:
		e = _find(M, state, word)
		if e >= 0:
			return e
		state = int(M.ent_sl[state, 0])


def _check_tables(M, arpa, histories):
	wid = M.word_id
	for words, w in histories:
		s = M.start_state
		for x in words:
			s = _table_advance(M, s, wid[x])
		assert s == M.state_of(words), (words, s)
		want = RL.log10_cond(arpa.ngrams, arpa.order, words, w)
		got = _table_log10(M, s, wid[w])
		assert got == want, (words, w, got, want)
	for k, e in list(M.entry_id.items())[:20000]:  # every listed key is found by probing, an absent one is not
		if len(k) > 1:
			assert _find(M, M.entry_id[k[:-1]], wid[k[-1]]) == e


def test_host_tables_against_the_full_context_backoff(tmp_path):
	"""The kernel's state walk (longest listed suffix, hashed full-key lookups) over lm.py's tables gives bit-identical log10 P to the
	restatement's backoff over the full context: on the small model for every history of up to four words, on the order-4 synthetic one of
	10^5 words (generated here) for histories drawn from its own n-grams.  The parse time of the large model is reported."""
	arpa = lm.read_arpa(SMALL)
	M = lm.NgramLM(arpa, RU_LABELS)
	V = sorted(M.vocabulary_of(37))
	hist = [(list(h), w) for n in range(4) for h in itertools.product(['как', 'дом', 'он', 'кот', 'да', 'нет'], repeat = n) for w in V]
	_check_tables(M, arpa, hist)
	path = _lm_synth.write(str(tmp_path / 'big.arpa'))
	t0 = time.perf_counter()
	big = lm.NgramLM(path, RU_LABELS)
	big.tables(37)
	total = time.perf_counter() - t0
	print(f'\norder-4 model of {len(big.arpa.words)} words, {len(big.arpa.ngrams)} n-grams: parse {big.parse_seconds:.2f} s, tables {big.build_seconds:.2f} s, '
	      f'trie + tables {total:.2f} s')
	assert big.order == 4 and len(big.arpa.words) >= 100_000 and total < 120
	rng = np.random.default_rng(3)
	grams = [k for k in big.arpa.ngrams if len(k) >= 2]
	words = [w for w in big.arpa.words if w not in lm.SPECIAL]
	hist = []
	for i in rng.integers(0, len(grams), 3000):
		g = [x for x in grams[i] if x != '<s>']
		cut = int(rng.integers(0, len(g)))
		hist.append((g[:cut], g[cut] if cut < len(g) and g[cut] in big.word_id and g[cut] not in lm.SPECIAL else words[int(rng.integers(len(words)))]))
		hist.append((g, words[int(rng.integers(len(words)))]))
	_check_tables(big, big.arpa, hist)


def test_argument_envelope_of_ctc_beam_search_lm_is_checked_before_any_launch():
	from convasr_amd import _lib
	lib = _lib.load()
	p = ctypes.c_void_p(4096)  # any non-NULL value: never dereferenced
	B, T, C = 2, 10, 38

	def run(W = 8, N = 5, topk = 1, blank = C - 1, cutoff = 1.0, C_ = C, n_nodes = 4, n_ent = 4, n_slots = 8, space = C - 2, order = 3, start = 1,
	        alpha = 0.5, beta = 1.0, ws = p, tab = p):
		return lib.convasr_ctc_beam_search_lm(p, p, p, p, p, p, ws, B, T, C_, blank, W, N, cutoff, topk, tab, p, p, n_nodes, p, p, n_ent, p, n_slots,
		                                      space, order, start, alpha, beta, None)

	for bad in (dict(W = 0), dict(W = 1025), dict(N = 0), dict(N = C + 1), dict(topk = 9), dict(blank = C), dict(cutoff = 0.0), dict(cutoff = 1.5),
	            dict(C_ = 257, N = 40), dict(order = 0), dict(order = 7), dict(alpha = float('nan')), dict(beta = float('inf')), dict(space = C - 1),
	            dict(space = C), dict(space = -1), dict(n_nodes = 0), dict(n_ent = 0), dict(n_slots = 6), dict(n_slots = 0), dict(start = -2),
	            dict(start = 4), dict(ws = None), dict(tab = None), dict(W = 1024, N = 128, C_ = 256, space = 0, blank = 255)):
		rc = run(**bad)
		assert rc < 0 and b'ctc_beam_search_lm' in lib.convasr_last_error(), (bad, rc)
	assert lib.convasr_ctc_beam_search_lm_workspace_bytes(64, 750, C, 1024, 38, 4) == 64 * 750 * 1024 * 8
	assert lib.convasr_ctc_beam_search_lm_workspace_bytes(64, 750, 256, 1024, 64, 4) == 64 * 750 * 1024 * 8
	assert lib.convasr_ctc_beam_search_lm_workspace_bytes(2, 10, 257, 8, 5, 1) < 0
	# the LDS budget: C = 256, N = 128 fits up to W = 1001 (166,992 bytes at W = 1024)
	assert lib.convasr_ctc_beam_search_lm_workspace_bytes(2, 10, 256, 1001, 128, 1) > 0
	assert lib.convasr_ctc_beam_search_lm_workspace_bytes(2, 10, 256, 1002, 128, 1) < 0 and b'LDS' in lib.convasr_last_error()
	assert b'166992 bytes' in (lib.convasr_ctc_beam_search_lm_workspace_bytes(2, 10, 256, 1024, 128, 1), lib.convasr_last_error())[1]
