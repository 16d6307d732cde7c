"""Alignment and error analysis without a GPU: the restatement of convasr_nw_align (tests/_align_ref.py) in its two forms, the host string code
of convasr_amd.metrics (align_strings' two levels, align_words, ErrorTagger, ErrorAnalyzer) fed by that restatement against the reference's
outputs in tests/golden/analysis.json, and the argument envelope of convasr_nw_align, which is checked before any launch.

Every comparison is exact.  The floats of the analysis are ratios of Python integers and in-order sums on both sides."""
import ctypes
import random

import pytest

import _align_ref as A
from _align_golden import check_analysis, load_golden, make_analyzer, ref_aligner, ref_scorer, words_of

P = ctypes.c_void_p(4096)  # any non-NULL, 16-byte aligned value: never dereferenced


@pytest.fixture(scope = 'module')
def golden():
	return load_golden()


def test_restatement_on_hand_computed_cases():
	for f in (A.nw_align_loop, A.nw_align):
		assert f([], [], A.CHAR_SCORES) == ([], [], 0)
		assert f([1, 2], [], A.CHAR_SCORES) == ([0, 1], [-1, -1], 0)
		assert f([], [1, 2], A.CHAR_SCORES) == ([-1, -1], [0, 1], 0)
		assert f([1, 2, 3], [1, 2, 3], A.CHAR_SCORES) == ([0, 1, 2], [0, 1, 2], 15)
		# la >= lb: the lowest row that maximises the last column ends the alignment, the rest of a is the tail
		assert f([7, 1, 2, 9, 9], [1, 2], A.CHAR_SCORES) == ([0, 1, 2, 3, 4], [-1, 0, 1, -1, -1], 10)
		# la < lb: the lowest column that maximises the last row
		assert f([1, 2], [7, 1, 2, 9, 9], A.CHAR_SCORES) == ([-1, 0, 1, -1, -1], [0, 1, 2, 3, 4], 10)
		assert f([1, 1], [1], A.WORD_SCORES) == ([0, 1], [0, -1], 100)  # 'б б' against 'б': row 1 already reaches the maximum
		assert f([1, 3, 2], [1, 2], A.CHAR_SCORES) == ([0, 1, 2], [0, -1, 1], 6)  # a deletion inside: 5 - 4 + 5
		assert f([1, 2], [1, 3, 2, 4], A.CHAR_SCORES) == ([0, -1, 1, -1], [0, 1, 2, 3], 7)  # an insertion inside: 5 - 3 + 5
		# nothing matches: M[1][1] = -3 < 0, the end cell is on the zero border, one side is the tail and the other the prefix
		assert f([1], [2], A.CHAR_SCORES) == ([-1, 0], [0, -1], 0) and f([1], [2, 3], A.CHAR_SCORES) == ([0, -1, -1], [-1, 0, 1], 0)


def test_numpy_restatement_equals_the_loop():
	rng = random.Random(11)
	for n in range(400):
		alpha = rng.choice((2, 3, 38))
		a = [rng.randrange(alpha) for _ in range(rng.randrange(0, 40))]
		b = [rng.randrange(alpha) for _ in range(rng.randrange(0, 40))]
		scores = rng.choice((A.WORD_SCORES, A.CHAR_SCORES, (rng.randint(-3, 9), rng.randint(-9, 4), rng.randint(-9, 2), rng.randint(-9, 2))))
		assert A.nw_align(a, b, scores) == A.nw_align_loop(a, b, scores), (a, b, scores)


def test_restatement_columns_are_an_alignment():
	rng = random.Random(12)
	for n in range(100):
		a = [rng.randrange(3) for _ in range(rng.randrange(0, 30))]
		b = [rng.randrange(3) for _ in range(rng.randrange(0, 30))]
		ia, ib, _ = A.nw_align(a, b, A.CHAR_SCORES)
		assert [i for i in ia if i >= 0] == list(range(len(a))) and [j for j in ib if j >= 0] == list(range(len(b)))
		assert len(ia) == len(ib) <= len(a) + len(b) and all(i >= 0 or j >= 0 for i, j in zip(ia, ib))


def test_scores_are_the_ones_the_reference_runs_with():
	from convasr_amd import metrics
	assert metrics.WORD_ALIGN_SCORES == A.WORD_SCORES == (100, -6, -8, -3) and metrics.CHAR_ALIGN_SCORES == A.CHAR_SCORES == (5, -3, -4, -3)


def test_align_strings_reproduces_the_reference(golden):
	from convasr_amd import metrics
	cases = golden['cases']
	assert len(cases) >= 200 and max(len(c['ref'].split()) for c in cases) >= 1000
	got = metrics.align_strings_batch([c['hyp'] for c in cases], [c['ref'] for c in cases], aligner = ref_aligner)
	for c, g in zip(cases, got):
		assert list(g) == c['align_strings'], (c['hyp'], c['ref'])
	assert metrics.align_strings(hyp = 'б б', ref = 'б', aligner = ref_aligner) == ('б б', 'б |')
	for c in cases[:40]:
		assert list(metrics.align_strings(hyp = c['hyp'], ref = c['ref'], aligner = ref_aligner)) == c['align_strings']


def test_align_strings_batch_makes_two_aligner_calls(golden):
	from convasr_amd import metrics
	calls = []

	def counting(a, b, scores):
		calls.append((len(a), scores))
		return ref_aligner(a, b, scores)

	cases = golden['cases'][:120]
	metrics.align_strings_batch([c['hyp'] for c in cases], [c['ref'] for c in cases], aligner = counting)
	assert [c[1] for c in calls] == [A.WORD_SCORES, A.CHAR_SCORES] and calls[0][0] == len(cases)


def test_align_words_reproduces_the_reference(golden):
	from convasr_amd import metrics
	analyzer = make_analyzer(golden)
	for c in golden['cases']:
		for postproc, key in ((False, 'align_words'), (True, 'align_words_postproc')):
			got = metrics.align_words(*c['align_strings'], word_tagger = analyzer.word_tagger, error_tagger = analyzer.error_tagger, postproc = postproc, compute_cer = True, scorer = ref_scorer)
			assert got == words_of(golden, c[key]), (c['hyp'], c['ref'], postproc)


def test_error_tagger_reproduces_the_reference(golden):
	from convasr_amd import metrics
	tagger = metrics.ErrorTagger()
	seen = set()
	for c in golden['cases']:
		for w in words_of(golden, c['align_words']) + words_of(golden, c['align_words_postproc']):
			assert tagger.tag(hyp = w['hyp'], ref = w['ref'], hyp_tags = w['hyp_tags'], ref_tags = w['ref_tags'])[0] == w['error_tag'], w
			seen.add(w['error_tag'])
	assert seen == {'ok', 'typo_easy', 'typo_hard', 'missing_ref'}  # (align_words tags the words with their placeholders removed, which never gives 'missing')
	assert tagger.tag(hyp = '||||', ref = 'абвг', clamp = True) == ('missing', -2)  # half of the reference or more is unmatched: not a typo
	assert tagger.tag(hyp = 'абв', ref = 'абг', clamp = True) == ('typo_easy', 1) and tagger.tag(hyp = 'абв', ref = 'абв', clamp = True) == ('ok', 0)


def test_analyze_and_aggregate_reproduce_the_reference(golden):
	analyzer = make_analyzer(golden)
	cases = golden['cases']
	results = analyzer.analyze_batch([c['hyp'] for c in cases], [c['ref'] for c in cases], detailed = True, extra = [dict(n = n) for n in range(len(cases))])
	check_analysis(golden, results, analyzer.aggregate(results))
	for n in (0, 5, 8, 40, 150):  # analyze is the batch of one
		c = cases[n]
		assert analyzer.analyze(c['hyp'], c['ref'], detailed = True, extra = dict(n = n)) == results[n]
	plain = analyzer.analyze(cases[40]['hyp'], cases[40]['ref'])
	assert set(plain) == {'ref', 'hyp', 'ref_orig', 'hyp_orig', 'cer', 'wer'} and plain['cer'] == cases[40]['analyze']['cer']


def test_analyze_options():
	from convasr_amd import metrics
	analyzer = metrics.ErrorAnalyzer(aligner = ref_aligner, scorer = ref_scorer, configs = dict(up = dict(postprocessor = 'upper')), postprocessors = dict(upper = str.upper))
	res = analyzer.analyze('мама мыла раму', 'мама мыла рану ; мама', postprocess_fn = str.strip, detailed = True, split_candidates = lambda s: [t.strip() for t in s.split(';')])
	assert (res['hyp'], res['ref']) == ('мама мыла раму', 'мама мыла рану') and res['cer'] == 1 / 12
	assert res['up']['num_words'] == 3 and res['up']['num_words_ok'] == 2 and res['up']['cer_pseudo'] == 0.0 and res['up']['cer_filtered'] == 1 / 12
	assert analyzer.aggregate([res])['up__wer_wordwise'] == 1.0 - 2 / 3


def test_envelope_of_nw_align():
	from convasr_amd import _lib
	lib = _lib.load()

	def run(N = 2, La = 10, Lb = 10, scores = (5, -3, -4, -3), ws_bytes = None, a = P, out = P, ws = P, n_cols = P):
		need = lib.convasr_nw_align_workspace_bytes(N, La, Lb)
		return lib.convasr_nw_align(a, P, P, P, out, P, n_cols, P, ws, need if ws_bytes is None else ws_bytes, N, La, Lb, *scores, None)

	for bad in (dict(N = 0), dict(N = -1), dict(N = 1 << 20), dict(La = -1), dict(Lb = -1), dict(La = 16384), dict(Lb = 16384),
	            dict(scores = (32769, 0, 0, 0)), dict(scores = (0, -32769, 0, 0)), dict(scores = (0, 0, 32769, 0)), dict(scores = (0, 0, 0, -32769)),
	            dict(a = None), dict(out = None), dict(ws = None), dict(n_cols = None), dict(ws_bytes = 0),
	            dict(ws_bytes = lib.convasr_nw_align_workspace_bytes(2, 10, 10) - 1)):
		rc = run(**bad)
		assert rc == -1 and b'nw_align' in lib.convasr_last_error(), (bad, rc)


def test_workspace_query():
	from convasr_amd import _lib
	lib = _lib.load()
	q = lib.convasr_nw_align_workspace_bytes
	formula = lambda N, La, Lb: N * La * ((Lb + 63) // 64) * 16 + N * (La + Lb) * 4
	for N, La, Lb in ((1, 0, 0), (1, 1, 1), (3, 64, 64), (3, 64, 65), (64, 300, 300), (1, 16383, 16383), ((1 << 20) - 1, 16383, 16383), (7, 0, 100), (7, 100, 0)):
		assert q(N, La, Lb) == formula(N, La, Lb), (N, La, Lb)
	assert q(1, 16383, 16383) == 16383 * 256 * 16 + 2 * 16383 * 4
	for N, La, Lb in ((2, 63, 63), (2, 64, 64), (5, 1000, 1024), (100, 16382, 16382)):  # monotone in every argument
		assert q(N, La, Lb) <= q(N + 1, La, Lb) and q(N, La, Lb) <= q(N, La + 1, Lb) and q(N, La, Lb) <= q(N, La, Lb + 1)
	for bad in ((0, 1, 1), (1 << 20, 1, 1), (1, -1, 1), (1, 1, 16384)):
		assert q(*bad) == -1 and b'nw_align' in lib.convasr_last_error(), bad
