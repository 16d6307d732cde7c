"""convasr_nw_align on the GPU against its Python restatement (tests/_align_ref.py), exactly: index arrays, column counts and scores; and the
analysis built on it -- metrics.align_strings / ErrorAnalyzer.analyze_batch against the reference's outputs (tests/golden/analysis.json),
train.evaluate_model(error_analyzer = ...) and transcribe.transcribe_batch with align_words."""
import random
import types

import pytest
import torch

import _align_ref as A
from _align_golden import check_analysis, load_golden, make_analyzer, ref_aligner, words_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope = 'module')
def golden():
	return load_golden()


def run(pairs, scores, **kwargs):
	"""ops.nw_align over a list of (a, b) id lists -> per pair (a_index, b_index, score), the rows cut at n_cols; checks the -1 fill."""
	from convasr_amd import ops
	N = len(pairs)
	La, Lb = max(len(a) for a, b in pairs), max(len(b) for a, b in pairs)
	ta, tb = torch.zeros(N, La, dtype = torch.int32), torch.zeros(N, Lb, dtype = torch.int32)
	for p, (a, b) in enumerate(pairs):
		ta[p, :len(a)], tb[p, :len(b)] = torch.tensor(a, dtype = torch.int32), torch.tensor(b, dtype = torch.int32)
	al, bl = torch.tensor([len(a) for a, b in pairs]), torch.tensor([len(b) for a, b in pairs])
	ai, bi, n, score = [t.cpu() for t in ops.nw_align(ta.to(DEV), al.to(DEV), tb.to(DEV), bl.to(DEV), scores, **kwargs)]
	assert ai.shape == bi.shape == (N, La + Lb) and ai.dtype == bi.dtype == n.dtype == score.dtype == torch.int32
	out = []
	for p in range(N):
		k = int(n[p])
		assert bool((ai[p, k:] == -1).all()) and bool((bi[p, k:] == -1).all())
		out.append((ai[p, :k].tolist(), bi[p, :k].tolist(), int(score[p])))
	return out


def check(pairs, scores, **kwargs):
	got = run(pairs, scores, **kwargs)
	for (a, b), g in zip(pairs, got):
		assert g == A.nw_align(a, b, scores), (len(a), len(b), scores)
	return got


def seq(rng, n, alpha):
	return [rng.randrange(alpha) for _ in range(n)]


def noisy_copy(rng, a, alpha, p = 0.08):
	out = []
	for x in a:
		r = rng.random()
		if r < p / 3:
			continue
		out.append(rng.randrange(alpha) if r < 2 * p / 3 else x)
		if r > 1 - p / 3:
			out.append(rng.randrange(alpha))
	return out


SCORE_SETS = [A.WORD_SCORES, A.CHAR_SCORES, (3, 1, -2, -5), (7, -4, -1, -6), (1, -1, -1, -1), (2, 2, -3, -2), (32768, -32768, -32768, -32768)]


@pytest.mark.parametrize('alpha', [2, 3, 38])
def test_random_pairs(alpha):
	rng = random.Random(100 + alpha)
	for scores in SCORE_SETS:
		pairs = []
		for n in range(96):
			la = rng.randrange(0, 301)
			lb = la if n % 3 == 0 else rng.randrange(0, 301)  # la == lb a third of the time, la < lb and la > lb the rest
			a = seq(rng, la, alpha)
			pairs.append((a, (noisy_copy(rng, a, alpha) + seq(rng, lb, alpha))[:lb] if n % 2 else seq(rng, lb, alpha)))
		lt, eq, gt = (sum(c(len(a), len(b)) for a, b in pairs) for c in (int.__lt__, int.__eq__, int.__gt__))
		assert min(lt, eq, gt) >= 20
		check(pairs, scores)


def test_hand_computed_and_empty():
	got = run([([], []), ([1, 2], []), ([], [1, 2]), ([7, 1, 2, 9, 9], [1, 2]), ([1, 2], [7, 1, 2, 9, 9]), ([1, 1], [1])], A.CHAR_SCORES)
	assert got == [([], [], 0), ([0, 1], [-1, -1], 0), ([-1, -1], [0, 1], 0), ([0, 1, 2, 3, 4], [-1, 0, 1, -1, -1], 10),
	               ([-1, 0, 1, -1, -1], [0, 1, 2, 3, 4], 10), ([0, 1], [0, -1], 5)]
	assert run([([], [])], A.WORD_SCORES) == [([], [], 0)]  # La = Lb = 0


def test_chunk_and_register_tier_boundaries():
	"""64 columns a chunk; rows of 1, 2, 4, 8, 16 chunks in registers, longer ones in LDS (1,024 / 1,025)."""
	rng = random.Random(7)
	for scores in (A.CHAR_SCORES, (3, 1, -2, -5)):
		for lb in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1100):
			b = seq(rng, lb, 3)
			check([(noisy_copy(rng, b, 3), b), (seq(rng, 70, 3), b), (b, noisy_copy(rng, b, 3)), (b, seq(rng, 65, 3))], scores)


def test_long_pairs():
	rng = random.Random(8)
	a = seq(rng, 3000, 38)
	check([(a, (noisy_copy(rng, a, 38) + seq(rng, 200, 38))[:3100])], A.CHAR_SCORES)
	b = seq(rng, 16383, 3)
	check([(noisy_copy(rng, b[2000:2300], 3), b)], A.CHAR_SCORES)  # la < lb, the row in LDS at its largest
	check([(b, noisy_copy(rng, b[9000:9300], 3))], (3, 1, -2, -5))  # la >= lb, 16,383 rows


def test_unequal_lengths_in_one_launch():
	rng = random.Random(9)
	b = seq(rng, 2500, 38)
	pairs = [([], []), (seq(rng, 1, 38), b), (noisy_copy(rng, b, 38), b), (seq(rng, 5, 38), seq(rng, 3, 38)), (b[:1500], seq(rng, 2, 38)), ([], b[:77]), (b[:66], [])]
	check(pairs + [(seq(rng, rng.randrange(0, 50), 38), seq(rng, rng.randrange(0, 50), 38)) for _ in range(40)], A.CHAR_SCORES)


def test_split_over_the_workspace_cap():
	from convasr_amd import _lib, ops
	rng = random.Random(10)
	pairs = [(seq(rng, rng.randrange(0, 200), 3), seq(rng, rng.randrange(0, 200), 3)) for _ in range(150)] + [(seq(rng, 700, 3), seq(rng, 650, 3))]
	rng.shuffle(pairs)
	whole = check(pairs, A.CHAR_SCORES)
	launches, real = [], ops.call
	ops.call = lambda name, *args: (launches.append(name), real(name, *args))[1]
	try:
		cap = 400_000  # the largest pair alone needs 700 * 11 * 16 + 1,350 * 4 = 128,600 bytes
		assert check(pairs, A.CHAR_SCORES, workspace_cap = cap) == whole
	finally:
		ops.call = real
	assert 2 <= len(launches) < 20 and set(launches) == {'convasr_nw_align'}
	with pytest.raises(_lib.ConvasrHipError, match = 'nw_align'):
		run(pairs, A.CHAR_SCORES, workspace_cap = 100_000)


def test_two_runs_give_identical_bits():
	from convasr_amd import ops
	rng = random.Random(13)
	N, L = 64, 400
	a, b = torch.randint(0, 3, (N, L), dtype = torch.int32, device = DEV), torch.randint(0, 3, (N, L + 30), dtype = torch.int32, device = DEV)
	al, bl = torch.randint(0, L + 1, (N,), device = DEV), torch.randint(0, L + 31, (N,), device = DEV)
	first = ops.nw_align(a, al, b, bl, A.CHAR_SCORES)
	torch.empty(1 << 26, dtype = torch.uint8, device = DEV).fill_(0xA5)  # (dirty the allocator's blocks between the runs)
	second = ops.nw_align(a, al, b, bl, A.CHAR_SCORES)
	assert all(torch.equal(x, y) for x, y in zip(first, second))


def test_envelope_raises():
	from convasr_amd import _lib, ops
	a = torch.zeros(2, 5, dtype = torch.int32, device = DEV)
	n = torch.full((2,), 5, device = DEV)
	with pytest.raises(_lib.ConvasrHipError, match = 'nw_align'):
		ops.nw_align(a, n, a, n, (40000, 0, 0, 0))
	with pytest.raises(_lib.ConvasrHipError):
		ops.nw_align(a.cpu(), n, a, n, A.CHAR_SCORES)


def test_align_strings_reproduces_the_reference(golden):
	from convasr_amd import metrics
	cases = golden['cases']
	got = metrics.align_strings_batch([c['hyp'] for c in cases], [c['ref'] for c in cases])
	for c, g in zip(cases, got):
		assert list(g) == c['align_strings'], (c['hyp'], c['ref'])
	assert metrics.align_strings(hyp = 'б б', ref = 'б') == ('б б', 'б |')
	c = cases[-1]
	words = metrics.align_words(*metrics.align_strings(hyp = c['hyp'], ref = c['ref']), compute_cer = True)
	assert [(w['_hyp_'], w['_ref_'], w['cer']) for w in words] == [(w['_hyp_'], w['_ref_'], w['cer']) for w in words_of(golden, c['align_words'])]


def test_analyze_batch_reproduces_the_reference(golden):
	analyzer = make_analyzer(golden, aligner = None, scorer = None)
	cases = golden['cases']
	results = analyzer.analyze_batch([c['hyp'] for c in cases], [c['ref'] for c in cases], detailed = True, extra = [dict(n = n) for n in range(len(cases))])
	check_analysis(golden, results, analyzer.aggregate(results))
	assert analyzer.analyze(cases[40]['hyp'], cases[40]['ref'], detailed = True, extra = dict(n = 40)) == results[40]


def test_launch_count_does_not_depend_on_the_batch_size(golden):
	from convasr_amd import metrics, ops
	noisy = [c for c in golden['cases'] if c['hyp'] != c['ref'] and c['hyp'] and c['ref']][:64]
	assert len(noisy) == 64
	analyzer = make_analyzer(golden, aligner = None, scorer = None)
	counts, real = {}, ops.call

	def counted(fn, cases):
		launches = []
		ops.call = lambda name, *args: (launches.append(name), real(name, *args))[1]
		try:
			fn([c['hyp'] for c in cases], [c['ref'] for c in cases])
		finally:
			ops.call = real
		return launches

	for fn in (metrics.align_strings_batch, lambda h, r: analyzer.analyze_batch(h, r, detailed = True)):
		small, large = counted(fn, noisy[:2]), counted(fn, noisy)
		assert small == large and small.count('convasr_nw_align') == 2, (small, large)


def tiny_model_and_batches(**model_kwargs):
	import convasr_amd as ca
	from convasr_amd.transcript_generators import CharTokenizerLegacy
	torch.manual_seed(4)
	tok = CharTokenizerLegacy('абвгдеёжзийклмнопрстуфхцчшщъыьэюя')
	fe = ca.models.LogFilterBankFrontend(64, 16000, 0.02, 0.01, 'hann_window')
	model = ca.models.JasperNet(64, [tok.vocab_size], base_width = 32, kernel_sizes = [11], out_width_factors = [2], dropouts = [0.0], out_width_factors_large = [2, 2], residual = False, repeat = 1, frontend = fe, check_time_dim_padded = False, nonlinearity = ('hardtanh', 0, 20), dilation = 2, **model_kwargs).to(DEV)
	batches = []
	for seed in (1, 2):
		g = torch.Generator().manual_seed(seed)
		B, T, S = 4, 24000, 24
		x = torch.rand(B, T, generator = g) * 2 - 1
		y = torch.randint(0, tok.vocab_size - 1, (B, 1, S), generator = g)
		y[:, :, 5::6] = tok.space_id
		ylen = torch.tensor([[24], [20], [11], [17]])
		batches.append((None, None, x.to(DEV), torch.tensor([1.0, 0.9, 0.5, 0.75], device = DEV), y.to(DEV), ylen.to(DEV)))
	return model, tok, batches


def same(a, b):
	if torch.is_tensor(a):
		return torch.is_tensor(b) and torch.equal(a, b)
	if isinstance(a, dict):
		return isinstance(b, dict) and set(a) == set(b) and all(same(a[k], b[k]) for k in a)
	return a == b


def test_evaluate_model_with_an_error_analyzer(golden):
	from convasr_amd import train
	model, tok, batches = tiny_model_and_batches()
	analyzer = make_analyzer(golden, aligner = None, scorer = None)
	plain = train.evaluate_model(model, batches, tok, return_text = True)
	assert set(plain) == {'loss', 'entropy', 'cer', 'wer', 'utterances', 'hyp'} and set(plain['utterances']) == {'loss', 'entropy', 'uncertainty', 'cer', 'wer'}
	res = train.evaluate_model(model, batches, tok, return_text = True, error_analyzer = analyzer)
	assert set(res) == set(plain) | {'analysis', 'ref'} and len(res['ref']) == len(res['hyp']) == 8
	assert same({k: v for k, v in res.items() if k not in ('analysis', 'ref', 'utterances')}, {k: v for k, v in plain.items() if k != 'utterances'})
	assert same({k: v for k, v in res['utterances'].items() if k != 'analysis'}, plain['utterances'])
	want = analyzer.analyze_batch(res['hyp'], res['ref'], detailed = True)
	assert res['utterances']['analysis'] == want and res['analysis'] == analyzer.aggregate(want)
	assert [a['cer'] for a in want] == res['utterances']['cer'].tolist()  # the string path and the token path agree for this tokenizer
	assert 'mer_wordwise' in res['analysis'] and 'no_stop__cer_pseudo' in res['analysis'] and 'hyp_vocabness' in res['analysis']
	assert same(train.evaluate_model(model, batches, tok), {k: v for k, v in plain.items() if k != 'hyp'})


def test_transcribe_batch_with_align_words():
	from convasr_amd import metrics, transcribe
	model, tok, batches = tiny_model_and_batches(dict = lambda logits, log_probs, olen, **kwargs: (log_probs[0], logits[0], olen[0]))
	_, _, x, xlen, y, ylen = batches[0]
	model.eval()
	args = types.SimpleNamespace(device = DEV, sample_rate = 16000, align_words = True)
	pipeline = transcribe.TextPipeline(tok)
	B = x.shape[0]
	call = lambda: transcribe.transcribe_batch(args, pipeline, model, transcribe.GreedyCTCGenerator(), x, xlen, torch.zeros(B), torch.full((B,), 1.5), y = y, ylen = ylen)
	with torch.no_grad():
		out = call()
		args.align_words = False
		off = call()
	assert off.words is None and off.ref is None and off.hyp == out.hyp
	assert out.ref == [tok.decode([row[:n]])[0].strip() for row, n in zip(y[:, 0].tolist(), ylen[:, 0].tolist())]
	for hyp, ref, words in zip(out.hyp, out.ref, out.words):
		assert words == metrics.align_words(*metrics.align_strings(hyp = hyp, ref = ref, aligner = ref_aligner))
		assert [w['ref'] for w in words if w['ref']] == ref.split()
