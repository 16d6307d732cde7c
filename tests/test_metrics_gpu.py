"""Validation metrics on the MI355X: ops.edit_distance and ops.ctc_greedy_collapse against the Python restatement (tests/_metrics_ref.py),
metrics.cer / wer / cer_wer against the reference's string semantics, the token path against the string path, train.evaluate_model against
the host path it replaces, its lack of side effects on training, and graph capture of both kernels."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _metrics_ref as R  # noqa: E402

ALPHABET = 'абвгдеёжзийклмнопрстуфхцчшщъыьэюя'


def _dev():
	return torch.device('cuda:0')


def _tokenizer():
	from convasr_amd.transcript_generators import CharTokenizerLegacy
	return CharTokenizerLegacy(ALPHABET)


def _pad(seqs):
	L = max([len(s) for s in seqs] + [1])
	out = torch.zeros(len(seqs), L, dtype = torch.int64)
	for i, s in enumerate(seqs):
		out[i, :len(s)] = torch.tensor(s, dtype = torch.int64)
	return out, torch.tensor([len(s) for s in seqs], dtype = torch.int64)


def _random_seq(rng, alpha, n, space, p_space):
	"""n tokens over `alpha` symbols; with space = 0 the space is token 0 (drawn with p_space) and the others are 1 .. alpha - 1."""
	if space < 0:
		return [rng.randrange(alpha) for _ in range(n)]
	return [space if rng.random() < p_space else rng.randrange(1, alpha) for _ in range(n)]


def _special_pairs(space):
	s = max(space, 0)
	return [([], []), ([], [1, 2, 3]), ([4, 5], []), ([1, 2, 3, 4], [1, 2, 3, 4]), ([s] * 7, [1, s, 2]), ([s] * 5, [s] * 3),
	        ([s, s, 1, 2, s, s, 3, s, s], [1, 2, s, 3]), ([s, 1, s], [s, s, 1, 1, s, s]), ([1, 2, 3, s, 4, 5, 6], [1, 2, 4, s, 4, 5, 6])]


def _word_seq(rng, vocab, n_words, space):
	"""Words drawn from vocab, separated by runs of spaces, with spaces at both ends; sometimes cut inside the last word."""
	out = [space] * rng.randrange(0, 3)
	for _ in range(n_words):
		out += list(rng.choice(vocab)) + [space] * rng.randrange(1, 3)
	return out[:rng.randrange(len(out) - 2, len(out) + 1)] if len(out) > 2 else out


@pytest.mark.gpu
def test_edit_distance_against_the_restatement():
	"""2,400 pairs per mode and space: alphabets of 2 and 38 symbols, lengths 0-400, the special cases, K = 4 hypotheses per reference,
	references read in place from a (B, 2, Lpad) target batch; WORDS mode also over a vocabulary of words that differ only in their last
	token or have equal lengths."""
	from convasr_amd import ops, _lib
	rng = random.Random(11)
	K, d = 4, _dev()
	vocab = [(1, 2, 3), (1, 2, 4), (1, 2, 5), (6, 7), (7, 6), (8, ), (9, ), (1, 2, 3, 4), (2, 2, 2), (10, 11, 12)]
	checked = 0
	for mode, space in ((_lib.METRIC_CHARS, -1), (_lib.METRIC_CHARS, 0), (_lib.METRIC_WORDS, 0)):
		special = _special_pairs(space)
		refs, hyps = [], []
		for b in range(600):
			if b < len(special):
				h, r = special[b]
				refs.append(r)
				hyps.append([h, r, list(reversed(h)), h + r])
			elif b % 3 == 2 and mode == _lib.METRIC_WORDS:
				refs.append(_word_seq(rng, vocab, rng.randrange(0, 40), space))
				hyps.append([_word_seq(rng, vocab, rng.randrange(0, 40), space) for _ in range(K)])
			else:
				alpha = 2 if b % 3 == 0 else 38
				n = rng.randrange(0, 401) if rng.random() < 0.3 else rng.randrange(0, 120)
				refs.append(_random_seq(rng, alpha, n, space, 0.25))
				hyps.append([_random_seq(rng, alpha, max(0, n + rng.randrange(-30, 30)), space, 0.25) for _ in range(K)])
		B = len(refs)
		Lh = max(len(h) for hs in hyps for h in hs)
		hyp = torch.full((B, K, Lh), 3, dtype = torch.int64)  # 3 past the lengths: never read
		hlen = torch.zeros(B, K, dtype = torch.int64)
		for b, hs in enumerate(hyps):
			for k, h in enumerate(hs):
				hyp[b, k, :len(h)] = torch.tensor(h, dtype = torch.int64)
				hlen[b, k] = len(h)
		r0, rl = _pad(refs)
		y = torch.full((B, 2, r0.shape[1] + 5), 3, dtype = torch.int64)
		y[:, 0, :r0.shape[1]] = r0
		ylen = torch.stack([rl, torch.zeros_like(rl)], dim = 1)
		y, ylen = y.to(d), ylen.to(d)
		dist, units = ops.edit_distance(hyp.to(d), hlen.to(d), y[:, 0], ylen[:, 0], mode, space)
		dist, units = dist.cpu().tolist(), units.cpu().tolist()
		for b in range(B):
			for k in range(K):
				want = R.edit_distance(hyps[b][k], refs[b], mode, space)
				assert (dist[b][k], units[b]) == want, (mode, space, b, k, hyps[b][k], refs[b])
				checked += 1
	assert checked >= 2 * 2000


@pytest.mark.gpu
def test_edit_distance_at_the_length_limit():
	from convasr_amd import ops, _lib
	rng = np.random.default_rng(3)
	L, d = _lib.METRIC_MAX_LEN, _dev()
	long_a, long_b, short = rng.integers(0, 38, L).tolist(), rng.integers(0, 38, L).tolist(), rng.integers(0, 38, 50).tolist()
	long_w = rng.integers(0, 4, L).tolist()
	cases = [(long_a, short, 0, -1), (short, long_a, 0, -1), (long_a, long_b, 0, -1), (long_w, short, 1, 0), (short, long_w, 1, 0), (long_w, long_w, 1, 0)]
	for h, r, mode, space in cases:
		hyp, hl = _pad([h])
		ref, rl = _pad([r])
		dist, units = ops.edit_distance(hyp.to(d), hl.to(d), ref.to(d), rl.to(d), mode, space)
		assert (int(dist[0]), int(units[0])) == R.edit_distance(h, r, mode, space), (len(h), len(r), mode)
	# hypotheses around the register-resident DP's limit (1,024 units) and past it, K = 5 against one reference of 300 tokens
	lens = [700, 1000, 1024, 1025, 2100]
	hs = [rng.integers(0, 38, n).tolist() for n in lens]
	r = rng.integers(0, 38, 300).tolist()
	hyp = torch.zeros(1, len(lens), max(lens), dtype = torch.int64)
	for k, h in enumerate(hs):
		hyp[0, k, :len(h)] = torch.tensor(h)
	ref, rl = _pad([r])
	for mode, space in ((0, -1), (0, 5), (1, 5)):
		dist, _ = ops.edit_distance(hyp.to(d), torch.tensor([lens]).to(d), ref.to(d), rl.to(d), mode, space)
		assert dist[0].tolist() == [R.edit_distance(h, r, mode, space)[0] for h in hs], (mode, space)
	with pytest.raises(_lib.ConvasrHipError):
		ops.edit_distance(torch.zeros(1, L + 1, dtype = torch.int64, device = d), torch.tensor([L + 1], device = d), ref.to(d), rl.to(d))


@pytest.mark.gpu
def test_string_metrics_equal_the_reference_semantics():
	from convasr_amd import metrics
	pairs = [('привет мир', 'привет мир'), ('Привет Мир', 'привет мир'), ('ПРИВЕТ', 'привет  мир'), ('İstanbul', 'istanbul'), ('i̇x', 'İx'),
	         ('a\tb\nc', 'a b c'), ('a\tb', 'a\tb '), ('', ''), ('', 'один два'), ('один два', ''), ('   ', ' '), ('kitten', 'sitting'),
	         ('the cat  sat', ' the cat sat down '), ('Ёлка ёлка', 'ёлка Ёлка'), ('x', 'İ'), ('слово\n\nслово', 'слово слово')]
	rng = random.Random(2)
	chars = ALPHABET + ALPHABET.upper() + ' \t\nİ.'
	pairs += [(''.join(rng.choice(chars) for _ in range(rng.randrange(0, 60))), ''.join(rng.choice(chars) for _ in range(rng.randrange(0, 60)))) for _ in range(200)]
	c, w = metrics.cer_wer([p[0] for p in pairs], [p[1] for p in pairs], device = _dev())
	for (h, r), ci, wi in zip(pairs, c, w):
		assert type(ci) is float and type(wi) is float
		assert ci == R.cer(h, r) and wi == R.wer(h, r), (h, r, ci, wi)
	for h, r in pairs[:16]:
		assert metrics.cer(hyp = h, ref = r) == R.cer(h, r) and metrics.wer(hyp = h, ref = r) == R.wer(h, r)
	assert metrics.cer_wer([], []) == ([], [])


@pytest.mark.gpu
def test_token_path_equals_string_path_on_decoded_tokens():
	from convasr_amd import metrics
	tok, d = _tokenizer(), _dev()
	g = torch.Generator().manual_seed(4)
	B, K, L = 64, 3, 90
	hyp = torch.randint(0, tok.vocab_size, (B, K, L), generator = g)
	hyp[torch.rand(B, K, L, generator = g) < 0.25] = tok.space_id
	hlen = torch.randint(0, L + 1, (B, K), generator = g)
	ref = hyp[:, 0].clone()
	ref[torch.rand(B, L, generator = g) < 0.2] = tok.space_id
	ref[:8] = hyp[:8, 1]
	rlen = torch.randint(0, L + 1, (B, ), generator = g)
	rlen[:8] = hlen[:8, 1]
	c, w = metrics.token_cer_wer(hyp.to(d), hlen.to(d), ref.to(d), rlen.to(d), tok.space_id)
	assert c.dtype == w.dtype == torch.float64 and c.shape == (B, K) and c.is_cuda
	c, w = c.cpu().tolist(), w.cpu().tolist()
	for b in range(B):
		rs = tok.decode([ref[b, :rlen[b]].tolist()])[0]
		for k in range(K):
			hs = tok.decode([hyp[b, k, :hlen[b, k]].tolist()])[0]
			assert c[b][k] == R.cer(hs, rs) and w[b][k] == R.wer(hs, rs), (b, k)
	c1, _ = metrics.token_cer_wer(hyp[:, 0].to(d), hlen[:, 0].to(d), ref.to(d), rlen.to(d), tok.space_id)
	assert c1.shape == (B, ) and c1.cpu().tolist() == [row[0] for row in c]


def _greedy_paths(B, T, C, eps, space, seed):
	"""Argmax paths biased towards the blank, the space and repeats."""
	g = torch.Generator().manual_seed(seed)
	path = torch.randint(0, C, (B, T), generator = g)
	pick = torch.rand(B, T, generator = g)
	path[pick < 0.45] = eps
	path[(pick >= 0.45) & (pick < 0.6)] = space
	rep = torch.rand(B, T, generator = g) > 0.8
	for t in range(1, T):
		path[:, t] = torch.where(rep[:, t], path[:, t - 1], path[:, t])
	path[0] = eps
	if B > 1:
		path[1] = space
	return path


@pytest.mark.gpu
def test_greedy_collapse_equals_the_host_generator():
	from convasr_amd import ops, transcribe
	from convasr_amd.transcript_generators import GreedyCTCGenerator
	tok, d = _tokenizer(), _dev()
	C, eps, space = tok.vocab_size, tok.eps_id, tok.space_id
	for B, T, seed in ((24, 300, 1), (6, 3000, 2), (1, 1, 3), (3, 1, 4)):
		path = _greedy_paths(B, T, C, eps, space, seed)
		lengths = torch.randint(0, T + 1, (B, ), generator = torch.Generator().manual_seed(seed))
		lengths[-1] = T
		lp = torch.nn.functional.one_hot(path, C).permute(0, 2, 1).float().to(d)  # argmax = path
		for bats in (1, 3, 10):
			tokens, n = ops.ctc_greedy_collapse(ops.argmax(lp), lengths.to(d), eps, space, bats)
			tokens, n = tokens.cpu(), n.cpu()
			host = GreedyCTCGenerator(bats).generate(tok, lp, torch.zeros(B), torch.ones(B), output_lengths = lengths.to(d))
			for b in range(B):
				want = R.greedy_collapse(path[b].tolist(), int(lengths[b]), eps, space, bats)
				assert tokens[b, :n[b]].tolist() == want, (T, bats, b)
				assert bool((tokens[b, n[b]:] == 0).all())
				text = host[b][0][0]['hyp'] if len(host[b][0]) else ''
				assert tok.decode([want])[0] == text and transcribe.join(hyp = host[b][0]) == text.strip()


def _tiny_model(dropout, seed = 1):
	import convasr_amd as ca
	torch.manual_seed(seed)
	fe = ca.models.LogFilterBankFrontend(64, 16000, 0.02, 0.01, 'hann_window')
	return ca.models.Wav2Letter(64, [38], frontend = fe, dropout = dropout, check_time_dim_padded = False).to(_dev())


def _batches(n = 3, B = 4, secs = 2, seed = 5):
	g = torch.Generator().manual_seed(seed)
	d, out = _dev(), []
	for i in range(n):
		x = torch.rand(B, 16000 * secs, generator = g) * 2 - 1
		xlen = torch.linspace(0.5, 1, B)
		y = torch.randint(0, 37, (B, 2, 10 * secs + i), generator = g)
		ylen = torch.randint(5, 10 * secs + 1, (B, 2), generator = g)
		out.append(([{}] * B, None, x.to(d), xlen.to(d), y.to(d), ylen.to(d)))
	return out


def _train(model, steps, batches, first = 0):
	import convasr_amd as ca
	opt = getattr(model, '_test_opt', None)
	if opt is None:
		opt = model._test_opt = ca.train.SGD(ca.train.FlatParameters(model), lr = 1e-3, momentum = 0.9, weight_decay = 1e-3)
	model.train()
	for i in range(first, first + steps):
		_, _, x, xlen, y, ylen = batches[i % len(batches)]
		ca.train.train_step(model, opt, x, xlen, y, ylen, iteration = i)


@pytest.mark.gpu
def test_evaluate_model_equals_the_host_path():
	import convasr_amd as ca
	from convasr_amd import transcribe
	from convasr_amd.transcript_generators import GreedyCTCGenerator
	tok = _tokenizer()
	model = _tiny_model(0.0)
	batches = _batches()
	_train(model, 4, batches)  # a few steps, so that the hypotheses are not all alike
	res = ca.train.evaluate_model(model, batches, tok, return_text = True)
	assert model.training
	model.eval()
	want = dict(loss = [], entropy = [], uncertainty = [], cer = [], wer = [], hyp = [])
	with torch.no_grad():
		for _, _, x, xlen, y, ylen in batches:
			out = model(x, xlen, y = y, ylen = ylen)
			lp, olen = out['log_probs'][0], out['olen'][0]
			want['loss'] += out['loss'].cpu().tolist()
			want['entropy'] += ca.models.entropy(lp, olen).cpu().tolist()
			want['uncertainty'] += ca.models.weighted_mean_entropy(lp, olen).cpu().tolist()
			gen = GreedyCTCGenerator().generate(tok, lp, torch.zeros(len(x)), torch.zeros(len(x)), output_lengths = olen)
			for b, alts in enumerate(gen):
				h = transcribe.join(hyp = alts[0])
				r = tok.decode([y[b, 0, :ylen[b, 0]].tolist()])[0]
				want['hyp'].append(h)
				want['cer'].append(R.cer(h, r))
				want['wer'].append(R.wer(h, r))
	utt = res['utterances']
	for k in ('loss', 'entropy', 'uncertainty'):
		assert utt[k].dtype == torch.float32 and utt[k].tolist() == want[k], k
	for k in ('cer', 'wer'):
		assert utt[k].dtype == torch.float64 and utt[k].tolist() == want[k], k
		assert res[k] == sum(want[k]) / len(want[k])  # metrics.nanmean: a sum of Python floats in order
	assert res['hyp'] == want['hyp']
	assert res['loss'] == sum(want['loss']) / len(want['loss']) and 'cer_oracle' not in res

	# the beam search's top 4: the first scored as above, the oracle the minimum over the four
	dec = ca.decoders.BeamSearchDecoder(tok, beam_width = 16, topk = 4)
	res = ca.train.evaluate_model(model, batches, tok, decoder = dec)
	model.eval()
	cer, wer, oc, ow = [], [], [], []
	with torch.no_grad():
		for _, _, x, xlen, y, ylen in batches:
			out = model(x, xlen, y = y, ylen = ylen)
			tokens, _, lengths, _ = dec.decode_with_scores(out['log_probs'][0], out['olen'][0])
			tokens, lengths = tokens.cpu(), lengths.cpu()
			for b in range(len(x)):
				r = tok.decode([y[b, 0, :ylen[b, 0]].tolist()])[0]
				hs = [tok.decode([tokens[b, k, :lengths[b, k]].tolist()])[0] for k in range(4)]
				cs, ws = [R.cer(h, r) for h in hs], [R.wer(h, r) for h in hs]
				cer.append(cs[0]); wer.append(ws[0]); oc.append(min(cs)); ow.append(min(ws))
	utt = res['utterances']
	assert utt['cer'].tolist() == cer and utt['wer'].tolist() == wer
	assert utt['cer_oracle'].tolist() == oc and utt['wer_oracle'].tolist() == ow
	assert res['cer_oracle'] <= res['cer'] and res['wer_oracle'] <= res['wer']


@pytest.mark.gpu
def test_evaluate_model_leaves_training_untouched():
	import convasr_amd as ca
	tok, batches = _tokenizer(), _batches()
	model = _tiny_model(0.2)
	ca.functional.manual_seed(21)
	_train(model, 1, batches)
	before = {k: v.detach().clone() for k, v in model.state_dict().items()}
	rng_cuda, rng_cpu = torch.cuda.get_rng_state(), torch.get_rng_state()
	drop = ca.functional._DropoutState
	offset, dev_state = drop.offset, {k: v['state'].clone() for k, v in drop.dev.items()}
	res = ca.train.evaluate_model(model, batches, tok)
	assert model.training and res['loss'] > 0
	for k, v in model.state_dict().items():
		assert torch.equal(v, before[k]), k
	assert torch.equal(torch.cuda.get_rng_state(), rng_cuda) and torch.equal(torch.get_rng_state(), rng_cpu)
	assert drop.offset == offset and all(torch.equal(v['state'], dev_state[k]) for k, v in drop.dev.items())
	model.eval()
	ca.train.evaluate_model(model, batches[:1], tok)
	assert not model.training

	# three steps, an evaluation, three more steps == six steps, dropout on: a change to the device-side step key or to the parameters, BN
	# statistics or momentum would show here (the host-side layer offset restarts at every step, so only the assertion above guards it)
	runs = []
	for with_eval in (True, False):
		m = _tiny_model(0.2, seed = 9)
		ca.functional.manual_seed(33)
		_train(m, 3, batches)
		if with_eval:
			ca.train.evaluate_model(m, batches, tok)
		_train(m, 3, batches, first = 3)
		runs.append({k: v.detach().clone() for k, v in m.state_dict().items()})
	for k in runs[0]:
		assert torch.equal(runs[0][k], runs[1][k]), k


@pytest.mark.gpu
def test_both_kernels_capture_into_one_graph():
	from convasr_amd import ops, _lib
	tok, d = _tokenizer(), _dev()
	B, T = 16, 500
	path = _greedy_paths(B, T, tok.vocab_size, tok.eps_id, tok.space_id, 7).to(d)
	lengths = torch.randint(0, T + 1, (B, ), generator = torch.Generator().manual_seed(7)).to(d)
	y = torch.randint(0, 38, (B, 2, 200), generator = torch.Generator().manual_seed(8)).to(d)
	ylen = torch.randint(0, 201, (B, 2), generator = torch.Generator().manual_seed(9)).to(d)

	def run():
		tokens, n = ops.ctc_greedy_collapse(path, lengths, tok.eps_id, tok.space_id, 3)
		c = ops.edit_distance(tokens, n, y[:, 0], ylen[:, 0], _lib.METRIC_CHARS, tok.space_id)
		w = ops.edit_distance(tokens, n, y[:, 0], ylen[:, 0], _lib.METRIC_WORDS, tok.space_id)
		return tokens, n, c[0], c[1], w[0], w[1]

	side = torch.cuda.Stream()
	side.wait_stream(torch.cuda.current_stream())
	with torch.cuda.stream(side):
		eager = [t.clone() for t in run()]
	torch.cuda.current_stream().wait_stream(side)
	graph = torch.cuda.CUDAGraph()
	with torch.cuda.graph(graph):
		static = run()
	graph.replay()
	torch.cuda.synchronize()
	for a, b in zip(eager, static):
		assert torch.equal(a, b)
	path[:, ::7] = tok.eps_id  # new inputs in place, then replayed again
	graph.replay()
	again = run()
	torch.cuda.synchronize()
	for a, b in zip(again, static):
		assert torch.equal(a, b)
