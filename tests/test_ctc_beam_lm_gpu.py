"""convasr_ctc_beam_search_lm on the MI355X against the float64 restatement (tests/_ctc_beam_lm_ref.py): tokens, offsets and lengths
exactly, the fused score to 1e-9 relative, on inputs whose decisions have a margin above GAP (as in test_ctc_beam_search_gpu.py).  Also
bitwise reruns, a graph-captured call, the LM-free entry point beside it, and the LM deciding a word through decoders.BeamSearchDecoder
and transcribe.setup(decoder = 'BeamSearchDecoder', lm = ...)."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ctc_beam_lm_ref as RL  # noqa: E402
import _ctc_beam_ref as R  # noqa: E402
import _lm_synth  # noqa: E402

gpu = pytest.mark.gpu
GAP = 1e-9
ROOT = os.path.dirname(os.path.abspath(__file__))
SMALL = os.path.join(ROOT, 'golden', 'lm_small.arpa')
ALPHA = 'абвгдеёжзийклмнопрстуфхцчшщъыьэюя'
RU_LABELS = ALPHA + '*.2 |'                 # CharTokenizerLegacy: space 36, blank '|' 37
LABELS_FRONT = '| ' + ALPHA + '*.2'         # blank 0, space 1
LABELS_MID = ALPHA[:5] + '|' + ALPHA[5:19] + ' ' + ALPHA[19:] + '*.2'  # blank 5, space 20


def _peaked(B, T, C, seed, sharp = 4.0):
	rng = np.random.default_rng(seed)
	x = rng.normal(size = (B, T, C))
	x[np.arange(B)[:, None], np.arange(T)[None, :], rng.integers(0, C, (B, T))] += sharp
	return (x - np.logaddexp.reduce(x, axis = -1, keepdims = True)).astype(np.float32)


def _lengths(B, T):
	return np.array([T, 0, 1, max(T // 2, 1), max(T - 7, 1), max(3 * T // 4, 1), min(17, T), T][:B], dtype = np.int64)


_models = {}


def _model(path, labels):
	from convasr_amd import lm
	key = (path, labels)
	if key not in _models:
		_models[key] = lm.NgramLM(path, labels)
	return _models[key]


def _gpu(lp_btc, lengths, M, alpha, beta, W, N, cutoff = 1.0, topk = 1, blank = None):
	from convasr_amd import ops
	blank = M.labels.index('|') if blank is None else blank
	x = torch.from_numpy(lp_btc).cuda().permute(0, 2, 1)
	out = ops.ctc_beam_search_lm(x, torch.from_numpy(lengths), blank, W, M, alpha, beta, N, cutoff, topk)
	torch.cuda.synchronize()
	return [o.cpu().numpy() for o in out]


def _case(B, T, M, alpha, beta, W, N, topk, cutoff = 1.0, seed0 = 0):
	"""The first seed whose restatement has a margin above GAP: (lp, lengths, reference outputs)."""
	C = M.num_classes
	blank = M.labels.index('|')
	ref_model = RL.Model(M.arpa, ''.join(M.labels), blank, alpha, beta)
	lengths = _lengths(B, T)
	for seed in range(seed0, seed0 + 6):
		lp = _peaked(B, T, C, 1000 * T + 10 * W + seed)
		ref = RL.decode(lp, lengths, ref_model, W, min(N, C), float(np.float32(cutoff)), topk)
		if ref[-1] > GAP:
			return lp, lengths, ref
	pytest.fail(f'no seed with a decision margin above {GAP} for T {T} W {W} N {N}')


def _compare(got, ref, what):
	tokens, offsets, out_len, logp = got
	rt, ro, rl, rp = ref[:4]
	assert logp.dtype == np.float64
	assert np.array_equal(out_len, rl), (what, out_len, rl)
	assert np.array_equal(tokens, rt), (what, np.argwhere(tokens != rt)[:5])
	assert np.array_equal(offsets, ro), (what, np.argwhere(offsets != ro)[:5])
	fin = np.isfinite(rp)
	assert np.array_equal(np.isfinite(logp), fin) and np.all(logp[~fin] == rp[~fin]), (what, logp, rp)
	err = np.abs(logp[fin] - rp[fin])
	assert np.all(err <= 1e-9 * np.maximum(np.abs(rp[fin]), 1.0)), (what, err.max())


@pytest.fixture(scope = 'module')
def orders(tmp_path_factory):
	d = tmp_path_factory.mktemp('lm')
	return {n: _lm_synth.write_small(str(d / f'o{n}.arpa'), n, seed = n) for n in (1, 2, 4, 6)}


@pytest.fixture(scope = 'module')
def big(tmp_path_factory):
	return _lm_synth.write(str(tmp_path_factory.mktemp('lm') / 'big.arpa'))


def _lm_max_w(C, N):
	from convasr_amd import _lib
	lib = _lib.load()
	return max(W for W in (1024, 768, 512, 256) if lib.convasr_ctc_beam_search_lm_workspace_bytes(1, 1, C, W, min(N, C), 1) > 0)


@gpu
def test_lm_search_matches_the_restatement(orders):
	WMAX = _lm_max_w(38, 40)
	assert WMAX == 1024
	cases = [  # (model, labels, alpha, beta, T, W, N, topk, cutoff)
		(SMALL, RU_LABELS, 0.8, 1.0, 1, 8, 40, 4, 1.0),
		(SMALL, RU_LABELS, 0.8, 1.0, 60, 1, 40, 1, 1.0),
		(SMALL, RU_LABELS, 0.5, -1.5, 60, 8, 40, 4, 1.0),
		(SMALL, RU_LABELS, 0.0, 2.0, 60, 64, 40, 4, 1.0),
		(SMALL, RU_LABELS, 1.0, 0.0, 60, 64, 10, 2, 1.0),
		(SMALL, RU_LABELS, 0.0, 0.0, 60, WMAX, 40, 4, 1.0),
		(SMALL, RU_LABELS, 0.4, 2.6, 750, 64, 40, 4, 1.0),
		(SMALL, RU_LABELS, 0.4, 2.6, 60, 64, 38, 4, 0.999),
		(SMALL, RU_LABELS, 0.7, 0.5, 200, 32, 40, 1, 0.99),
		(SMALL, RU_LABELS, 0.7, 0.5, 60, 16, 40, 2, 0.5),
		(orders[1], RU_LABELS, 0.6, 1.0, 60, 64, 40, 4, 1.0),
		(orders[2], LABELS_FRONT, 0.6, 1.0, 60, 64, 40, 4, 1.0),
		(orders[4], LABELS_MID, 0.6, -0.5, 60, 64, 40, 4, 1.0),
		(orders[6], RU_LABELS, 0.6, 1.0, 750, 8, 40, 2, 1.0),
		(orders[6], LABELS_MID, 1.5, 3.0, 60, WMAX, 40, 4, 1.0),
	]
	for path, labels, alpha, beta, T, W, N, topk, cutoff in cases:
		M = _model(path, labels)
		lp, lengths, ref = _case(8, T, M, alpha, beta, W, N, topk, cutoff)
		_compare(_gpu(lp, lengths, M, alpha, beta, W, min(N, 38), cutoff, topk), ref, (os.path.basename(path), labels[:3], alpha, beta, T, W, N, topk, cutoff))


@gpu
def test_lm_search_with_the_large_model(big):
	"""The order-4 model of 10^5 words generated in the test run: a dictionary that allows most extensions, and long contexts."""
	M = _model(big, RU_LABELS)
	for T, W, topk, alpha, beta in ((750, 64, 4, 0.4, 2.6), (60, 1024, 4, 0.8, 0.5), (60, 8, 1, 0.3, -1.0)):
		lp, lengths, ref = _case(4, T, M, alpha, beta, W, 40, topk)
		_compare(_gpu(lp, lengths, M, alpha, beta, W, 40, 1.0, topk), ref, ('big', T, W, topk))


@gpu
def test_reruns_graph_capture_and_the_lm_free_entry_point():
	from convasr_amd import ops
	M = _model(SMALL, RU_LABELS)
	lp, lengths, ref = _case(8, 200, M, 0.5, 1.0, 256, 40, 4)
	a = _gpu(lp, lengths, M, 0.5, 1.0, 256, 40, 1.0, 4)
	b = _gpu(lp, lengths, M, 0.5, 1.0, 256, 40, 1.0, 4)
	_compare(a, ref, 'rerun')
	for x, y in zip(a, b):
		assert x.tobytes() == y.tobytes()
	# graph capture: the tables are uploaded by the eager calls above; the call itself has no copy, memset or host synchronisation
	x = torch.from_numpy(lp).cuda().permute(0, 2, 1)
	lens = torch.from_numpy(lengths).cuda()
	s = torch.cuda.Stream()
	s.wait_stream(torch.cuda.current_stream())
	with torch.cuda.stream(s):
		ops.ctc_beam_search_lm(x, lens, 37, 256, M, 0.5, 1.0, 40, 1.0, 4)
	torch.cuda.current_stream().wait_stream(s)
	g = torch.cuda.CUDAGraph()
	with torch.cuda.graph(g):
		out = ops.ctc_beam_search_lm(x, lens, 37, 256, M, 0.5, 1.0, 40, 1.0, 4)
	for o in out:
		o.fill_(-7)
	g.replay()
	torch.cuda.synchronize()
	for o, e in zip(out, a):
		assert o.cpu().numpy().tobytes() == e.tobytes()
	# the LM-free entry point beside it: still the LM-free restatement
	lpf, lenf = _peaked(8, 60, 38, 4242), _lengths(8, 60)
	want = R.decode(lpf, lenf, 37, 64, 38, 1.0, 4)
	assert want[-1] > GAP
	got = ops.ctc_beam_search(torch.from_numpy(lpf).cuda().permute(0, 2, 1), torch.from_numpy(lenf), 37, 64, 40, 1.0, 4)
	got = [o.cpu().numpy() for o in got]
	assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
	assert got[3].dtype == np.float32 and np.allclose(got[3], want[3], rtol = 1e-5, atol = 1e-3)


def _spell(frames, C, seed = 0):
	"""(1, C, T) log-probs: each frame a dict class -> probability, the rest spread over the other classes."""
	rng = np.random.default_rng(seed)
	out = np.empty((len(frames), C))
	for t, f in enumerate(frames):
		rest = 1.0 - sum(f.values())
		p = rng.uniform(0.5, 1.5, size = C)
		p[list(f)] = 0
		p *= rest / p.sum()
		for c, v in f.items():
			p[c] = v
		out[t] = np.log(p)
	return np.ascontiguousarray(out.T[None].astype(np.float32))


def _word_case(tok):
	"""Frames spelling 'он ко?' where ? is л (the acoustically best, 'кол' is no word), д ('код', a word of weak bigram after 'он') or т
	('кот', a word of strong bigram): the LM must pick 'он кот', the LM-free search 'он кол'."""
	c = tok.char2idx
	blank, space = tok.eps_id, tok.space_id
	frames = []
	for ch in 'он':
		frames += [{c[ch]: 0.9}] * 2 + [{blank: 0.9}]
	frames += [{space: 0.9}] * 2 + [{blank: 0.9}]
	for ch in 'ко':
		frames += [{c[ch]: 0.9}] * 2 + [{blank: 0.9}]
	frames += [{c['л']: 0.42, c['д']: 0.30, c['т']: 0.26}] * 2 + [{blank: 0.9}] * 2
	return _spell(frames, tok.vocab_size)


@gpu
def test_the_language_model_decides_the_word():
	"""The test that fails without LM fusion: the acoustically best labelling is not a word, a close one is the word of a strong bigram."""
	from convasr_amd import decoders
	from convasr_amd.transcript_generators import CharTokenizerLegacy
	tok = CharTokenizerLegacy(ALPHA)
	lp = _word_case(tok)
	x = torch.from_numpy(lp).cuda()
	free = decoders.BeamSearchDecoder(tok, beam_width = 16).decode(x)
	fused = decoders.BeamSearchDecoder(tok, lm_path = SMALL, beam_width = 16, beam_alpha = 0.8, beam_beta = 0.0).decode(x)
	assert tok.decode(free)[0] == 'он кол'
	assert tok.decode(fused)[0] == 'он кот'
	M = RL.Model(_model(SMALL, RU_LABELS).arpa, RU_LABELS, 37, 0.8, 0.0)
	ref = RL.decode(np.ascontiguousarray(lp.transpose(0, 2, 1)), [lp.shape[2]], M, 16, 38, 1.0, 1)
	assert ref[0][0, 0, :ref[2][0, 0]].tolist() == fused[0] and ref[-1] > GAP


def _fixture():
	g = np.load(os.path.join(ROOT, 'golden', 'transcribe.npz'))
	j = json.load(open(os.path.join(ROOT, 'golden', 'transcribe.json')))
	return g, j


@gpu
def test_transcribe_setup_with_a_language_model():
	"""args.decoder = 'BeamSearchDecoder', args.lm = the ARPA fixture, args.beam_alpha / beam_beta: the generator decides 'он кот' on the
	word case, and on the transcribe fixture's audio every emitted word is a word of the vocabulary and the top beam is the restatement's."""
	import convasr_amd as ca
	from convasr_amd.transcript_generators import BeamCTCGenerator
	g, j = _fixture()
	T_ = lambda a: torch.as_tensor(np.asarray(a))
	sd = {k[3:]: T_(g[k]) for k in g.files if k.startswith('sd/')}
	ckpt_args = dict(j['args'], alphabet = j['alphabet'], model_kwargs = dict(base_width = 32, kernel_sizes = [11], out_width_factors = [2], dropouts = [0.2], out_width_factors_large = [2, 2], residual = False, repeat = 1, nonlinearity = ('hardtanh', 0, 20), dilation = 2))
	args = types.SimpleNamespace(checkpoint = dict(args = dict(ckpt_args), model_state_dict = {k: v.clone() for k, v in sd.items()}), device = 'cuda:0', fp16 = None, frontend_in_model = True,
	                             model = None, align = False, decoder = 'BeamSearchDecoder', beam_width = 32, decoder_topk = 1, lm = SMALL, beam_alpha = 0.8, beam_beta = 0.0)
	try:
		text_pipeline, frontend, model, generator = ca.transcribe.setup(args)
		assert isinstance(generator, BeamCTCGenerator)
		tok = text_pipeline.tokenizer
		word = generator.generate(tokenizer = tok, log_probs = torch.from_numpy(_word_case(tok)).cuda(), begin = torch.zeros(1), end = torch.ones(1))
		assert ''.join(s['hyp'] for s in word[0][0]) == 'он кот'
		args.beam_alpha, args.beam_beta = 0.4, 2.6
		text_pipeline, frontend, model, generator = ca.transcribe.setup(args)
		res = ca.transcribe.transcribe_batch(args, text_pipeline, model, generator, T_(g['wav']).unsqueeze(1), T_(g['xlen']), T_(g['begin']), T_(g['end']), segment_extra_info = j['extra'])
	finally:
		torch.set_grad_enabled(True)
	lmodel = _model(SMALL, RU_LABELS)
	V = set(lmodel.vocabulary_of(tok.eps_id))
	M = RL.Model(lmodel.arpa, ''.join(tok.vocab), tok.eps_id, 0.4, 2.6)
	lp_btc = res.log_probs.permute(0, 2, 1).contiguous().cpu().numpy()
	ref = RL.decode(lp_btc, res.olen.cpu().numpy(), M, 32, min(40, lp_btc.shape[2]), 1.0, 1)
	assert ref[-1] > GAP
	for b, hyp in enumerate(res.hyp):
		toks = ref[0][b, 0, :ref[2][b, 0]].tolist()
		assert hyp == ' '.join(tok.decode([toks])[0].split()), (hyp, tok.decode([toks])[0])
		assert hyp and all(w in V for w in hyp.split()), hyp
