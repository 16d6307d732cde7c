"""convasr_ctc_beam_search_hot / _lm_hot and their wide forms on the MI355X against the float64 restatement (tests/_ctc_beam_hot_ref.py):
tokens, offsets and lengths exactly, the ranking score to 1e-9 relative, on the inputs of tests/_hot_inputs.py (whose coverage of the rule
test_ctc_beam_hot_ref.py asserts on the CPU).  Also the identity with the four existing entry points at weight 0 and with an empty list,
the list deciding a word through decoders.BeamSearchDecoder and transcribe.setup, bitwise reruns, a graph-captured call and the refusals."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ctc_beam_hot_ref as RH  # noqa: E402
import _hot_inputs as I  # noqa: E402
from test_ctc_beam_lm_gpu import _compare, _fixture, _model, _peaked, _spell  # noqa: E402

gpu = pytest.mark.gpu


def _hot(phrases, labels):
	from convasr_amd import hotwords
	return hotwords.HotWords(phrases, labels)


def _run(lp_btc, lengths, blank, W, hw, weight, lm = None, N = 40, cutoff = 1.0, topk = 1, wide = None):
	from convasr_amd import ops
	x = torch.from_numpy(lp_btc).cuda().permute(0, 2, 1)
	out = ops.ctc_beam_search_hot(x, torch.from_numpy(lengths), blank, W, hw, weight, lm, I.LM_ALPHA, I.LM_BETA, N, cutoff, topk, wide = wide)
	torch.cuda.synchronize()
	return [o.cpu().numpy() for o in out]


def _max_w(name, C, N):
	from convasr_amd import _lib
	lib = _lib.load()
	return max(W for W in (1024, 768, 512, 256) if getattr(lib, f'convasr_{name}_workspace_bytes')(1, 1, C, W, min(N, C), 1) > 0)


@gpu
def test_the_largest_lds_width_at_38_classes():
	assert _max_w('ctc_beam_search_hot', 38, 40) == I.WMAX and _max_w('ctc_beam_search_lm_hot', 38, 40) == I.WMAX


@gpu
@pytest.mark.parametrize('row', range(len(I.CASES)))
@pytest.mark.parametrize('form', ['free', 'lm'])
def test_hot_search_matches_the_restatement(form, row):
	labels, weight, B, T, W, N, topk, cutoff = I.CASES[row]
	M = _model(I.SMALL, labels)
	lp, lengths, ref = I.form_case(form, M.arpa, *I.CASES[row])
	hw = _hot(I.FREE_PHRASES if form == 'free' else I.LM_PHRASES, labels)
	got = _run(lp, lengths, labels.index('|'), W, hw, weight, M if form == 'lm' else None, min(N, 38), cutoff, topk)
	_compare(got, ref, (form, I.CASES[row]))
	if W <= I.WMAX and T == 60 and W in (8, 64):  # both kernels take it: byte-equal
		for wide in (True, False):
			again = _run(lp, lengths, labels.index('|'), W, hw, weight, M if form == 'lm' else None, min(N, 38), cutoff, topk, wide = wide)
			for x, y in zip(got, again):
				assert x.tobytes() == y.tobytes(), (form, row, wide)


@gpu
def test_weight_zero_and_an_empty_list_are_the_existing_searches():
	from convasr_amd import ops
	M = _model(I.SMALL, I.RU_LABELS)
	B, T, W, topk = 8, 60, 64, 4
	lp, lengths = _peaked(B, T, 38, 4242), I.lengths_of(B, T)
	x, lens = torch.from_numpy(lp).cuda().permute(0, 2, 1), torch.from_numpy(lengths)
	for wide in (False, True):
		free = [o.cpu().numpy() for o in ops.ctc_beam_search(x, lens, 37, W, 40, 1.0, topk, wide = wide)]
		fused = [o.cpu().numpy() for o in ops.ctc_beam_search_lm(x, lens, 37, W, M, I.LM_ALPHA, I.LM_BETA, 40, 1.0, topk, wide = wide)]
		for hw, weight in ((_hot(I.LM_PHRASES, I.RU_LABELS), 0.0), (_hot([], I.RU_LABELS), 3.0), (_hot([], I.RU_LABELS), 0.0)):
			got = _run(lp, lengths, 37, W, hw, weight, None, 40, 1.0, topk, wide = wide)
			for a, b in zip(got[:3], free[:3]):
				assert a.tobytes() == b.tobytes()
			assert got[3].dtype == np.float64 and free[3].dtype == np.float32
			fin = np.isfinite(free[3])
			assert np.array_equal(np.isfinite(got[3]), fin)
			assert np.all(np.abs(got[3][fin].astype(np.float32) - free[3][fin]) <= np.spacing(np.abs(free[3][fin])))  # (one fp32 rounding)
			got = _run(lp, lengths, 37, W, hw, weight, M, 40, 1.0, topk, wide = wide)
			for a, b in zip(got, fused):
				assert a.tobytes() == b.tobytes()


def _word_case(tok):
	"""Frames spelling 'он ко?' with ? = л (the acoustically best), д or т, as test_ctc_beam_lm_gpu._word_case: the hot-less search says
	'он кол', which differs from the hot phrase 'он кот' in one letter."""
	c = tok.char2idx
	blank, space = tok.eps_id, tok.space_id
	frames = []
	for ch in 'он':
		frames += [{c[ch]: 0.9}] * 2 + [{blank: 0.9}]
	frames += [{space: 0.9}] * 2 + [{blank: 0.9}]
	for ch in 'ко':
		frames += [{c[ch]: 0.9}] * 2 + [{blank: 0.9}]
	# one undecided frame, not two as there: over two, 'он котл' (т then л) would be likelier than 'он кот' and keep the completed phrase's bonus
	frames += [{c['л']: 0.42, c['д']: 0.30, c['т']: 0.26}] + [{blank: 0.9}] * 2
	return _spell(frames, tok.vocab_size)


@gpu
def test_the_list_decides_the_word():
	"""The test that fails without the hot rule: 'кол' beats 'кот' acoustically by about 2 ln(0.42 / 0.26) < 1, and a listed 'он кот' gains
	6 labels x 0.5.  With weight 0, or without the list, the transcript stays 'он кол'."""
	from convasr_amd import decoders
	from convasr_amd.transcript_generators import CharTokenizerLegacy
	tok = CharTokenizerLegacy(I.ALPHA)
	x = torch.from_numpy(_word_case(tok)).cuda()
	say = lambda **kw: tok.decode(decoders.BeamSearchDecoder(tok, beam_width = 16, **kw).decode(x))[0]
	assert say() == 'он кол'
	assert say(hotwords = ['Он  кот'], hotword_weight = 0.0) == 'он кол'
	assert say(hotwords = ['он кот'], hotword_weight = 0.5) == 'он кот'
	assert say(hotwords = ['кот'], hotword_weight = 0.5) == 'он кот'
	assert say(hotwords = ['он кот', 'код'], hotword_weight = 0.5, lm_path = I.SMALL, beam_alpha = 0.0, beam_beta = 0.0) == 'он кот'
	scores = decoders.BeamSearchDecoder(tok, beam_width = 16, hotwords = ['он кот'], hotword_weight = 0.5).decode_with_scores(x)[3]
	assert scores.dtype == torch.float64


@gpu
def test_transcribe_setup_with_hotwords(tmp_path):
	import convasr_amd as ca
	from convasr_amd.transcript_generators import BeamCTCGenerator
	g, j = _fixture()
	T_ = lambda a: torch.as_tensor(np.asarray(a))
	sd = {k[3:]: T_(g[k]) for k in g.files if k.startswith('sd/')}
	ckpt_args = dict(j['args'], alphabet = j['alphabet'], model_kwargs = dict(base_width = 32, kernel_sizes = [11], out_width_factors = [2], dropouts = [0.2], out_width_factors_large = [2, 2], residual = False, repeat = 1, nonlinearity = ('hardtanh', 0, 20), dilation = 2))
	listed = tmp_path / 'hot.txt'
	listed.write_text('он кот\n\nдом\n', encoding = 'utf-8')
	said = {}
	try:
		for name, hot, weight in (('none', None, None), ('zero', ['он кот'], 0.0), ('list', ['он кот'], 0.5), ('file', str(listed), 0.5)):
			args = types.SimpleNamespace(checkpoint = dict(args = dict(ckpt_args), model_state_dict = {k: v.clone() for k, v in sd.items()}), device = 'cuda:0', fp16 = None,
			                             frontend_in_model = True, model = None, align = False, decoder = 'BeamSearchDecoder', beam_width = 16, decoder_topk = 1,
			                             hotwords = hot, hotword_weight = weight)
			text_pipeline, frontend, model, generator = ca.transcribe.setup(args)
			assert isinstance(generator, BeamCTCGenerator)
			tok = text_pipeline.tokenizer
			out = generator.generate(tokenizer = tok, log_probs = torch.from_numpy(_word_case(tok)).cuda(), begin = torch.zeros(1), end = torch.ones(1))
			said[name] = ''.join(s['hyp'] for s in out[0][0])
	finally:
		torch.set_grad_enabled(True)
	assert said == dict(none = 'он кол', zero = 'он кол', list = 'он кот', file = 'он кот')


@gpu
def test_reruns_and_graph_capture():
	from convasr_amd import ops
	M = _model(I.SMALL, I.RU_LABELS)
	for form in ('free', 'lm'):
		lp, lengths, ref = I.form_case(form, M.arpa, I.RU_LABELS, 0.7, 8, 200, 256, 40, 4, 1.0)
		hw = _hot(I.FREE_PHRASES if form == 'free' else I.LM_PHRASES, I.RU_LABELS)
		model = M if form == 'lm' else None
		a = _run(lp, lengths, 37, 256, hw, 0.7, model, 40, 1.0, 4)
		b = _run(lp, lengths, 37, 256, hw, 0.7, model, 40, 1.0, 4)
		_compare(a, ref, ('rerun', form))
		for x, y in zip(a, b):
			assert x.tobytes() == y.tobytes()
		# graph capture: the tables are uploaded by the eager calls above; the call itself has no copy, memset or host synchronisation
		x = torch.from_numpy(lp).cuda().permute(0, 2, 1)
		lens = torch.from_numpy(lengths).cuda()
		call = lambda: ops.ctc_beam_search_hot(x, lens, 37, 256, hw, 0.7, model, I.LM_ALPHA, I.LM_BETA, 40, 1.0, 4)
		s = torch.cuda.Stream()
		s.wait_stream(torch.cuda.current_stream())
		with torch.cuda.stream(s):
			call()
		torch.cuda.current_stream().wait_stream(s)
		graph = torch.cuda.CUDAGraph()
		with torch.cuda.graph(graph):
			out = call()
		for o in out:
			o.fill_(-7)
		graph.replay()
		torch.cuda.synchronize()
		for o, e in zip(out, a):
			assert o.cpu().numpy().tobytes() == e.tobytes()


@gpu
def test_refusals():
	from convasr_amd import _lib, decoders, ops
	from convasr_amd.transcript_generators import CharTokenizerLegacy
	M = _model(I.SMALL, I.RU_LABELS)
	hw = _hot(I.LM_PHRASES, I.RU_LABELS)
	x = torch.from_numpy(_peaked(2, 8, 38, 1)).cuda().permute(0, 2, 1)
	wide_labels = ''.join(chr(0x4e00 + k) for k in range(298)) + ' |'  # C = 300
	big = _hot([chr(0x4e00) + chr(0x4e01)], wide_labels)
	with pytest.raises(_lib.ConvasrHipError, match = '256'):
		ops.ctc_beam_search_hot(torch.from_numpy(_peaked(2, 8, 300, 1)).cuda().permute(0, 2, 1), None, 299, 8, big, 1.0)
	with pytest.raises(ValueError, match = 'кошка'):
		ops.ctc_beam_search_hot(x, None, 37, 8, _hot(['кошка'], I.RU_LABELS), 1.0, M, 0.5, 0.0)
	for bad in (float('nan'), float('inf'), -1.0):
		with pytest.raises((ValueError, _lib.ConvasrHipError), match = 'finite'):
			ops.ctc_beam_search_hot(x, None, 37, 8, hw, bad)
	tok = CharTokenizerLegacy(I.ALPHA)
	with pytest.raises(ValueError, match = 'hotword_weight'):
		decoders.BeamSearchDecoder(tok, beam_width = 8, hotwords = ['кот'])
	with pytest.raises(ValueError, match = 'кошка'):
		decoders.BeamSearchDecoder(tok, beam_width = 8, lm_path = I.SMALL, hotwords = ['кошка'], hotword_weight = 1.0)
	# the C entry point's own checks, past the Python ones
	t = hw.device_tables(37, x.device)
	lp = x.permute(0, 2, 1).contiguous()
	lens = torch.full((2,), 8, dtype = torch.int64, device = x.device)
	tokens, offsets = torch.empty(2, 1, 8, dtype = torch.int64, device = x.device), torch.empty(2, 1, 8, dtype = torch.int32, device = x.device)
	out_len, logp = torch.empty(2, 1, dtype = torch.int64, device = x.device), torch.empty(2, 1, dtype = torch.float64, device = x.device)
	ws = torch.empty(2 * 8 * 8 * 8, dtype = torch.uint8, device = x.device)
	head = (_lib.ptr(lp), _lib.ptr(lens), _lib.ptr(tokens), _lib.ptr(offsets), _lib.ptr(out_len), _lib.ptr(logp), _lib.ptr(ws), 2, 8, 38, 37, 8, 38, 1.0, 1)
	tabs = (_lib.ptr(t['hot_mask']), _lib.ptr(t['hot_child']), _lib.ptr(t['hot_term']))
	for n_nodes, words, space, weight, what in ((0, 2, 36, 1.0, 'empty'), (hw.num_nodes, 1, 36, 1.0, 'mask words'), (hw.num_nodes, 2, 37, 1.0, 'space'),
	                                          (hw.num_nodes, 2, 38, 1.0, 'space'), (hw.num_nodes, 2, 36, float('nan'), 'finite'), (hw.num_nodes, 2, 36, -0.5, 'finite')):
		with pytest.raises(_lib.ConvasrHipError, match = what):
			_lib.call('convasr_ctc_beam_search_hot', *head, *tabs, n_nodes, words, space, weight, _lib.stream_ptr())
	torch.cuda.synchronize()
