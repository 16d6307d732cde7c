"""The wide CTC beam search (convasr_ctc_beam_search_wide / _lm_wide: the beam state in the workspace, W <= 8192) on the MI355X.

- At the widths both forms accept, wide = True gives the LDS kernel's bits: the arithmetic is the same, so any difference would be a
  changed summation order or a selection bug.
- Above 1024 (or the LM's LDS budget), against the float64 restatements (tests/_ctc_beam_ref.py, tests/_ctc_beam_lm_ref.py) on inputs
  whose decisions have a margin above GAP: tokens, offsets and lengths exactly, the score to 1e-9 relative (the LM-free score is
  returned in fp32: to its rounding).
- Bitwise reruns, a graph-captured call, and the reference transcribe.py's default --beam-width 5000 end to end."""
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
LABELS_MID = ALPHA[:5] + '|' + ALPHA[5:19] + ' ' + ALPHA[19:] + '*.2'  # blank 5, space 20
LABELS_256 = RU_LABELS + ''.join(chr(0x4E00 + i) for i in range(256 - len(RU_LABELS)))  # 218 classes no word uses


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


def _run(lp_btc, lengths, blank, W, N, cutoff, topk, M = None, alpha = 0.0, beta = 0.0, wide = None):
	from convasr_amd import ops
	x = torch.from_numpy(lp_btc).cuda().permute(0, 2, 1)
	lens = torch.from_numpy(lengths)
	if M is None:
		out = ops.ctc_beam_search(x, lens, blank, W, N, cutoff, topk, wide = wide)
	else:
		out = ops.ctc_beam_search_lm(x, lens, blank, W, M, alpha, beta, N, cutoff, topk, wide = wide)
	torch.cuda.synchronize()
	return [o.cpu().numpy() for o in out]


def _compare(got, ref, what):
	tokens, offsets, out_len, logp = got
	rt, ro, rl, rp = ref[:4]
	assert np.array_equal(out_len, rl), (what, out_len, rl)
	assert np.array_equal(tokens, rt), (what, np.argwhere(tokens != rt)[:5])
	assert np.array_equal(offsets, ro), (what, np.argwhere(offsets != ro)[:5])
	fin = np.isfinite(rp)
	assert np.array_equal(np.isfinite(logp), fin) and np.all(logp[~fin] == rp[~fin]), (what, logp, rp)
	err = np.abs(logp[fin].astype(np.float64) - rp[fin])
	tol = 1e-9 * np.maximum(np.abs(rp[fin]), 1.0)
	if logp.dtype == np.float32:  # the LM-free score: the fp64 score rounded to fp32
		tol = np.maximum(tol, np.spacing(np.abs(rp[fin]).astype(np.float32)).astype(np.float64))
	assert np.all(err <= tol), (what, err.max())


def _same_bits(a, b, what):
	for x, y, name in zip(a, b, ('tokens', 'offsets', 'lengths', 'log_prob')):
		assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, name)


@pytest.fixture(scope = 'module')
def orders(tmp_path_factory):
	d = tmp_path_factory.mktemp('lm')
	return {n: _lm_synth.write_small(str(d / f'o{n}.arpa'), n, seed = n) for n in (1, 2, 4, 6)}


@pytest.fixture(scope = 'module')
def big(tmp_path_factory):
	return _lm_synth.write(str(tmp_path_factory.mktemp('lm') / 'big.arpa'))


@gpu
def test_wide_kernel_gives_the_lds_kernels_bits(orders, big):
	"""W in {1, 8, 64, 1024}, T in {1, 60, 750}, C in {38, 1024}, cutoff_prob < 1, ragged lengths (0 and 1 among them), a blank that is
	not the last class: wide = True and wide = False return the same bytes, for both searches."""
	for T, C, W, N, topk, cutoff, blank in ((1, 38, 8, 40, 4, 1.0, 37), (60, 38, 1, 40, 1, 1.0, 37), (60, 38, 1024, 38, 4, 0.999, 0),
	                                        (750, 38, 64, 38, 4, 1.0, 37), (750, 38, 1024, 38, 4, 1.0, 37), (1, 1024, 1024, 40, 4, 1.0, 1023),
	                                        (60, 1024, 64, 40, 4, 0.99, 1023), (60, 1024, 1024, 128, 4, 1.0, 5), (750, 1024, 8, 5, 2, 0.9, 1023)):
		lp, lengths = _peaked(8, T, C, 7 * T + C + W), _lengths(8, T)
		args = (lp, lengths, blank, W, min(N, C), cutoff, topk)
		_same_bits(_run(*args, wide = True), _run(*args, wide = False), ('lm-free', T, C, W, N, cutoff, blank))
	for path, labels, T, W, topk, cutoff, alpha, beta in ((SMALL, RU_LABELS, 1, 8, 4, 1.0, 0.8, 1.0), (SMALL, RU_LABELS, 60, 1, 1, 1.0, 0.8, 1.0),
	                                                      (SMALL, RU_LABELS, 60, 1024, 4, 0.999, 0.4, 2.6), (orders[6], LABELS_MID, 750, 64, 4, 1.0, 0.6, -0.5),
	                                                      (SMALL, RU_LABELS, 750, 1024, 4, 1.0, 0.4, 2.6), (big, RU_LABELS, 60, 1024, 4, 1.0, 0.8, 0.5),
	                                                      (orders[2], RU_LABELS, 60, 64, 2, 0.9, 0.6, 1.0)):
		M = _model(path, labels)
		lp, lengths = _peaked(8, T, 38, 11 * T + W), _lengths(8, T)
		args = (lp, lengths, labels.index('|'), W, 38, cutoff, topk, M, alpha, beta)
		_same_bits(_run(*args, wide = True), _run(*args, wide = False), ('lm', os.path.basename(path), labels[:3], T, W, cutoff))


def _case(B, T, C, W, N, topk, cutoff = 1.0, blank = None):
	"""The first seed whose LM-free restatement has a margin above GAP."""
	blank = C - 1 if blank is None else blank
	lengths = _lengths(B, T)
	for seed in range(6):
		lp = _peaked(B, T, C, 1000 * T + 10 * W + seed)
		ref = R.decode(lp, lengths, blank, W, min(N, C), float(np.float32(cutoff)), topk)
		if ref[-1] > GAP:
			return lp, lengths, blank, ref
	pytest.fail(f'no seed with a decision margin above {GAP} for T {T} C {C} W {W} N {N}')


def _lm_case(B, T, M, alpha, beta, W, N, topk, cutoff = 1.0):
	"""The first seed whose LM restatement has a margin above GAP."""
	ref_model = RL.Model(M.arpa, ''.join(M.labels), M.labels.index('|'), alpha, beta)
	lengths = _lengths(B, T)
	for seed in range(6):
		lp = _peaked(B, T, M.num_classes, 1000 * T + 10 * W + seed)
		ref = RL.decode(lp, lengths, ref_model, W, min(N, M.num_classes), float(np.float32(cutoff)), topk)
		if ref[-1] > GAP:
			return lp, lengths, ref
	pytest.fail(f'no seed with a decision margin above {GAP} for T {T} W {W} N {N}')


@gpu
def test_wide_search_matches_the_restatement():
	"""W in {1025, 2048, 5000, 8192}, C in {38, 128}, topk up to 16, topk = W once (with unfilled slots); lengths T, 0 and 1."""
	for T, C, W, N, topk, cutoff in ((200, 38, 1025, 40, 16, 0.99), (60, 128, 2048, 128, 16, 1.0), (2, 38, 2048, 40, 2048, 1.0),
	                                 (200, 38, 5000, 40, 4, 1.0), (60, 38, 8192, 40, 8, 1.0)):
		lp, lengths, blank, ref = _case(3, T, C, W, N, topk, cutoff)
		_compare(_run(lp, lengths, blank, W, min(N, C), cutoff, topk), ref, (T, C, W, N, topk, cutoff))


@gpu
def test_wide_lm_search_matches_the_restatement(orders, big):
	"""Orders 1-6 with the small models, the 10^5-word model, and C = 256, N = 128 at W = 1024 (beyond the LDS form's budget)."""
	cases = [  # (model, labels, alpha, beta, T, W, N, topk, cutoff)
		(SMALL, RU_LABELS, 0.4, 2.6, 60, 5000, 40, 4, 1.0),
		(SMALL, RU_LABELS, 0.8, 1.0, 60, 1025, 40, 4, 0.999),
		(orders[1], RU_LABELS, 0.6, 1.0, 60, 2048, 40, 4, 1.0),
		(orders[2], RU_LABELS, 0.6, 1.0, 60, 8192, 40, 16, 1.0),
		(orders[4], LABELS_MID, 0.6, -0.5, 60, 2048, 40, 4, 1.0),
		(orders[6], RU_LABELS, 1.5, 3.0, 60, 5000, 40, 4, 1.0),
		(big, RU_LABELS, 0.4, 2.6, 60, 2048, 40, 16, 1.0),
		(big, RU_LABELS, 0.8, 0.5, 30, 8192, 40, 4, 1.0),
		(SMALL, LABELS_256, 0.4, 2.6, 60, 1024, 128, 4, 1.0),
	]
	from convasr_amd import _lib
	assert _lib.load().convasr_ctc_beam_search_lm_workspace_bytes(3, 60, 256, 1024, 128, 4) < 0  # the LDS form refuses the last case
	for path, labels, alpha, beta, T, W, N, topk, cutoff in cases:
		M = _model(path, labels)
		lp, lengths, ref = _lm_case(3, T, M, alpha, beta, W, N, topk, cutoff)
		got = _run(lp, lengths, labels.index('|'), W, min(N, M.num_classes), cutoff, topk, M, alpha, beta)
		assert got[3].dtype == np.float64
		_compare(got, ref, (os.path.basename(path), labels[:3], alpha, beta, T, W, N, topk, cutoff))


@gpu
def test_wide_reruns_and_graph_capture():
	from convasr_amd import ops
	lp, lengths = _peaked(4, 100, 38, 99), _lengths(4, 100)
	a = _run(lp, lengths, 37, 2048, 38, 1.0, 4)
	b = _run(lp, lengths, 37, 2048, 38, 1.0, 4)
	_same_bits(a, b, 'rerun')
	M = _model(SMALL, RU_LABELS)
	la = _run(lp, lengths, 37, 2048, 38, 1.0, 4, M, 0.4, 2.6)
	_same_bits(la, _run(lp, lengths, 37, 2048, 38, 1.0, 4, M, 0.4, 2.6), 'lm rerun')
	# a graph-captured wide call, replayed on new log-probs, equals the eager call on them
	lp2 = _peaked(4, 100, 38, 100)
	want, want_lm = _run(lp2, lengths, 37, 2048, 38, 1.0, 4), _run(lp2, lengths, 37, 2048, 38, 1.0, 4, M, 0.4, 2.6)
	x = torch.from_numpy(lp).cuda().permute(0, 2, 1)
	lens = torch.from_numpy(lengths).cuda()
	s = torch.cuda.Stream()
	s.wait_stream(torch.cuda.current_stream())
	with torch.cuda.stream(s):
		ops.ctc_beam_search(x, lens, 37, 2048, 38, 1.0, 4)
		ops.ctc_beam_search_lm(x, lens, 37, 2048, M, 0.4, 2.6, 38, 1.0, 4)
	torch.cuda.current_stream().wait_stream(s)
	g = torch.cuda.CUDAGraph()
	with torch.cuda.graph(g):
		out = ops.ctc_beam_search(x, lens, 37, 2048, 38, 1.0, 4)
		out_lm = ops.ctc_beam_search_lm(x, lens, 37, 2048, M, 0.4, 2.6, 38, 1.0, 4)
	x.copy_(torch.from_numpy(lp2).cuda().permute(0, 2, 1))
	for o in (*out, *out_lm):
		o.fill_(-7)
	g.replay()
	torch.cuda.synchronize()
	_same_bits([o.cpu().numpy() for o in out], want, 'graph')
	_same_bits([o.cpu().numpy() for o in out_lm], want_lm, 'graph lm')


def _fixture():
	g = np.load(os.path.join(ROOT, 'golden', 'transcribe.npz'))
	j = json.load(open(os.path.join(ROOT, 'golden', 'transcribe.json')))
	return g, j


@gpu
def test_the_reference_default_beam_width_end_to_end():
	"""transcribe.py's default --beam-width 5000: decoders.BeamSearchDecoder(beam_width = 5000, topk = 4) on the transcribe fixture equals
	the restatement; transcribe.setup(decoder = 'BeamSearchDecoder', beam_width = 5000) gives segments without and with --lm (at the
	reference's --beam-alpha 0.3 / --beam-beta 1.0)."""
	import convasr_amd as ca
	from convasr_amd import decoders
	from convasr_amd.transcript_generators import BeamCTCGenerator, CharTokenizerLegacy
	g, j = _fixture()
	tok = CharTokenizerLegacy(j['alphabet'])
	lp, olen = g['log_probs'], g['olen']
	lp_btc = np.ascontiguousarray(lp.transpose(0, 2, 1))
	ref = R.decode(lp_btc, olen, tok.eps_id, 5000, min(40, lp.shape[1]), 1.0, 4)
	assert ref[-1] > GAP
	dec = decoders.BeamSearchDecoder(tok, beam_width = 5000, topk = 4)
	got = dec.decode(torch.from_numpy(lp).cuda(), torch.from_numpy(olen))
	for b in range(lp.shape[0]):
		assert got[b] == [ref[0][b, k, :ref[2][b, k]].tolist() for k in range(4)]
	_compare([o.cpu().numpy() for o in dec.decode_with_scores(torch.from_numpy(lp).cuda(), torch.from_numpy(olen))], ref, 'fixture 5000')

	T_ = lambda a: torch.as_tensor(np.asarray(a))
	sd = {k[3:]: T_(g[k]) for k in g.files if k.startswith('sd/')}
	ckpt_args = dict(j['args'], alphabet = j['alphabet'], model_kwargs = dict(base_width = 32, kernel_sizes = [11], out_width_factors = [2], dropouts = [0.2], out_width_factors_large = [2, 2], residual = False, repeat = 1, nonlinearity = ('hardtanh', 0, 20), dilation = 2))
	try:
		for lm_path in (None, SMALL):
			args = types.SimpleNamespace(checkpoint = dict(args = dict(ckpt_args), model_state_dict = {k: v.clone() for k, v in sd.items()}), device = 'cuda:0', fp16 = None,
			                             frontend_in_model = True, model = None, align = False, decoder = 'BeamSearchDecoder', beam_width = 5000, decoder_topk = 1,
			                             lm = lm_path, beam_alpha = 0.3, beam_beta = 1.0)
			text_pipeline, frontend, model, generator = ca.transcribe.setup(args)
			assert isinstance(generator, BeamCTCGenerator)
			res = ca.transcribe.transcribe_batch(args, text_pipeline, model, generator, T_(g['wav']).unsqueeze(1), T_(g['xlen']), T_(g['begin']), T_(g['end']), segment_extra_info = j['extra'])
			assert len(res.hyp_segments) == len(olen) and any(res.hyp_segments), lm_path
			assert all(s['hyp'] for segs in res.hyp_segments for s in segs), lm_path
	finally:
		torch.set_grad_enabled(True)
