"""convasr_ctc_beam_search on the MI355X against the float64 restatement (tests/_ctc_beam_ref.py), the CTC loss kernel, and through
decoders.BeamSearchDecoder / transcribe.setup(decoder = 'BeamSearchDecoder') on the transcribe fixture.

Inputs are only compared where the restatement's decisions have a margin (min_gap) above GAP.  The kernel keeps beam scores in fp64 and
uses numpy's logaddexp formula, so it differs from the restatement by rounding in the last bits of exp / log1p (~1e-13 on scores of a
few hundred); the log-probs are fp32, so sums of them differ by multiples of ~5e-7, and a seed whose search rests on an exact tie (gap 0)
or a rounding-level one is skipped for the next.  (A 1e-3 margin, what an fp32 search would need, is out of reach at W = 1024 over 750
frames: the W-th and (W+1)-th of ~40,000 candidates lie closer than that in most frames.)"""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ctc_beam_ref as R  # noqa: E402

gpu = pytest.mark.gpu
GAP = 1e-9
ROOT = os.path.dirname(os.path.abspath(__file__))


def _peaked(B, T, C, seed, sharp = 4.0):
	"""(B, T, C) fp32 log-probs: one class per frame raised by `sharp` over unit-normal logits."""
	rng = np.random.default_rng(seed)
	x = rng.normal(size = (B, T, C))
	x[np.arange(B)[:, None], np.arange(T)[None, :], rng.integers(0, C, (B, T))] += sharp
	return (x - np.logaddexp.reduce(x, axis = -1, keepdims = True)).astype(np.float32)


def _lengths(B, T):
	return np.array([T, 0, 1, max(T // 2, 1), max(T - 7, 1), max(3 * T // 4, 1), min(17, T), T][:B], dtype = np.int64)


def _gpu(lp_btc, lengths, blank, W, N, cutoff = 1.0, topk = 1):
	from convasr_amd import ops
	x = torch.from_numpy(lp_btc).cuda().permute(0, 2, 1)  # (B, C, T) view of (B, T, C) memory: the model's channels-last layout
	out = ops.ctc_beam_search(x, torch.from_numpy(lengths), blank, W, N, cutoff, topk)
	torch.cuda.synchronize()
	return [o.cpu().numpy() for o in out]


def _case(B, T, C, W, N, topk, cutoff = 1.0, blank = None):
	"""The first seed whose restatement has a margin above GAP: (lp, lengths, blank, reference outputs)."""
	blank = C - 1 if blank is None else blank
	N = min(N, C)
	lengths = _lengths(B, T)
	for seed in range(6):
		lp = _peaked(B, T, C, 1000 * T + 10 * C + seed)
		ref = R.decode(lp, lengths, blank, W, N, float(np.float32(cutoff)), topk)
		if ref[-1] > GAP:
			return lp, lengths, blank, N, ref
	pytest.fail(f'no seed with a decision margin above {GAP} for T {T} C {C} W {W} N {N}')


def _compare(got, ref, what):
	tokens, offsets, out_len, logp = got
	rt, ro, rl, rp = ref[:4]
	assert np.array_equal(out_len, rl), (what, out_len, rl)
	assert np.array_equal(tokens, rt), (what, np.argwhere(tokens != rt)[:5])
	assert np.array_equal(offsets, ro), (what, np.argwhere(offsets != ro)[:5])
	fin = np.isfinite(rp)
	assert np.array_equal(np.isfinite(logp), fin) and np.all(logp[~fin] == rp[~fin]), (what, logp, rp)
	err = np.abs(logp[fin] - rp[fin])
	assert np.all(err <= 1e-3 + 1e-5 * np.abs(rp[fin])), (what, err.max())


CASES = [  # (T, C, W, N, topk)
	(1, 38, 8, 5, 4),
	(1, 38, 1, 40, 1),
	(1, 128, 256, 128, 4),
	(1, 1024, 1024, 40, 4),
	(60, 38, 1, 40, 1),
	(60, 128, 8, 5, 4),
	(60, 1024, 64, 40, 4),
	(60, 128, 256, 128, 4),
	(60, 38, 256, 38, 1),
	(60, 1024, 1024, 40, 1),
	(750, 38, 1, 40, 1),
	(750, 38, 64, 40, 4),
	(750, 1024, 8, 5, 1),
	(750, 128, 1024, 40, 4),
]


@gpu
def test_beam_search_matches_the_restatement():
	for T, C, W, N, topk in CASES:
		lp, lengths, blank, N, ref = _case(8, T, C, W, N, topk)
		_compare(_gpu(lp, lengths, blank, W, N, 1.0, topk), ref, (T, C, W, N, topk))
	# a blank that is not the last class, and length-0 / length-1 utterances of a batch whose every other utterance is long
	lp, lengths, blank, N, ref = _case(8, 60, 38, 16, 10, 4, blank = 0)
	_compare(_gpu(lp, lengths, blank, 16, N, 1.0, 4), ref, 'blank 0')


@gpu
def test_cutoff_prob_matches_the_restatement():
	for T, C, W, N, topk, cutoff in ((60, 38, 16, 38, 4, 0.9), (60, 128, 64, 40, 4, 0.5), (200, 1024, 32, 128, 1, 0.99), (60, 38, 8, 38, 2, 0.05)):
		lp, lengths, blank, N, ref = _case(8, T, C, W, N, topk, cutoff)
		_compare(_gpu(lp, lengths, blank, W, N, cutoff, topk), ref, (T, C, W, N, topk, cutoff))


@gpu
def test_top_hypothesis_agrees_with_the_ctc_loss_kernel():
	"""Nothing pruned (W above the number of reachable labellings, N = C): the top beam's log-probability is -ctc_loss of its labelling.
	Pruned: it can only be lower."""
	from convasr_amd import ops
	for T, C, W, N, exact in ((5, 4, 1024, 4, True), (6, 3, 1024, 3, True), (60, 38, 8, 5, False), (200, 128, 64, 40, False)):
		B = 8
		lp = _peaked(B, T, C, 77 + T, sharp = 2.0)
		lengths = np.full(B, T, dtype = np.int64)
		tokens, _, out_len, logp = _gpu(lp, lengths, C - 1, W, N, 1.0, 1)
		S = max(int(out_len.max()), 1)
		targets = torch.zeros(B, S, dtype = torch.int64)
		for b in range(B):
			targets[b, :out_len[b, 0]] = torch.from_numpy(tokens[b, 0, :out_len[b, 0]])
		x = torch.from_numpy(lp).cuda().permute(0, 2, 1)
		nll, _ = ops.ctc_loss(x, targets, torch.from_numpy(lengths), torch.from_numpy(out_len[:, 0].copy()), C - 1, need_grad = False)
		want = -nll.cpu().double().numpy()
		if exact:
			assert np.all(np.abs(logp[:, 0] - want) <= 1e-4), (logp[:, 0], want)
		else:
			assert np.all(logp[:, 0] <= want + 1e-4), (logp[:, 0], want)


@gpu
def test_lengths_must_match_the_batch():
	from convasr_amd import ops
	x = torch.from_numpy(_peaked(4, 10, 38, 5)).cuda().permute(0, 2, 1)
	with pytest.raises(ValueError, match = 'lengths'):
		ops.ctc_beam_search(x, torch.tensor([10, 10]), 37, 8, 5)


@gpu
def test_two_runs_are_bitwise_identical():
	lp, lengths, blank, N, _ = _case(8, 200, 128, 256, 40, 4)
	a = _gpu(lp, lengths, blank, 256, N, 1.0, 4)
	b = _gpu(lp, lengths, blank, 256, N, 1.0, 4)
	for x, y in zip(a, b):
		assert x.tobytes() == y.tobytes()


def _fixture():
	g = np.load(os.path.join(ROOT, 'golden', 'transcribe.npz'))
	j = json.load(open(os.path.join(ROOT, 'golden', 'transcribe.json')))
	return g, j


@gpu
def test_decoders_on_the_transcribe_fixture():
	from convasr_amd import decoders
	from convasr_amd.transcript_generators import CharTokenizerLegacy
	g, j = _fixture()
	tok = CharTokenizerLegacy(j['alphabet'])
	lp, olen = g['log_probs'], g['olen']  # (B, C, T) fp32, frames per utterance
	x = torch.from_numpy(lp).cuda()
	# greedy: the reference's form (decoders.py:5-16) computed on the CPU
	for K in (1, 3):
		want = [l[... if K > 1 else 0, :o].tolist() for o, l in zip(olen.tolist(), torch.from_numpy(lp).topk(K, dim = 1).indices)]
		assert decoders.GreedyDecoder().decode(x, torch.from_numpy(olen), K = K) == want
	lp_btc = np.ascontiguousarray(lp.transpose(0, 2, 1))
	for W, topk in ((16, 1), (64, 3)):
		ref = R.decode(lp_btc, olen, tok.eps_id, W, lp.shape[1], 1.0, topk)
		assert ref[-1] > GAP
		dec = decoders.BeamSearchDecoder(tok, beam_width = W, cutoff_top_n = 40, topk = topk)
		got = dec.decode(x, torch.from_numpy(olen))
		for b in range(lp.shape[0]):
			want = [ref[0][b, k, :ref[2][b, k]].tolist() for k in range(topk)]
			assert got[b] == (want if topk > 1 else want[0])
			if topk == 1:
				assert tok.decode([got[b]])[0] == tok.decode([want[0]])[0] and len(got[b]) > 20
		_compare([o.cpu().numpy() for o in dec.decode_with_scores(x, torch.from_numpy(olen))], ref, ('fixture', W, topk))


@gpu
def test_transcribe_setup_with_the_beam_search_decoder():
	"""args.decoder = 'BeamSearchDecoder': segments built from the top beam (word starts at spaces, times = begin + ts[offset]); without a
	decoder, or with 'GreedyDecoder', the greedy output of the fixture as before.  With args.align, the reference segments are the fixture's
	(the one-hot targets go through the greedy collapse) for every decoder."""
	import convasr_amd as ca
	from convasr_amd.transcript_generators import BeamCTCGenerator, GreedyCTCGenerator
	g, j = _fixture()
	T_ = lambda a: torch.as_tensor(np.asarray(a))
	sd = {k[3:]: T_(g[k]) for k in g.files if k.startswith('sd/')}
	ckpt_args = dict(j['args'], alphabet = j['alphabet'], model_kwargs = dict(base_width = 32, kernel_sizes = [11], out_width_factors = [2], dropouts = [0.2], out_width_factors_large = [2, 2], residual = False, repeat = 1, nonlinearity = ('hardtanh', 0, 20), dilation = 2))
	results = {}
	try:
		for decoder in (None, 'GreedyDecoder', 'BeamSearchDecoder'):
			args = types.SimpleNamespace(checkpoint = dict(args = dict(ckpt_args), model_state_dict = {k: v.clone() for k, v in sd.items()}), device = 'cuda:0', fp16 = None, frontend_in_model = True, model = None, align = True)
			if decoder is not None:
				args.decoder, args.beam_width, args.decoder_topk = decoder, 32, 2
			text_pipeline, frontend, model, generator = ca.transcribe.setup(args)
			assert isinstance(generator, BeamCTCGenerator if decoder == 'BeamSearchDecoder' else GreedyCTCGenerator)
			results[decoder] = (ca.transcribe.transcribe_batch(args, text_pipeline, model, generator, T_(g['wav']).unsqueeze(1), T_(g['xlen']), T_(g['begin']), T_(g['end']), y = T_(g['y']), ylen = T_(g['ylen']), segment_extra_info = j['extra']), text_pipeline, generator)
	finally:
		torch.set_grad_enabled(True)
	greedy, plain = results['GreedyDecoder'][0], results[None][0]
	assert plain.hyp == j['hyp'] and greedy.hyp == plain.hyp and greedy.hyp_segments == plain.hyp_segments
	res, text_pipeline, generator = results['BeamSearchDecoder']
	# --align: the reference segments come from the one-hot targets through the greedy collapse, whatever the decoder
	assert torch.equal(res.alignment.cpu(), T_(g['alignment'])) and res.ref_segments == plain.ref_segments == greedy.ref_segments
	for got, want in zip(sum(res.ref_segments, []), sum(j['ref_segments'], [])):
		assert got['ref'] == want['ref'] and abs(got['begin'] - want['begin']) <= 1e-5 and abs(got['end'] - want['end']) <= 1e-5, (got, want)
	tok = text_pipeline.tokenizer
	lp_btc = res.log_probs.permute(0, 2, 1).contiguous().cpu().numpy()
	olen = res.olen.cpu().numpy()
	ref = R.decode(lp_btc, olen, tok.eps_id, 32, min(40, lp_btc.shape[2]), 1.0, 2)
	assert ref[-1] > GAP
	ts, begin = res.ts.cpu().tolist(), g['begin'].tolist()
	for b, segs in enumerate(res.hyp_segments):
		toks, offs = ref[0][b, 0, :ref[2][b, 0]].tolist(), ref[1][b, 0, :ref[2][b, 0]].tolist()
		start = next(i for i, c in enumerate(toks) if c not in tok.silence_tokens_ids)
		assert ''.join(s['hyp'] for s in segs) == tok.decode([toks[start:]])[0]
		word_starts = [start] + [i for i in range(start + 1, len(toks)) if tok.is_start_word_token(toks[i])]
		assert len(segs) == len(word_starts)
		for s, i in zip(segs, word_starts):
			assert abs(s['begin'] - (max(begin[b], 0.0) + ts[b][offs[i]])) <= 1e-6 and s['speaker'] == j['extra'][b]['speaker']
		assert abs(segs[-1]['end'] - (max(begin[b], 0.0) + ts[b][offs[-1]])) <= 1e-6
		assert res.hyp[b] == ' '.join(s['hyp'].strip() for s in segs if s['hyp'].strip())
	# the generator's alternatives: topk = 2 transcripts per utterance, best first
	alts = generator.generate(tokenizer = tok, log_probs = res.log_probs, begin = T_(g['begin']), end = T_(g['end']), output_lengths = res.olen)
	assert all(len(a) == 2 for a in alts)
	for b, a in enumerate(alts):
		for k in range(2):
			toks = ref[0][b, k, :ref[2][b, k]].tolist()
			start = next((i for i, c in enumerate(toks) if c not in tok.silence_tokens_ids), len(toks))
			assert ''.join(s['hyp'] for s in a[k]) == tok.decode([toks[start:]])[0]
