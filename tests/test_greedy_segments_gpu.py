"""The greedy decode on the MI355X: ops.ctc_greedy_segments against the numpy restatement of its rule (tests/_greedy_ref.py), exact, on
shapes that straddle the kernel's chunks; GreedyCTCGenerator.generate on CUDA tensors against its host loop generate_host, segment for
segment; which inputs take which route; determinism; the transcribe goldens through the device route."""
import json
import os
import random
import types

import numpy as np
import pytest
import torch

import _greedy_ref as R

pytestmark = pytest.mark.gpu
BATS = (0, 1, 3, 10)


@pytest.fixture(scope = 'module')
def tok():
	from convasr_amd.transcript_generators import CharTokenizerLegacy
	return CharTokenizerLegacy('ab')


def _dev():
	return torch.device('cuda:0')


def _chunk():
	from convasr_amd import ops
	return ops.ctc_greedy_segments_chunk()


def _run_path(rng, T, eps, space, longest = 12):
	path = []
	while len(path) < T:
		c = rng.choice((eps, eps, space, rng.randrange(3), rng.randrange(3)))
		path += [c] * rng.randint(1, longest)
	return path[:T]


def _mixed_batch(T, seed, eps, space):
	"""B = 5 with mixed lengths: full, random, 0, all silence, speech only at or after the length."""
	rng = random.Random(seed)
	paths = [_run_path(rng, T, eps, space) for _ in range(5)]
	paths[3] = [rng.choice((eps, space)) for _ in range(T)]
	cut = T // 2
	paths[4] = [rng.choice((eps, space)) for _ in range(cut)] + [0] * (T - cut)
	return paths, [T, rng.randint(0, T), 0, T, cut]


def _straddle_batch(CH, bats, eps, space):
	"""Runs of blanks and of spaces of bats + 2 frames that begin at every offset from -bats - 1 to +1 around the chunk boundary CH, the same
	letter on both sides of the run; a blank run, a space run and a run of one letter longer than two chunks with speech on both sides; a
	leading silence longer than a chunk; a length of 0; speech only at or after the length."""
	T = 3 * CH + 40
	rng = random.Random(bats)
	paths, lengths = [], []
	for cls in (eps, space):
		for off in range(-bats - 1, 2):
			p = _run_path(rng, T, eps, space, 5)
			lo, hi = CH + off, CH + off + bats + 2
			p[lo:hi] = [cls] * (hi - lo)
			p[lo - 1] = p[hi] = 1
			paths.append(p)
			lengths.append(rng.choice((T, T, hi, hi + 1, CH, CH + 1)))
	for cls, tail in ((eps, [0, space, 1]), (space, [0, 0, eps, 0]), (0, [eps, space, space, 1])):
		p = _run_path(rng, T, eps, space, 5)
		p[7] = 0
		p[8:8 + 2 * CH + 9] = [cls] * (2 * CH + 9)
		p[8 + 2 * CH + 9:8 + 2 * CH + 9 + len(tail)] = tail
		paths.append(p)
		lengths.append(T)
	p = _run_path(rng, T, eps, space, 5)
	p[:CH + 17] = [rng.choice((eps, space)) for _ in range(CH + 17)]
	paths.append(p)
	lengths.append(T - 3)
	paths.append(_run_path(rng, T, eps, space, 5))
	lengths.append(0)
	paths.append([eps, space] * (CH // 2 + 1) + [0, 1] * ((T - CH - 2) // 2))
	lengths.append(CH + 2)
	return paths, lengths


def _cases(tok):
	"""(name, paths, lengths, bats) of every case the kernel and the generator are held to."""
	CH, eps, space = _chunk(), tok.eps_id, tok.space_id
	out = []
	for k, T in enumerate((1, 2, 63, 64, 65, CH - 1, CH, CH + 1, 2 * CH + 3)):
		paths, lengths = _mixed_batch(T, 100 + k, eps, space)
		out.append((f'T{T}', paths, lengths, BATS[k % 4]))
	for bats in BATS:
		out.append((f'straddle{bats}', *_straddle_batch(CH, bats, eps, space), bats))
	return out


def _check_ops(tok, paths, lengths, bats, split):
	from convasr_amd import ops
	d = _dev()
	got = ops.ctc_greedy_segments(torch.tensor(paths, device = d), torch.tensor(lengths, device = d), tok.eps_id, tok.space_id, bats, split_words = split)
	want = R.greedy_segments_batch(paths, lengths, tok.eps_id, tok.space_id, bats, split)
	dtypes = (torch.int64, torch.int32, torch.int64, torch.int64, torch.int32, torch.int32)
	for name, g, w, dt in zip(('tokens', 'frames', 'counts', 'seg_first', 'seg_begin', 'seg_end'), got, want, dtypes):
		assert g.is_cuda and g.dtype == dt, name
		assert g.cpu().tolist() == w, (name, bats, split)


def test_ops_equal_the_restatement(tok):
	for name, paths, lengths, bats in _cases(tok):
		for split in (True, False):
			for b in (BATS if name.startswith('T') and len(paths[0]) in (65, _chunk() + 1) else (bats, )):
				_check_ops(tok, paths, lengths, b, split)


def test_ops_argument_checks(tok):
	from convasr_amd import ops, _lib
	d = _dev()
	path = torch.zeros(2, 10, dtype = torch.int64, device = d)
	with pytest.raises(ValueError):
		ops.ctc_greedy_segments(path.int(), None, 6, 5)
	with pytest.raises(ValueError):
		ops.ctc_greedy_segments(path[0], None, 6, 5)
	with pytest.raises(ValueError):
		ops.ctc_greedy_segments(path, torch.zeros(3, dtype = torch.int64), 6, 5)
	with pytest.raises(_lib.ConvasrHipError):
		ops.ctc_greedy_segments(path, None, 5, 5)
	with pytest.raises(Exception):
		ops.ctc_greedy_segments(path.cpu(), None, 6, 5)
	tokens, frames, counts, first, begin, end = ops.ctc_greedy_segments(path, None, 6, 5)  # lengths None: all T; 'a' x 10 -> one token
	assert tokens.tolist() == [0, 0] and frames.tolist() == [0, 0] and counts.tolist() == [[1, 1], [1, 1]]
	assert first.tolist() == [0, 1] and begin.tolist() == [0, 0] and end.tolist() == [0, 0]


def _generate_both(tok, paths, lengths, bats, with_ts, seed = 0, **kw):
	from convasr_amd.transcript_generators import GreedyCTCGenerator
	d = _dev()
	B, T = len(paths), len(paths[0])
	g = torch.Generator().manual_seed(seed)
	lp = torch.nn.functional.one_hot(torch.tensor(paths), tok.vocab_size).permute(0, 2, 1).float().to(d)
	begin, end = (torch.rand(B, generator = g) * 4 - 1).to(d), (torch.rand(B, generator = g) + 5).to(d)
	ts = torch.cumsum(torch.rand(B, T, generator = g), 1).to(d) if with_ts else None
	olen = torch.tensor(lengths, device = d) if lengths is not None else None
	gen = GreedyCTCGenerator(bats)
	got = gen.generate(tok, lp, begin, end, output_lengths = olen, time_stamps = ts, **kw)
	want = gen.generate_host(tok, lp, begin, end, output_lengths = olen, time_stamps = ts, **kw)
	return got, want


def test_generate_equals_the_host_loop(tok, monkeypatch):
	from convasr_amd import ops
	calls = []
	real = ops.ctc_greedy_segments
	monkeypatch.setattr(ops, 'ctc_greedy_segments', lambda *a, **k: calls.append(1) or real(*a, **k))
	n = 0
	for name, paths, lengths, bats in _cases(tok):
		for with_ts in (True, False):
			got, want = _generate_both(tok, paths, lengths, bats, with_ts, seed = n)
			n += 1
			assert len(calls) == n
			assert got == want, (name, with_ts)
			assert all(len(alt) == 1 and type(alt[0]) is type(w[0]) for alt, w in zip(got, want))
	paths, lengths, bats = _cases(tok)[-1][1:]
	extra = [dict(speaker = b % 2, channel = b) for b in range(len(paths))]
	got, want = _generate_both(tok, paths, None, bats, True, segment_text_key = 'ref', segment_extra_info = extra)
	assert got == want and any(seg['channel'] == 3 and 'ref' in seg for seg in got[3][0])


def test_generate_one_long_recording(tok):
	rng = random.Random(5)
	path = []
	while len(path) < 200000:
		r = rng.random()
		path += [tok.eps_id if r < 0.6 else tok.space_id if r < 0.63 else rng.randrange(5)] * 3
	got, want = _generate_both(tok, [path[:200000]], [199990], 10, True)
	assert got == want and len(want[0][0]) > 1000


def test_routes(tok, monkeypatch):
	from convasr_amd.transcript_generators import CharTokenizerLegacy, GreedyCTCGenerator
	d = _dev()
	paths, lengths = _mixed_batch(70, 1, tok.eps_id, tok.space_id)
	lp = torch.nn.functional.one_hot(torch.tensor(paths), tok.vocab_size).permute(0, 2, 1).float()
	begin, end, ts = torch.zeros(5), torch.ones(5), torch.arange(70.).expand(5, -1)
	gen = GreedyCTCGenerator(3)
	want = gen.generate_host(tok, lp, begin, end, lengths, ts)
	hits = []

	def refuse(*a, **k):
		hits.append(1)
		raise AssertionError('generate_host called')
	monkeypatch.setattr(GreedyCTCGenerator, 'generate_host', refuse)
	assert gen.generate(tok, lp.to(d), begin.to(d), end.to(d), torch.tensor(lengths, device = d), ts.to(d)) == want and not hits
	assert gen.generate(tok, lp.to(d), begin, end, torch.tensor(lengths), ts) == want and not hits  # lengths and stamps may live on the host

	class OtherWordStart(CharTokenizerLegacy):
		def is_start_word_token(self, idx):
			return idx in (self.space_id, 1)

	class OtherSilence(CharTokenizerLegacy):
		silence_tokens_ids = property(lambda self: {self.eps_id})
	for k, call in enumerate((lambda: gen.generate(OtherWordStart('ab'), lp.to(d), begin, end, torch.tensor(lengths), ts),
	                          lambda: gen.generate(OtherSilence('ab'), lp.to(d), begin, end, torch.tensor(lengths), ts),
	                          lambda: gen.generate(tok, lp.to(d), begin, end, lengths, ts),  # lengths as a list
	                          lambda: gen.generate(tok, lp, begin, end, torch.tensor(lengths), ts))):  # CPU log-probs
		with pytest.raises(AssertionError, match = 'generate_host called'):
			call()
		assert len(hits) == k + 1


def test_deterministic_and_independent_of_the_batch(tok):
	from convasr_amd import ops
	d = _dev()
	name, paths, lengths, bats = _cases(tok)[-2]
	path, n = torch.tensor(paths, device = d), torch.tensor(lengths, device = d)
	one = ops.ctc_greedy_segments(path, n, tok.eps_id, tok.space_id, bats)
	two = ops.ctc_greedy_segments(path, n, tok.eps_id, tok.space_id, bats)
	for a, b in zip(one, two):
		assert torch.equal(a, b)
	tokens, frames, counts, first, begin, end = [t.cpu() for t in one]
	tok_off, seg_off = [0] + counts[0].cumsum(0).tolist(), [0] + counts[1].cumsum(0).tolist()
	for b in range(len(paths)):
		alone = [t.cpu() for t in ops.ctc_greedy_segments(path[b:b + 1], n[b:b + 1], tok.eps_id, tok.space_id, bats)]
		assert alone[2].tolist() == [[counts[0][b]], [counts[1][b]]]
		assert torch.equal(alone[0], tokens[tok_off[b]:tok_off[b + 1]]) and torch.equal(alone[1], frames[tok_off[b]:tok_off[b + 1]])
		assert torch.equal(alone[3] + tok_off[b], first[seg_off[b]:seg_off[b + 1]])
		assert torch.equal(alone[4], begin[seg_off[b]:seg_off[b + 1]]) and torch.equal(alone[5], end[seg_off[b]:seg_off[b + 1]])


def test_transcribe_batch_reproduces_the_golden_segments_on_the_device_route(monkeypatch):
	"""tests/golden/transcribe.json holds the segments the reference's own generator wrote (loaded as tests/test_bf16_parity_gpu.py does):
	text identical, begin / end to 1e-5 s, with the host loop out of reach -- both decodes of transcribe_batch (the hypotheses, and the
	one-hot targets under --align with ylen as lengths) run ops.ctc_greedy_segments."""
	import convasr_amd as ca
	from convasr_amd.transcript_generators import GreedyCTCGenerator
	root = os.path.dirname(os.path.abspath(__file__))
	g = np.load(os.path.join(root, 'golden', 'transcribe.npz'))
	j = json.load(open(os.path.join(root, 'golden', 'transcribe.json')))
	T_ = lambda a: torch.as_tensor(np.asarray(a))
	sd = {k[3:]: T_(g[k]) for k in g.files if k.startswith('sd/')}
	ckpt_args = dict(j['args'], alphabet = j['alphabet'], model_kwargs = dict(base_width = 32, kernel_sizes = [11], out_width_factors = [2], dropouts = [0.2], out_width_factors_large = [2, 2], residual = False, repeat = 1, nonlinearity = ('hardtanh', 0, 20), dilation = 2))
	args = types.SimpleNamespace(checkpoint = dict(args = dict(ckpt_args), model_state_dict = {k: v.clone() for k, v in sd.items()}), device = 'cuda:0', fp16 = None, frontend_in_model = True, model = None, align = True)
	try:
		text_pipeline, frontend, model, generator = ca.transcribe.setup(args)
		assert isinstance(generator, GreedyCTCGenerator)

		def refuse(*a, **k):
			raise AssertionError('generate_host called')
		monkeypatch.setattr(GreedyCTCGenerator, 'generate_host', refuse)
		res = ca.transcribe.transcribe_batch(args, text_pipeline, model, generator, T_(g['wav']).unsqueeze(1), T_(g['xlen']), T_(g['begin']), T_(g['end']), y = T_(g['y']), ylen = T_(g['ylen']), segment_extra_info = j['extra'])
		for got_list, want_list, key in ((res.hyp_segments, j['hyp_segments'], 'hyp'), (res.ref_segments, j['ref_segments'], 'ref')):
			assert [len(s) for s in got_list] == [len(s) for s in want_list] and sum(len(s) for s in want_list) > 0
			for got, want in zip(sum(got_list, []), sum(want_list, [])):
				assert got[key] == want[key] and got['speaker'] == want['speaker'] and got['channel'] == want['channel'], (got, want)
				assert abs(got['begin'] - want['begin']) <= 1e-5 and abs(got['end'] - want['end']) <= 1e-5, (got, want)
		assert res.hyp == j['hyp']
	finally:
		torch.set_grad_enabled(True)  # (transcribe.setup switches autograd off for the process, like the reference)
