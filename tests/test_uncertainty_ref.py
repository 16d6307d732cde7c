"""The uncertainty rule without a GPU: tests/_uncertainty_ref.py (the float64 restatement the kernels are held against) equals the
reference's own numbers (tests/golden/uncertainty.npz, written by tests/golden/make_golden_uncertainty.py) up to the reference's fp32
rounding, a class-by-class and a span-by-span Python loop, and hand-written event lists; its spans are those of the host loop; and both
entry points refuse arguments outside their envelope before any launch."""
import ctypes
import math
import os
import random
import types

import numpy as np
import pytest
import torch

import _greedy_ref as G
import _uncertainty_ref as R

U = 2.0 ** -24  # half an ulp of an fp32 value in [1, 2): the unit of every fp32 bound below
P = ctypes.c_void_p(4096)  # any non-NULL value: never dereferenced


@pytest.fixture(scope = 'module')
def golden():
	g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'uncertainty.npz'))
	return types.SimpleNamespace(lp = np.ascontiguousarray(g['log_probs'].transpose(0, 2, 1)), **{k: g[k] for k in g.files})


@pytest.fixture(scope = 'module')
def tok():
	from convasr_amd.transcript_generators import CharTokenizerLegacy
	return CharTokenizerLegacy('ab')


def test_golden_file_is_what_its_generator_describes(golden):
	assert golden.lp.shape == (3, 97, 38) and golden.lp.dtype == np.float32 and golden.lengths.tolist() == [97, 61, 1]
	assert np.abs(np.exp(golden.lp.astype(np.float64)).sum(-1) - 1).max() < 1e-5
	# the three utterances are flat, speech-like and saturated: the measures span three orders of magnitude
	assert golden.entropy_frames[0].mean() > 3.0 and golden.entropy_frames[2].mean() < 0.5 and golden.margin[2].mean() > 0.7


def test_frame_restatement_equals_the_reference(golden):
	"""The reference works in fp32: C products of an exp (1 ulp) and a multiply (1/2 ulp), summed in some order (at most C - 1 roundings of
	a partial sum of same-signed terms), so its entropy is within (C + 3) U of the exact one, relatively; a margin is the difference of two
	exps of values <= 1 (U each) and one subtraction (U / 2): 3 U absolute, 4 U allowed."""
	C = golden.lp.shape[-1]
	got = R.frame_uncertainty(golden.lp, eps_id = -1)
	for name, ref, bar in (('entropy', golden.entropy_frames, (C + 3) * U), ('entropy_nb', golden.entropy_no_blank, None)):
		want = ref.astype(np.float64)
		err = np.abs(getattr(got, name) - want)
		if bar is None:
			# log_softmax comes first, in fp32.  Its sum of C - 1 exps in [0, 1] carries up to (C + 1) U relatively, which shifts EVERY log q by
			# that much absolutely: d H = shift * (H - 1).  Every log q is then rounded (U |log q| each, |log q| up to 150 here), which moves the
			# sum by at most sum_c q (1 + |log q|) U |log q|; a factor 2 for the second-order terms.
			lq = golden.lp[..., :-1].astype(np.float64)
			lq = lq - np.log(np.exp(lq).sum(-1, keepdims = True))
			tol = (C + 3) * U * want + (C + 1) * U * np.abs(want - 1) + 2 * U * (np.exp(lq) * (1 + np.abs(lq)) * np.abs(lq)).sum(-1)
		else:
			tol = bar * want
		print(f'{name}: worst error / bar {float((err / tol).max()):.3f}')
		assert (err <= tol).all(), name
	err = np.abs(got.margin - golden.margin.astype(np.float64))
	print(f'margin: worst error {float(err.max()) / U:.2f} U, bar 4 U')
	assert err.max() <= 4 * U
	masked = R.frame_uncertainty(golden.lp, eps_id = -1, lengths = golden.lengths)
	live = np.arange(97)[None] < golden.lengths[:, None]
	assert (masked.entropy[~live] == 0).all() and (golden.entropy_frames_masked[~live] == 0).all()
	assert np.array_equal(masked.entropy[live], got.entropy[live]) and np.array_equal(masked.idx, got.idx)
	assert np.array_equal(got.idx, golden.lp.argmax(-1))


def test_whole_utterance_spans_equal_the_reference(golden):
	"""A span over [0, n) is the utterance: its uncertainty is models.weighted_mean_entropy and its entropy models.entropy with lengths (up to
	that function's eps / n, below 1e-9).  The reference's fp32: per-frame entropies as above, T of them summed, one division -- (C + T + 5) U
	relative for the entropy; the weighted form is held to the project's weighted-entropy bar (2e-5, 1e-6)."""
	C, T = golden.lp.shape[-1], golden.lp.shape[1]
	stats = R.frame_uncertainty(golden.lp, eps_id = -1, lengths = golden.lengths)
	n = golden.lengths
	got = R.span_uncertainty(golden.lp, stats, [0, 1, 2], [0, 0, 0], (n - 1).tolist())
	want_e, want_u = golden.entropy.astype(np.float64), golden.weighted_mean_entropy.astype(np.float64)
	err_e, err_u = np.abs(got.entropy - want_e), np.abs(got.uncertainty - want_u)
	print('entropy error / bar', (err_e / ((C + T + 5) * U * want_e + 1e-9)).max(), 'uncertainty error / bar', (err_u / (2e-5 * want_u + 1e-6)).max())
	assert (err_e <= (C + T + 5) * U * want_e + 1e-9).all()
	assert (err_u <= 2e-5 * want_u + 1e-6).all()
	everything = R.span_uncertainty(golden.lp, R.frame_uncertainty(golden.lp), [0, 1, 2], [0] * 3, [T - 1] * 3)
	assert np.abs(everything.entropy - golden.entropy_all_frames).max() <= (C + T + 5) * U * golden.entropy_all_frames.max()


@pytest.mark.parametrize('C', [2, 3, 38, 65])
def test_vectorised_frame_restatement_equals_the_class_by_class_loop(C):
	rng = np.random.default_rng(C)
	x = R.special_frames(rng, C)
	for eps_id, lengths in ((-1, None), (0, [12, 5, 0]), (C // 2, [0, 12, 1])):
		a, b = R.frame_uncertainty(x, eps_id, lengths), R.frame_uncertainty_loop(x, eps_id, lengths)
		assert np.array_equal(a.idx, b.idx)
		for k in ('p1', 'p2', 'margin', 'entropy', 'entropy_nb', 'p_eps'):
			va, vb = getattr(a, k), getattr(b, k)
			assert np.array_equal(np.isnan(va), np.isnan(vb)), (k, eps_id)
			assert np.allclose(va, vb, rtol = 1e-12, atol = 1e-14, equal_nan = True), (k, eps_id)
	full = R.frame_uncertainty(x, -1)
	assert full.idx[0, 1] == 0 and full.margin[0, 1] == 0 and full.idx[0, 2] == 0 and full.margin[0, 2] == 0  # ties: the lower index, margin exactly 0
	assert full.idx[0, 3] == C - 1 and full.idx[0, 4] == 0 and full.idx[1, 2] == 0  # NaN above every number, +inf included; the first NaN
	assert all(np.isnan(getattr(full, k)[0, 3]) for k in ('p1', 'margin', 'entropy', 'entropy_nb', 'p_eps'))
	assert np.isnan(full.entropy[1, 0]) and np.isfinite(full.p1[1, 0]) and np.isfinite(full.margin[1, 0])  # a class at -inf: 0 * inf in the entropy alone
	if C == 2:
		assert (full.entropy_nb[2] == 0).all() and not np.signbit(full.entropy_nb[2]).any()


def _random_spans(rng, B, T, C, N, with_path):
	"""N random spans with events at random frames inside them; some events doubled, some whose token is not the path's."""
	lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32)) * 3, -1).numpy()
	path = lp.argmax(-1)
	utt, begin, end, first, tokens, frames = [], [], [], [0], [], []
	for k in range(N):
		u, b = int(rng.integers(B)), int(rng.integers(T))
		e = min(T - 1, b + int(rng.integers(0, 40)))
		utt.append(u); begin.append(b); end.append(e)
		for f in sorted(rng.integers(b, e + 1, int(rng.integers(0, 6))).tolist()):
			tk = int(path[u, f]) if rng.random() < 0.7 else int(rng.integers(C))
			tokens.append(tk); frames.append(f)
			if rng.random() < 0.2:
				tokens.append(tk); frames.append(f)
		first.append(len(tokens))
	return lp, (path if with_path else None), types.SimpleNamespace(utt = utt, begin = begin, end = end, first = first, tokens = tokens, frames = frames)


@pytest.mark.parametrize('with_path', [False, True])
def test_span_restatement_equals_a_scalar_loop(with_path):
	rng = np.random.default_rng(7 + with_path)
	B, T, C, N = 3, 120, 6, 200
	lp, path, s = _random_spans(rng, B, T, C, N, with_path)
	stats = R.frame_uncertainty(lp, eps_id = -1, lengths = [T, T - 7, T // 2])
	got = R.span_uncertainty(lp, stats, s.utt, s.begin, s.end, s.first, s.tokens, s.frames, path = path)
	seen_zero = seen_negative = 0
	for k in range(N):
		u = s.utt[k]
		sh = num = den = 0.0
		for t in range(s.begin[k], s.end[k] + 1):
			h, w = float(stats.entropy[u, t]), 1.0 - float(stats.p_eps[u, t])
			sh += h; num += h * w; den += w
		ls, ms = [], []
		for j in range(s.first[k], s.first[k + 1]):
			tk, f = s.tokens[j], s.frames[j]
			if j > s.first[k] and (s.tokens[j - 1], s.frames[j - 1]) == (tk, f):
				continue
			if path is not None and path[u, f] != tk:
				continue
			l = float(lp[u, f, tk])
			ls.append(l)
			ms.append(float(stats.margin[u, f]) if stats.idx[u, f] == tk else math.exp(l) - float(stats.p1[u, f]))
		want = dict(entropy = sh / (s.end[k] - s.begin[k] + 1), uncertainty = num / (float(np.float32(1e-9)) + den), confidence = math.exp(sum(ls) / len(ls)) if ls else 0.0,
		            confidence_min = math.exp(min(ls)) if ls else 0.0, margin = min(ms) if ms else 0.0)
		assert got.n_events[k] == len(ls)
		for name, v in want.items():
			assert abs(getattr(got, name)[k] - v) <= 1e-12 * max(1.0, abs(v)), (k, name)
		seen_zero += not ls
		seen_negative += bool(ms) and min(ms) < 0
	assert seen_zero > 5 and (with_path or seen_negative > 5)
	only_frames = R.span_uncertainty(lp, stats, s.utt, s.begin, s.end)
	assert np.array_equal(only_frames.entropy, got.entropy) and np.array_equal(only_frames.uncertainty, got.uncertainty)


def test_skip_rules_on_hand_written_events(tok):
	"""'a|||b  a' with blank_amount_to_space = 3: the greedy rule emits a, an INSERTED space at the third blank, b, then the space of the
	path twice (it opens the second word), a."""
	eps, space, a, b = tok.eps_id, tok.space_id, 0, 1
	path = [a, eps, eps, eps, b, space, space, a]
	tokens, frames, segments = G.greedy_segments(path, len(path), eps, space, 3)
	assert tokens == [a, space, b, space, space, a] and frames == [0, 3, 4, 5, 5, 7] and segments == [(0, 0, 4), (3, 5, 7)]
	T, C = len(path), tok.vocab_size
	lp = np.full((1, T, C), math.log(0.02), np.float32)
	for t, c in enumerate(path):
		lp[0, t, c] = math.log(0.5 + 0.05 * t)
	stats = R.frame_uncertainty(lp, eps_id = eps)
	spans = dict(utt = [0, 0], begin = [0, 5], end = [4, 7], first = [0, 3, 6], tokens = tokens, frames = frames)
	with_path = R.span_uncertainty(lp, stats, path = [path], **spans)
	assert with_path.n_events.tolist() == [2, 2]  # word 0: a and b (the inserted space is skipped); word 1: the space ONCE, and a
	p = lambda t: 0.5 + 0.05 * t
	assert np.allclose(with_path.confidence, [math.sqrt(p(0) * p(4)), math.sqrt(p(5) * p(7))], rtol = 1e-6)
	assert np.allclose(with_path.confidence_min, [p(0), p(5)], rtol = 1e-6)
	assert np.allclose(with_path.margin, [p(0) - 0.02, p(5) - 0.02], rtol = 1e-6)
	without = R.span_uncertainty(lp, stats, **spans)
	assert without.n_events.tolist() == [3, 2]  # no path: the inserted space counts, at the blank's frame, where space has probability 0.02
	assert np.allclose(without.confidence_min, [0.02, p(5)], rtol = 1e-6) and np.allclose(without.margin, [0.02 - p(3), p(5) - 0.02], rtol = 1e-6)
	# a span whose only event is an inserted space, and one without events: n = 0, the three event outputs are 0, the frame outputs are not
	empty = R.span_uncertainty(lp, stats, [0, 0], [3, 1], [3, 2], [0, 1, 1], [space], [3], path = [path])
	assert empty.n_events.tolist() == [0, 0] and not empty.confidence.any() and not empty.confidence_min.any() and not empty.margin.any()
	assert (empty.entropy > 0).all() and (empty.uncertainty > 0).all()
	# three identical events in a row count once
	triple = R.span_uncertainty(lp, stats, [0], [0], [7], [0, 3], [a, a, a], [0, 0, 0])
	assert triple.n_events.tolist() == [1]


def test_frame_map_moves_the_events_after_the_skip_rules(tok):
	"""Positions on a transcript's grid: rule (a) and (b) look at the positions, the statistics at the mapped frames."""
	rng = np.random.default_rng(3)
	lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((1, 30, 5)).astype(np.float32)) * 2, -1).numpy()
	stats = R.frame_uncertainty(lp, eps_id = 4)
	fmap = [[2, 2, 9, 17, 29]]
	path = [[0, 1, 1, 3, 2]]
	got = R.span_uncertainty(lp, stats, [0], [0], [3], [0, 4], [0, 1, 1, 3], [0, 1, 2, 3], path = path, frame_map = fmap)
	assert got.n_events.tolist() == [4]  # positions 1 and 2 differ, whatever they map to; 0 and 1 both map to frame 2
	ls = [lp[0, 2, 0], lp[0, 2, 1], lp[0, 9, 1], lp[0, 17, 3]]
	assert np.isclose(got.confidence[0], math.exp(np.mean(np.float64(ls)))) and np.isclose(got.entropy[0], stats.entropy[0, 2:18].mean())
	assert R.span_envelope(1, 1, 30, 5, Tp = 5, frame_map = True) == 0 and R.span_envelope(1, 1, 30, 5, Tp = 5) == R.EINVAL


def test_spans_of_the_host_loop_are_the_restated_segments(tok):
	"""With time_stamps = arange(T) and begin = 0 the host loop's begin / end ARE frames: they equal the restated seg_begin / seg_end, and
	the events that count per word are the characters of its text minus the doubled word-start space and the inserted spaces."""
	from convasr_amd.transcript_generators import GreedyCTCGenerator
	rng = random.Random(5)
	eps, space = tok.eps_id, tok.space_id
	B, T, bats = 24, 150, 3
	paths = []
	for _ in range(B):
		p = []
		while len(p) < T:
			p += [rng.choice((eps, eps, space, rng.randrange(3), rng.randrange(3)))] * rng.randint(1, 6)
		paths.append(p[:T])
	lengths = [rng.choice((T, T, rng.randint(0, T))) for _ in range(B)]
	lp = torch.nn.functional.one_hot(torch.tensor(paths), tok.vocab_size).permute(0, 2, 1).float()
	ts = torch.arange(T, dtype = torch.float32).expand(B, -1)
	host = GreedyCTCGenerator(bats).generate_host(tok, lp, torch.zeros(B), torch.ones(B), output_lengths = torch.tensor(lengths), time_stamps = ts)
	s = R.greedy_spans(paths, lengths, eps, space, bats)
	words = [seg for alternatives in host for seg in alternatives[0]]
	assert len(words) == len(s.utt) > 100
	assert [int(w['begin']) for w in words] == s.begin and [int(w['end']) for w in words] == s.end
	assert s.utt == [b for b, alternatives in enumerate(host) for _ in alternatives[0]]
	x = np.log(np.full((B, T, tok.vocab_size), 0.01, np.float32))
	got = R.span_uncertainty(x, R.frame_uncertainty(x, eps), s.utt, s.begin, s.end, s.first, s.tokens, s.frames, path = paths)
	inserted = doubled = 0
	for k, w in enumerate(words):
		ev = list(zip(s.tokens[s.first[k]:s.first[k + 1]], s.frames[s.first[k]:s.first[k + 1]]))
		assert tok.decode([[c for c, _ in ev]])[0] == w['hyp']
		ins = sum(paths[s.utt[k]][f] == eps for c, f in ev)
		dbl = int(len(ev) > 1 and ev[0] == ev[1])
		assert got.n_events[k] == len(w['hyp']) - ins - dbl and (not dbl or ev[0][0] == space)
		inserted += ins
		doubled += dbl
	assert inserted > 20 and doubled > 20


def test_envelope_of_both_calls():
	from convasr_amd import _lib
	lib = _lib.load()
	assert 1 <= lib.convasr_frame_uncertainty_row_classes() <= 64

	def frame(B = 2, T = 10, C = 38, eps_id = 37, lp = P, lengths = None, idx = P, out = P):
		return lib.convasr_frame_uncertainty(lp, lengths, idx, out, out, out, out, out, B, T, C, eps_id, None)

	for bad in (dict(B = 0), dict(T = 0), dict(B = -1), dict(B = 1 << 16, T = 1 << 15), dict(C = 1), dict(C = 0), dict(C = 8193), dict(eps_id = -1), dict(eps_id = 38),
	            dict(C = 2, eps_id = 2), dict(lp = None)):
		rc = frame(**bad)
		assert rc == R.EINVAL and b'frame_uncertainty' in lib.convasr_last_error(), (bad, rc)
		sizes = dict(dict(B = 2, T = 10, C = 38, eps_id = 37), **{k: v for k, v in bad.items() if k != 'lp'})
		assert R.frame_envelope(**sizes) == R.EINVAL or 'lp' in bad, bad
	assert R.frame_envelope(2, 10, 38, 37) == 0 and R.frame_envelope(1, (1 << 31) - 1, 8192, 0) == 0 and R.frame_envelope(1, 1, 2, 1) == 0

	def span(N = 3, B = 2, T = 10, C = 38, eps = 1e-9, Tp = 10, n_events = 5, lp = P, stats = P, ent = P, utt = P, begin = P, end = P, first = P, tokens = P, frames = P, path = None,
	         fmap = None, n_out = P, conf = P, out = P):
		return lib.convasr_span_uncertainty(lp, stats, stats, stats, ent, ent, utt, begin, end, first, tokens, frames, n_events, path, fmap, Tp, n_out, conf, conf, conf, out, out,
		                                    N, B, T, C, eps, None)

	for bad in (dict(N = 0), dict(N = -1), dict(N = 1 << 31), dict(B = 0), dict(T = 0), dict(B = 1 << 16, T = 1 << 15, Tp = 1 << 15), dict(C = 1), dict(C = 8193), dict(eps = -1.0),
	            dict(Tp = 7), dict(Tp = 0, fmap = P), dict(B = 1 << 16, Tp = 1 << 15, fmap = P), dict(n_events = -1), dict(ent = None), dict(utt = None), dict(begin = None),
	            dict(end = None), dict(out = None), dict(first = None), dict(tokens = None), dict(frames = None), dict(lp = None), dict(stats = None), dict(n_out = None),
	            dict(conf = None), dict(first = None, tokens = None, frames = None, path = P)):
		rc = span(**bad)
		assert rc == R.EINVAL and b'span_uncertainty' in lib.convasr_last_error(), (bad, rc)
	assert R.span_envelope(0, 2, 10, 38) == R.EINVAL and R.span_envelope(1 << 31, 2, 10, 38) == R.EINVAL and R.span_envelope(3, 2, 10, 38, eps = -1.0) == R.EINVAL
	assert R.span_envelope(3, 2, 10, 38, Tp = 7) == R.EINVAL and R.span_envelope(3, 2, 10, 38, events = False, path = True) == R.EINVAL and R.span_envelope(3, 2, 10, 38) == 0


def test_models_surface_refuses_what_it_does_not_implement():
	from convasr_amd import models, _lib
	x = torch.zeros(1, 4, 5)
	for call in (lambda: models.entropy(x, dim = 2, sum = False), lambda: models.entropy(x, sum = False, keepdim = True), lambda: models.margin(x, dim = 2), lambda: models.margin(x[0])):
		with pytest.raises(_lib.ConvasrHipError):
			call()
	with pytest.raises(Exception):  # a CPU tensor: there is no host path
		models.entropy(x, sum = False)
