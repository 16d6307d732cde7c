"""Word confidence and per-frame uncertainty on the MI355X: ops.frame_uncertainty and ops.span_uncertainty against the float64 restatement
of their rule (tests/_uncertainty_ref.py) on the same fp32 log-probs, on shapes on both sides of the frame pass's two mappings and around
the span pass's 64-lane and 256-thread steps; the generators, transcribe_batch and the models surface on top of them.

Bars (U = 2^-24), each printed next to what was measured:
  integers (idx, n_events)                      exact
  entropy, entropy_nb (frame and span)          the project's entropy bar, rtol 1e-4 + atol 1e-5
  uncertainty                                   the project's weighted-entropy bar, rtol 2e-5 + atol 1e-6, on spans that hold a frame whose argmax
                                                is not the blank (weight sum >= 0.5); a span of pure blank frames: finite and bit-equal only
  p1, p_eps, margin, confidence_min             atol 8 U: two expf of values <= 1, each taken to be within 2 ulp, one subtraction (measured on the MI355X: at most 0.15 of it)
  confidence                                    relative (n + 1) U mean|l_j| + 4 U: a mean of n terms in fp32 (the kernel's is fp64), then one expf"""
import ctypes
import json
import os
import random
import types

import numpy as np
import pytest
import torch

import _uncertainty_ref as R

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
ENTROPY_BAR, WEIGHTED_BAR, PROB_ATOL = (1e-4, 1e-5), (2e-5, 1e-6), 8 * U
FRAME_FLOATS = ('p1', 'margin', 'entropy', 'entropy_nb', 'p_eps')
SPAN_FLOATS = ('confidence', 'confidence_min', 'margin', 'entropy', 'uncertainty')
ROOT = os.path.dirname(os.path.abspath(__file__))


def _dev():
	return torch.device('cuda:0')


def _to_dev(lp):
	"""(B, T, C) numpy log-probs -> the (B, C, T) channels-last device tensor the model would hand over."""
	return torch.from_numpy(lp).to(_dev()).permute(0, 2, 1)


def _held(name, got, want, rtol, atol, where = None):
	"""|got - want| <= atol + rtol |want| at every entry (where: a mask of the entries that are held); prints the worst use of the bar."""
	got, want = np.asarray(got, dtype = np.float64), np.asarray(want, dtype = np.float64)
	assert got.shape == want.shape, (name, got.shape, want.shape)
	assert np.array_equal(np.isnan(got), np.isnan(want)), f'{name}: NaN positions differ'
	ok = ~np.isnan(want) if where is None else (~np.isnan(want) & where)
	if not ok.any():
		return 0.0
	use = float((np.abs(got - want)[ok] / (atol + rtol * np.abs(want[ok]))).max())
	print(f'  {name}: worst error {float(np.abs(got - want)[ok].max()):.3e}, {use:.3f} of its bar (rtol {rtol:g}, atol {atol:.3g})')
	assert use <= 1.0, (name, use)
	return use


def _frame_check(got, want, what):
	assert np.array_equal(got.idx.cpu().numpy(), want.idx), what
	print(what)
	for name in FRAME_FLOATS:
		rtol, atol = ENTROPY_BAR if name.startswith('entropy') else (0.0, PROB_ATOL)
		_held(name, getattr(got, name).cpu().numpy(), getattr(want, name), rtol, atol)


def _bit_equal(a, b, names):
	for name in names:
		x, y = getattr(a, name), getattr(b, name)
		assert (x is None and y is None) or torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), name


# ------------------------------------------------------------------------------------------------ frame pass

@pytest.mark.parametrize('C, T', [(2, 1), (3, 65), (38, 211), (64, 32), (65, 64), (129, 63), (257, 5)])
def test_frame_pass(C, T):
	from convasr_amd import ops
	assert ops.frame_uncertainty_row_classes() == 64  # (64, 32) and (65, 64) sit on either side of the two mappings
	rng = np.random.default_rng(1000 * C + T)
	B = 3
	for scale in (0.5, 3.0, 12.0):
		lp = R.log_softmax32(rng.standard_normal((B, T, C)) * scale)
		x = _to_dev(lp)
		arg = ops.argmax(x)
		for lengths in (None, [0, 1, T - 1], [T, T - 1, 1]):
			for eps_id in (-1, 0):
				got = ops.frame_uncertainty(x, eps_id, None if lengths is None else torch.tensor(lengths))
				assert torch.equal(got.idx, arg) and got.idx.dtype == torch.int64 and all(getattr(got, k).shape == (B, T) for k in FRAME_FLOATS)
				_frame_check(got, R.frame_uncertainty(lp, eps_id, lengths), f'C {C} T {T} scale {scale} lengths {lengths} eps_id {eps_id}')
				if C == 2:
					assert not got.entropy_nb.any()
		once, again = (ops.frame_uncertainty(x, -1, torch.tensor([T, T - 1, 1])) for _ in range(2))
		_bit_equal(once, again, ('idx', ) + FRAME_FLOATS)
		contiguous = x.contiguous()  # torch-contiguous (B, C, T): the op converts it
		assert not ops.is_cl(contiguous) or T == 1
		_bit_equal(ops.frame_uncertainty(contiguous, -1, torch.tensor([T, T - 1, 1])), once, ('idx', ) + FRAME_FLOATS)


@pytest.mark.parametrize('C', [2, 3, 38, 64, 65, 129])
def test_frame_pass_ties_nan_and_infinities(C):
	from convasr_amd import ops
	lp = R.special_frames(np.random.default_rng(C), C)
	x = _to_dev(lp)
	for eps_id, lengths in ((-1, None), (0, [12, 5, 0])):
		got = ops.frame_uncertainty(x, eps_id, None if lengths is None else torch.tensor(lengths))
		assert torch.equal(got.idx, ops.argmax(x))
		_frame_check(got, R.frame_uncertainty(lp, eps_id, lengths), f'C {C} special frames, eps_id {eps_id} lengths {lengths}')
	got = ops.frame_uncertainty(x)
	assert got.idx[0, 1] == 0 and got.margin[0, 1] == 0 and got.idx[0, 2] == 0 and got.margin[0, 2] == 0  # exact ties: the lower index, margin exactly 0
	assert got.idx[0, 3] == C - 1 and got.idx[0, 4] == 0 and got.idx[1, 2] == 0
	assert all(bool(torch.isnan(getattr(got, k)[0, 3])) for k in FRAME_FLOATS) and bool(torch.isnan(got.entropy[1, 0])) and bool(torch.isfinite(got.p1[1, 0]))
	_bit_equal(got, ops.frame_uncertainty(x), ('idx', ) + FRAME_FLOATS)


def test_frame_pass_many_workgroups_and_a_batch_offset():
	"""(5, 1031, 38): 41 workgroups of the row mapping, the last one partial, utterance boundaries inside workgroups; and a view that starts
	at utterance 1 (its base is only 8-byte aligned)."""
	from convasr_amd import ops
	rng = np.random.default_rng(9)
	lp = R.log_softmax32(rng.standard_normal((5, 1031, 38)) * 3)
	x, lengths = _to_dev(lp), [1031, 0, 517, 1030, 1]
	_frame_check(ops.frame_uncertainty(x, -1, torch.tensor(lengths)), R.frame_uncertainty(lp, -1, lengths), '5 x 1031 x 38')
	_frame_check(ops.frame_uncertainty(x[1:], -1, torch.tensor(lengths[1:])), R.frame_uncertainty(lp[1:], -1, lengths[1:]), 'utterances 1 .. 4 of it')


def test_models_surface_equals_the_reference_golden():
	"""models.entropy(sum = False), models.margin and the per-utterance forms on tests/golden/uncertainty.npz: the reference's own fp32 numbers."""
	from convasr_amd import models, ops
	g = np.load(os.path.join(ROOT, 'golden', 'uncertainty.npz'))
	x, n = torch.from_numpy(g['log_probs']).to(_dev()), torch.from_numpy(g['lengths']).to(_dev())
	_held('entropy(sum = False)', models.entropy(x, sum = False).cpu().numpy(), g['entropy_frames'], *ENTROPY_BAR)
	_held('entropy(lengths, sum = False)', models.entropy(x, n, sum = False).cpu().numpy(), g['entropy_frames_masked'], *ENTROPY_BAR)
	_held('margin', models.margin(x).cpu().numpy(), g['margin'], 0.0, PROB_ATOL + 4 * U)  # (the golden's own fp32 rounding: 4 U, tests/test_uncertainty_ref.py)
	_held('entropy without the blank', ops.frame_uncertainty(x).entropy_nb.cpu().numpy(), g['entropy_no_blank'], *ENTROPY_BAR)
	_held('entropy(lengths)', models.entropy(x, n).cpu().numpy(), g['entropy'], *ENTROPY_BAR)
	_held('weighted_mean_entropy', models.weighted_mean_entropy(x, n).cpu().numpy(), g['weighted_mean_entropy'], *WEIGHTED_BAR)
	with pytest.raises(ca_error()):
		models.entropy(x, dim = 2, sum = False)


def ca_error():
	from convasr_amd import _lib
	return _lib.ConvasrHipError


def test_uncertain_spans():
	from convasr_amd import models, ops
	rng = np.random.default_rng(21)
	scale = np.where(rng.random((3, 400, 1)) < 0.5, 0.3, 8.0)  # runs of flat and of peaked frames
	scale = np.repeat(scale[:, ::8], 8, axis = 1)
	lp = R.log_softmax32(rng.standard_normal((3, 400, 38)) * scale)
	lengths = [400, 123, 0]
	want = R.frame_uncertainty(lp, -1, lengths).entropy
	got = models.uncertain_spans(_to_dev(lp), torch.tensor(lengths), max_entropy = 1.0)
	assert len(got) == 3
	near = 0
	for b in range(3):
		over = want[b] > 1.0
		near += int((np.abs(want[b] - 1.0) < 1.1e-4).sum())  # (the entropy bar at 1.0)
		edges = np.flatnonzero(np.diff(np.concatenate([[0], over.astype(np.int8), [0]])))
		starts, ends = edges[::2], edges[1::2]
		assert got[b][0].tolist() == starts.tolist() and got[b][1].tolist() == (ends - starts).tolist(), b
		assert got[b][0].is_cuda and got[b][0].dtype == torch.int64
	assert near == 0 and len(got[0][0]) > 5 and len(got[2][0]) == 0  # (no entropy close enough to the limit for fp32 to decide otherwise)
	everything = models.uncertain_spans(_to_dev(lp), None, max_entropy = -1.0)
	assert [s.tolist() for s in everything[2]] == [[0], [400]]


# ------------------------------------------------------------------------------------------------ span pass

def _span_inputs():
	"""(3, 700, 6) log-probs, blank = class 5; frames 300 .. 340 of utterance 0 are pure blank.  Spans of 1, 63, 64, 65, 256, 257 frames at
	the start and at the end of every utterance (they overlap), with 0, 1, 64 or 65 events or a few; some events doubled, some tokens not
	the argmax; then random spans up to N = 1,000."""
	rng = np.random.default_rng(77)
	B, T, C = 3, 700, 6
	logits = rng.standard_normal((B, T, C)) * 3
	logits[0, 300:341, 5] += 40
	lp = R.log_softmax32(logits)
	path = lp.argmax(-1)
	spans = []
	for u in range(B):
		for k, n in enumerate((1, 63, 64, 65, 256, 257)):
			spans.append((u, 0, n - 1, (0, 1, 64, 65, 3, 5)[k]))
			spans.append((u, T - n, T - 1, (1, 64, 65, 0, 300, 4)[k]))
	spans.append((0, 305, 335, 3))  # pure blank frames
	while len(spans) < 1000:
		b = int(rng.integers(T))
		spans.append((int(rng.integers(B)), b, min(T - 1, b + int(rng.integers(0, 60))), int(rng.integers(0, 9))))
	utt, begin, end, first, tokens, frames = [], [], [], [0], [], []
	for u, b, e, n_ev in spans:
		utt.append(u); begin.append(b); end.append(e)
		for f in sorted(rng.integers(b, e + 1, n_ev).tolist()):
			tk = int(path[u, f]) if rng.random() < 0.7 else int(rng.integers(C))
			tokens.append(tk); frames.append(f)
			if rng.random() < 0.15:
				tokens.append(tk); frames.append(f)
		first.append(len(tokens))
	return lp, path, types.SimpleNamespace(utt = utt, begin = begin, end = end, first = first, tokens = tokens, frames = frames), 36


def _span_check(got, want, lp, s, path, held_weighted, what):
	print(what)
	assert np.array_equal(got.n_events.cpu().numpy(), want.n_events)
	n = want.n_events.astype(np.float64)
	mean_abs = R.span_mean_abs_l(lp, s.utt, s.first, s.tokens, s.frames, path)
	conf, conf_want = got.confidence.cpu().numpy().astype(np.float64), want.confidence
	use = np.abs(conf - conf_want) / (conf_want * ((n + 1) * U * mean_abs + 4 * U) + (n == 0))
	print(f'  confidence: {float(use.max()):.3f} of its bar')
	assert use.max() <= 1.0 and not conf[n == 0].any()
	_held('confidence_min', got.confidence_min.cpu().numpy(), want.confidence_min, 0.0, PROB_ATOL)
	_held('margin', got.margin.cpu().numpy(), want.margin, 0.0, PROB_ATOL)
	_held('entropy', got.entropy.cpu().numpy(), want.entropy, *ENTROPY_BAR)
	_held('uncertainty', got.uncertainty.cpu().numpy(), want.uncertainty, *WEIGHTED_BAR, where = held_weighted)
	assert bool(torch.isfinite(got.uncertainty).all())


def _has_speech(idx, s, eps_id):
	return np.array([bool((idx[u, b:e + 1] != eps_id).any()) for u, b, e in zip(s.utt, s.begin, s.end)])


def test_span_pass():
	from convasr_amd import ops
	lp, path, s, blank_span = _span_inputs()
	x = _to_dev(lp)
	stats, want_stats = ops.frame_uncertainty(x, 5), R.frame_uncertainty(lp, 5)
	held = _has_speech(want_stats.idx, s, 5)
	assert not held[blank_span] and held.sum() > 800
	names = ('n_events', ) + SPAN_FLOATS
	for with_path in (False, True):
		p = path if with_path else None
		got = ops.span_uncertainty(x, stats, s.utt, s.begin, s.end, s.first, s.tokens, s.frames, path = None if p is None else torch.from_numpy(p))
		want = R.span_uncertainty(lp, want_stats, s.utt, s.begin, s.end, s.first, s.tokens, s.frames, path = p)
		_span_check(got, want, lp, s, p, held, f'1,000 spans, path {with_path}')
		assert (want.n_events == 0).sum() > 20 and want.n_events.max() >= 65
		assert (want.margin < 0).sum() == 0 if with_path else (want.margin < 0).sum() > 100  # (with the path only the argmax's own tokens count)
		_bit_equal(got, ops.span_uncertainty(x, stats, s.utt, s.begin, s.end, s.first, s.tokens, s.frames, path = None if p is None else torch.from_numpy(p)), names)
		# a permutation of the spans permutes the outputs; one span alone gives its own row: bit for bit
		perm = np.random.default_rng(5).permutation(len(s.utt))
		first, tokens, frames = [0], [], []
		for k in perm:
			tokens += s.tokens[s.first[k]:s.first[k + 1]]
			frames += s.frames[s.first[k]:s.first[k + 1]]
			first.append(len(tokens))
		take = lambda v: [v[k] for k in perm]
		shuffled = ops.span_uncertainty(x, stats, take(s.utt), take(s.begin), take(s.end), first, tokens, frames, path = None if p is None else torch.from_numpy(p))
		index = torch.from_numpy(perm).to(_dev())
		_bit_equal(shuffled, types.SimpleNamespace(**{k: getattr(got, k)[index] for k in names}), names)
		for k in (0, 9, blank_span, 500):
			lo, hi = s.first[k], s.first[k + 1]
			alone = ops.span_uncertainty(x, stats, [s.utt[k]], [s.begin[k]], [s.end[k]], [0, hi - lo], s.tokens[lo:hi] or [0], s.frames[lo:hi] or [0], path = None if p is None else torch.from_numpy(p))
			_bit_equal(alone, types.SimpleNamespace(**{name: getattr(got, name)[k:k + 1] for name in names}), names)
	frames_only = ops.span_uncertainty(x, stats, s.utt, s.begin, s.end)
	assert frames_only.n_events is None and frames_only.confidence is None
	_bit_equal(frames_only, got, ('entropy', 'uncertainty'))


def test_span_pass_one_long_recording():
	"""One span over 1 x 200,000 frames (split_words = False gives such a segment) with 50,000 events, next to short ones inside it."""
	from convasr_amd import ops
	rng = np.random.default_rng(13)
	T, C = 200000, 6
	lp = R.log_softmax32(rng.standard_normal((1, T, C)) * 3)
	path = lp.argmax(-1)
	ev = np.sort(rng.integers(0, T, 50000))
	s = types.SimpleNamespace(utt = [0, 0, 0], begin = [0, 199000, 0], end = [T - 1, T - 1, 0], first = [0, 50000, 50000, 50000], tokens = path[0, ev].tolist(), frames = ev.tolist())
	x = _to_dev(lp)
	stats, want_stats = ops.frame_uncertainty(x, 5), R.frame_uncertainty(lp, 5)
	_frame_check(stats, want_stats, '1 x 200,000 x 6 frames')
	got = ops.span_uncertainty(x, stats, s.utt, s.begin, s.end, s.first, s.tokens, s.frames, path = torch.from_numpy(path))
	want = R.span_uncertainty(lp, want_stats, s.utt, s.begin, s.end, s.first, s.tokens, s.frames, path = path)
	assert want.n_events[0] > 40000  # (two events at one frame are one doubled event)
	_span_check(got, want, lp, s, path, _has_speech(want_stats.idx, s, 5), 'a span of 200,000 frames')
	_bit_equal(got, ops.span_uncertainty(x, stats, s.utt, s.begin, s.end, s.first, s.tokens, s.frames, path = torch.from_numpy(path)), ('n_events', ) + SPAN_FLOATS)


def test_calls_outside_the_envelope_launch_nothing():
	from convasr_amd import ops, _lib
	lib = _lib.load()
	d = _dev()
	x = _to_dev(R.log_softmax32(np.random.default_rng(0).standard_normal((2, 10, 4))))
	stats = ops.frame_uncertainty(x)
	out = torch.full((6, 2, 10), 7.0, device = d)
	idx = torch.full((2, 10), 7, dtype = torch.int64, device = d)
	p = lambda t: ctypes.c_void_p(t.data_ptr())
	lp = ops.as_cl(x, torch.float32)
	for B, T, C, eps_id in ((0, 10, 4, 3), (2, 0, 4, 3), (2, 10, 1, 0), (2, 10, 8193, 0), (2, 10, 4, 4), (2, 10, 4, -1), (1 << 16, 1 << 15, 4, 0)):
		assert R.frame_envelope(B, T, C, eps_id) == R.EINVAL
		assert lib.convasr_frame_uncertainty(p(lp), None, p(idx), p(out[0]), p(out[1]), p(out[2]), p(out[3]), p(out[4]), B, T, C, eps_id, None) == R.EINVAL
	utt, begin, end = torch.zeros(3, dtype = torch.int64, device = d), torch.zeros(3, dtype = torch.int32, device = d), torch.ones(3, dtype = torch.int32, device = d)
	for N, B, T, C, eps in ((0, 2, 10, 4, 1e-9), (1 << 31, 2, 10, 4, 1e-9), (3, 0, 10, 4, 1e-9), (3, 2, 10, 1, 1e-9), (3, 2, 10, 4, -1.0)):
		assert R.span_envelope(N, B, T, C, eps, events = False) == R.EINVAL
		rc = lib.convasr_span_uncertainty(None, None, None, None, p(stats.entropy), p(stats.p_eps), p(utt), p(begin), p(end), None, None, None, 0, None, None, T, None, None, None, None,
		                                  p(out[0]), p(out[1]), N, B, T, C, eps, None)
		assert rc == R.EINVAL
	torch.cuda.synchronize()
	assert bool((out == 7).all()) and bool((idx == 7).all())
	for call in (lambda: ops.span_uncertainty(x, stats, [], [], []), lambda: ops.frame_uncertainty(x, 4), lambda: ops.frame_uncertainty(x[:, :1])):
		with pytest.raises(_lib.ConvasrHipError):
			call()
	with pytest.raises(ValueError):
		ops.span_uncertainty(x, stats, [0], [0], [1], first = [0, 1])
	# what only the device can see is clamped: spans and events that point outside read nothing out of bounds and equal their clamped selves
	wild = ops.span_uncertainty(x, stats, [5, -3], [-4, 8], [99, 2], [0, 2, 9], [9, -1, 0], [50, -2, 3])
	tame = ops.span_uncertainty(x, stats, [1, 0], [0, 8], [9, 8], [0, 2, 3], [9, -1, 0], [50, -2, 3])
	_bit_equal(wild, tame, ('n_events', ) + SPAN_FLOATS)
	want = R.span_uncertainty(ops.as_cl(x).permute(0, 2, 1).cpu().numpy(), R.frame_uncertainty(ops.as_cl(x).permute(0, 2, 1).cpu().numpy()), [5, -3], [-4, 8], [99, 2], [0, 2, 9], [9, -1, 0], [50, -2, 3])
	assert wild.n_events.tolist() == want.n_events.tolist() == [2, 1]
	_held('clamped confidence_min', wild.confidence_min.cpu().numpy(), want.confidence_min, 0.0, PROB_ATOL)


# ------------------------------------------------------------------------------------------------ generators

def _random_paths(rng, B, T, eps, space, letters):
	paths = []
	for _ in range(B):
		p = []
		while len(p) < T:
			p += [rng.choice((eps, eps, space, rng.randrange(letters), rng.randrange(letters)))] * rng.randint(1, 12)
		paths.append(p[:T])
	return paths


def _log_probs_around(paths, C, seed, scale = 2.0, boost = 4.0):
	"""Random log-probs whose frames lean towards the given paths (the decoded path is their argmax, wherever it falls)."""
	rng = np.random.default_rng(seed)
	logits = rng.standard_normal((len(paths), len(paths[0]), C)) * scale
	np.put_along_axis(logits, np.asarray(paths)[..., None], np.take_along_axis(logits, np.asarray(paths)[..., None], -1) + boost, -1)
	return R.log_softmax32(logits)


def _strip(result):
	from convasr_amd.transcript_generators import UNCERTAINTY_KEYS
	return [[[{k: v for k, v in seg.items() if k not in UNCERTAINTY_KEYS} for seg in alt] for alt in alternatives] for alternatives in result]


def _fields_check(segments, want, lp, s, path, what, frame_map = None, held_weighted = None):
	"""The five fields of the generator's segments (in span order) against the restatement's spans."""
	print(what)
	assert len(segments) == len(s.utt) > 0
	got = {k: np.array([seg[k] for seg in segments]) for k in SPAN_FLOATS}
	assert all(type(seg[k]) is float for seg in segments for k in SPAN_FLOATS)
	n = want.n_events.astype(np.float64)
	mean_abs = R.span_mean_abs_l(lp, s.utt, s.first, s.tokens, s.frames, path, frame_map)
	use = np.abs(got['confidence'] - want.confidence) / (want.confidence * ((n + 1) * U * mean_abs + 4 * U) + (n == 0))
	print(f'  confidence: {float(use.max()):.3f} of its bar')
	assert use.max() <= 1.0
	_held('confidence_min', got['confidence_min'], want.confidence_min, 0.0, PROB_ATOL)
	_held('margin', got['margin'], want.margin, 0.0, PROB_ATOL)
	_held('entropy', got['entropy'], want.entropy, *ENTROPY_BAR)
	_held('uncertainty', got['uncertainty'], want.uncertainty, *WEIGHTED_BAR, where = held_weighted)


def _greedy_case(tok, B, T, lengths, seed, bats = 10):
	from convasr_amd.transcript_generators import GreedyCTCGenerator
	from convasr_amd import ops
	d = _dev()
	rng = random.Random(seed)
	C, eps, space = tok.vocab_size, tok.eps_id, tok.space_id
	lp = _log_probs_around(_random_paths(rng, B, T, eps, space, C - 5), C, seed)
	x = _to_dev(lp)
	path = lp.argmax(-1)
	begin, end, olen = torch.zeros(B, device = d), torch.full((B, ), 9.0, device = d), torch.tensor(lengths, device = d)
	ts = torch.arange(T, dtype = torch.float32, device = d).expand(B, -1)
	gen = GreedyCTCGenerator(bats)
	calls = []
	real_frame, real_argmax = ops.frame_uncertainty, ops.argmax
	ops.frame_uncertainty = lambda *a, **k: calls.append('frame') or real_frame(*a, **k)
	ops.argmax = lambda *a, **k: calls.append('argmax') or real_argmax(*a, **k)
	try:
		with_fields = gen.generate(tok, x, begin, end, output_lengths = olen, time_stamps = ts, uncertainty = True)
		single = gen.generate(tok, x, begin, end, output_lengths = olen, uncertainty = True)
	finally:
		ops.frame_uncertainty, ops.argmax = real_frame, real_argmax
	assert calls == ['frame', 'frame']  # one pass per call, and its idx in place of ops.argmax
	plain = gen.generate(tok, x, begin, end, output_lengths = olen, time_stamps = ts)
	host = gen.generate_host(tok, x, begin, end, output_lengths = olen, time_stamps = ts)
	assert _strip(with_fields) == plain == host and _strip(single) == gen.generate(tok, x, begin, end, output_lengths = olen)
	assert not any(k in seg for alternatives in plain for seg in alternatives[0] for k in SPAN_FLOATS)
	stats = R.frame_uncertainty(lp, eps, lengths)
	assert np.array_equal(stats.idx, path)
	for result, split in ((with_fields, True), (single, False)):
		s = R.greedy_spans(path.tolist(), lengths, eps, space, bats, split)
		words = [seg for alternatives in result for seg in alternatives[0]]
		if split:  # the host loop's segments ARE these spans: its stamps are the frames
			host_words = [seg for alternatives in host for seg in alternatives[0]]
			assert [int(w['begin']) for w in host_words] == s.begin and [int(w['end']) for w in host_words] == s.end
		want = R.span_uncertainty(lp, stats, s.utt, s.begin, s.end, s.first, s.tokens, s.frames, path = path)
		_fields_check(words, want, lp, s, path, f'greedy {B} x {T}, split_words {split}: {len(words)} segments')
	return len([seg for alternatives in with_fields for seg in alternatives[0]])


def test_greedy_generator_64_x_753():
	from convasr_amd.transcript_generators import CharTokenizerLegacy
	tok = CharTokenizerLegacy('абвгдеёжзийклмнопрстуфхцчшщъыьэюя')
	assert tok.vocab_size == 38
	rng = random.Random(3)
	lengths = [753, 0, 1, 752] + [rng.randint(100, 753) for _ in range(60)]
	assert _greedy_case(tok, 64, 753, lengths, seed = 31) > 1000


def test_greedy_generator_one_long_recording():
	from convasr_amd.transcript_generators import CharTokenizerLegacy
	assert _greedy_case(CharTokenizerLegacy('ab'), 1, 200000, [199990], seed = 32) > 1000


def test_host_route_refuses_uncertainty():
	from convasr_amd.transcript_generators import CharTokenizerLegacy, GreedyCTCGenerator
	tok = CharTokenizerLegacy('ab')
	lp = torch.log_softmax(torch.randn(2, tok.vocab_size, 30, generator = torch.Generator().manual_seed(0)), 1)
	begin, end, ts = torch.zeros(2), torch.ones(2), torch.arange(30.).expand(2, -1)
	gen = GreedyCTCGenerator(3)
	with pytest.raises(ca_error(), match = 'device_route'):
		gen.generate(tok, lp, begin, end, None, ts, uncertainty = True)  # CPU log-probs
	with pytest.raises(ca_error(), match = 'device_route'):
		gen.generate(tok, lp.to(_dev()), begin, end, [30, 20], ts, uncertainty = True)  # lengths as a list
	assert gen.generate(tok, lp, begin, end, None, ts) == gen.generate_host(tok, lp, begin, end, None, ts)
	assert gen.generate(tok, lp.to(_dev()), begin, end, None, ts, uncertainty = False) == gen.generate_host(tok, lp, begin, end, None, ts)


def test_beam_generator():
	"""W = 16, top 2: the spans are rebuilt here from the decoder's tokens and offsets as the generator's host loop cuts them."""
	from convasr_amd.transcript_generators import BeamCTCGenerator, CharTokenizerLegacy
	tok = CharTokenizerLegacy('ab')
	d = _dev()
	B, T, C, eps = 6, 120, tok.vocab_size, tok.eps_id
	rng = random.Random(8)
	lp = _log_probs_around(_random_paths(rng, B, T, eps, tok.space_id, 2), C, 41, scale = 1.5, boost = 2.5)
	x = _to_dev(lp)
	lengths = [120, 119, 64, 1, 90, 77]
	begin, end, olen = torch.zeros(B, device = d), torch.full((B, ), 9.0, device = d), torch.tensor(lengths, device = d)
	ts = torch.arange(T, dtype = torch.float32, device = d).expand(B, -1)
	gen = BeamCTCGenerator(beam_width = 16, topk = 2)
	stats = R.frame_uncertainty(lp, eps, lengths)
	tokens, offsets, lens, _ = gen.decoder(tok).decode_with_scores(x, olen)
	tokens, offsets, lens = tokens.cpu().tolist(), offsets.cpu().tolist(), lens.cpu().tolist()
	for stamps in (ts, None):
		got = gen.generate(tok, x, begin, end, output_lengths = olen, time_stamps = stamps, uncertainty = True)
		assert _strip(got) == gen.generate(tok, x, begin, end, output_lengths = olen, time_stamps = stamps)
		s = types.SimpleNamespace(utt = [], begin = [], end = [], first = [0], tokens = [], frames = [])
		for i in range(B):
			for k in range(2):
				toks, offs = tokens[i][k][:lens[i][k]], offsets[i][k][:lens[i][k]]
				start = next((j for j, c in enumerate(toks) if c not in tok.silence_tokens_ids), len(toks))
				cuts = [start] + [j for j in range(start + 1, len(toks)) if stamps is not None and toks[j] == tok.space_id] + [len(toks)]
				for lo, hi in zip(cuts[:-1], cuts[1:]):
					if hi > lo:
						s.utt.append(i); s.begin.append(offs[lo]); s.end.append(offs[hi - 1])
						s.tokens += toks[lo:hi]; s.frames += offs[lo:hi]
						s.first.append(len(s.tokens))
		words = [seg for alternatives in got for alt in alternatives for seg in alt]
		if stamps is not None:
			assert [int(w['begin']) for w in words] == s.begin and [int(w['end']) for w in words] == s.end
		want = R.span_uncertainty(lp, stats, s.utt, s.begin, s.end, s.first, s.tokens, s.frames)
		_fields_check(words, want, lp, s, None, f'beam search, W 16, top 2, time stamps {stamps is not None}: {len(words)} segments')
		assert stamps is None or (want.margin < 0).any()  # a beam's token need not be its frame's argmax


def test_transcribe_batch_with_uncertainty_and_align():
	"""tests/golden/transcribe.npz through transcribe_batch with args.uncertainty and args.align: strings, segments and alignment are what they
	are without the flag; hyp and ref segments carry the five fields; the ref words' fields are the restatement's over the aligned frames."""
	import convasr_amd as ca
	from convasr_amd.transcript_generators import UNCERTAINTY_KEYS
	g = np.load(os.path.join(ROOT, 'golden', 'transcribe.npz'))
	j = json.load(open(os.path.join(ROOT, 'golden', 'transcribe.json')))
	T_ = lambda a: torch.as_tensor(np.asarray(a))
	sd = {k[3:]: T_(g[k]) for k in g.files if k.startswith('sd/')}
	ckpt_args = dict(j['args'], alphabet = j['alphabet'], model_kwargs = dict(base_width = 32, kernel_sizes = [11], out_width_factors = [2], dropouts = [0.2], out_width_factors_large = [2, 2], residual = False, repeat = 1, nonlinearity = ('hardtanh', 0, 20), dilation = 2))
	args = types.SimpleNamespace(checkpoint = dict(args = dict(ckpt_args), model_state_dict = {k: v.clone() for k, v in sd.items()}), device = 'cuda:0', fp16 = None, frontend_in_model = True, model = None, align = True)
	try:
		text_pipeline, frontend, model, generator = ca.transcribe.setup(args)
		run = lambda: ca.transcribe.transcribe_batch(args, text_pipeline, model, generator, T_(g['wav']).unsqueeze(1), T_(g['xlen']), T_(g['begin']), T_(g['end']), y = T_(g['y']), ylen = T_(g['ylen']), segment_extra_info = j['extra'])
		plain = run()
		args.uncertainty = True
		res = run()
		assert res.hyp == plain.hyp == j['hyp'] and torch.equal(res.alignment, plain.alignment)
		strip = lambda segs: [[{k: v for k, v in seg.items() if k not in UNCERTAINTY_KEYS} for seg in utt] for utt in segs]
		assert strip(res.hyp_segments) == plain.hyp_segments and strip(res.ref_segments) == plain.ref_segments
		words = [seg for utt in res.hyp_segments + res.ref_segments for seg in utt]
		assert len(words) > 0 and all(set(UNCERTAINTY_KEYS) <= set(seg) for seg in words)
		assert all(0 < seg['confidence_min'] <= seg['confidence'] <= 1 and seg['entropy'] >= 0 and seg['uncertainty'] >= 0 and -1 <= seg['margin'] <= 1 for seg in words)
		# the reference words against the restatement: positions of y mapped through the alignment onto the model's frames
		tok = text_pipeline.tokenizer
		lp = ca.ops.as_cl(res.log_probs, torch.float32).permute(0, 2, 1).cpu().numpy()
		y, ylen, fmap = T_(g['y'])[:, 0].tolist(), T_(g['ylen'])[:, 0].tolist(), res.alignment.cpu().tolist()
		s = R.greedy_spans(y, ylen, tok.eps_id, tok.space_id, generator.blank_amount_to_space)
		stats = R.frame_uncertainty(lp, tok.eps_id)
		want = R.span_uncertainty(lp, stats, s.utt, s.begin, s.end, s.first, s.tokens, s.frames, path = y, frame_map = fmap)
		held = np.array([bool((stats.idx[u, fmap[u][b]:max(fmap[u][b], fmap[u][e]) + 1] != tok.eps_id).any()) for u, b, e in zip(s.utt, s.begin, s.end)])
		_fields_check([seg for utt in res.ref_segments for seg in utt], want, lp, s, y, 'reference words over their aligned frames', frame_map = fmap, held_weighted = held)
	finally:
		torch.set_grad_enabled(True)  # (transcribe.setup switches autograd off for the process, like the reference)
