"""The keyword search on the MI355X: convasr_ctc_keyword_search, ops.ctc_keyword_search, ctc.search / search_bct and transcribe.search_batch /
search_long against the float32 restatement of the rule (tests/_kws_ref.py) on the same fp32 inputs.

Every comparison is bit for bit: scores as int32 views, begins, ends and counts equal, the dense outputs too wherever they are asked for, and
what lies beyond the stored hits still holds what the buffer held before the call.  The limits the shapes straddle -- labels per phrase,
phrases per workgroup, frames per tile, the class count at which staging through LDS ends -- are the library's own answers."""
import types

import numpy as np
import pytest
import torch

import _kws_ref as R

pytestmark = pytest.mark.gpu
SENT_F, SENT_I = np.float32(123.0), np.int32(-777)


def _dev():
	return torch.device('cuda:0')


def _limits():
	from convasr_amd import ops
	return ops.ctc_keyword_search_limits()


def _bits(a):
	return np.ascontiguousarray(np.asarray(a, dtype = np.float32)).view(np.int32)


def _pad(phrases):
	L_max = max(len(p) for p in phrases)
	return np.array([list(p) + [0] * (L_max - len(p)) for p in phrases], dtype = np.int32), np.array([len(p) for p in phrases], dtype = np.int32)


def c_call(lp, lengths, phrases, blank, thresholds, min_gap, H, dense = True):
	"""convasr_ctc_keyword_search itself on lp (B, T, C) float32, every output buffer pre-filled with a sentinel; returns numpy arrays."""
	from convasr_amd import _lib
	d = _dev()
	B, T, C = lp.shape
	K = len(phrases)
	tokens, tl = _pad(phrases)
	g = lambda a: torch.from_numpy(np.array(a)).to(d)
	lp_d, tok_d, tl_d = g(lp), g(tokens), g(tl)
	thr_d = g(np.broadcast_to(np.asarray(thresholds, dtype = np.float32), (K,)))
	len_d = None if lengths is None else g(np.asarray(lengths, dtype = np.int64))
	count = torch.full((B, K), int(SENT_I), dtype = torch.int32, device = d)
	score = torch.full((B, K, H), float(SENT_F), dtype = torch.float32, device = d)
	begin, end = torch.full((B, K, H), int(SENT_I), dtype = torch.int32, device = d), torch.full((B, K, H), int(SENT_I), dtype = torch.int32, device = d)
	ds = torch.full((B, K, T), float(SENT_F), dtype = torch.float32, device = d) if dense else None
	db = torch.full((B, K, T), int(SENT_I), dtype = torch.int32, device = d) if dense else None
	P = _lib.ptr
	_lib.call('convasr_ctc_keyword_search', P(lp_d), P(len_d), P(tok_d), P(tl_d), P(thr_d), P(count), P(score), P(begin), P(end), P(ds), P(db),
	          B, T, C, K, tokens.shape[1], H, int(blank), int(min_gap), _lib.stream_ptr())
	torch.cuda.synchronize()
	n = lambda t: None if t is None else t.cpu().numpy()
	return types.SimpleNamespace(count = n(count), score = n(score), begin = n(begin), end = n(end), dense_score = n(ds), dense_begin = n(db))


def same(got, want, what, dense = True):
	assert np.array_equal(got.count, want.count), (what, got.count, want.count)
	assert np.array_equal(_bits(got.score), _bits(want.score)), (what, got.score, want.score)
	assert np.array_equal(got.begin, want.begin) and np.array_equal(got.end, want.end), what
	if dense:
		assert np.array_equal(_bits(got.dense_score), _bits(want.dense_score)), what
		assert np.array_equal(got.dense_begin, want.dense_begin), what


def check_c(lp, lengths, phrases, blank, thresholds, min_gap, H, what):
	B, _, _ = lp.shape
	K = len(phrases)
	fill = np.full((B, K, H), SENT_F), np.full((B, K, H), SENT_I), np.full((B, K, H), SENT_I)
	want = R.search(lp, lengths, phrases, blank, thresholds, min_gap, H, fill = fill)
	got = c_call(lp, lengths, phrases, blank, thresholds, min_gap, H)
	same(got, want, what)
	print(f'  {what}: {int(want.count.sum())} hits, most per row {int(want.count.max())} (capacity {H})')
	return want


def rough(rng, B, T, C):
	"""Continuous inputs: normal logits x 2 with 5 % -inf entries."""
	lp = (rng.randn(B, T, C) * 2).astype(np.float32)
	lp[rng.rand(B, T, C) < 0.05] = -np.inf
	return lp


def phrase_of(rng, L, C, blank, repeat = True):
	labels = [c for c in range(C) if c != blank]
	p = [labels[rng.randint(len(labels))] for _ in range(L)]
	if repeat and L > 2:
		p[L // 2] = p[L // 2 - 1]
	return p


def ragged(T):
	return [0, T, max(1, (T + 1) // 2)]


def test_edges_labels():
	limit, _, _ = _limits()
	assert limit == 64
	rng = np.random.RandomState(1)
	C, blank = 38, 37
	T = 2 * _tile(C) + 3
	phrases = [phrase_of(rng, L, C, blank) for L in (1, 2, 31, 32, 33, 63, 64)]
	lp = rough(rng, 3, T, C)
	want = check_c(lp, ragged(T), phrases, blank, [-6.0 * len(p) for p in phrases], 3, 4, 'labels 1, 2, 31, 32, 33, 63, 64')
	print('  counts', want.count.tolist())
	assert (want.count[1] > 0).all() and (want.count[0] == 0).all()  # every phrase length is found in the full utterance; length 0 finds nothing


def _tile(C):
	from convasr_amd import ops
	return ops.ctc_keyword_search_tile_frames(C)


@pytest.mark.parametrize('which', range(5))
def test_edges_phrases_per_workgroup(which):
	_, P, _ = _limits()
	K = [1, P - 1, P, P + 1, 2 * P + 1][which]
	assert K >= 1
	rng = np.random.RandomState(10 + which)
	C, blank = 38, 0
	T = _tile(C) + 1
	phrases = [phrase_of(rng, 1 + (k * 3) % 7, C, blank) for k in range(K)]
	want = check_c(rough(rng, 3, T, C), ragged(T), phrases, blank, [-2.0 * len(p) for p in phrases], 2, 4, f'K = {K} phrases, {P} per workgroup')
	assert want.count.sum() > 0


@pytest.mark.parametrize('which', range(6))
def test_edges_frames_per_tile(which):
	C, blank = 38, 37
	F = _tile(C)
	T = [1, 2, F - 1, F, F + 1, 2 * F + 3][which]
	rng = np.random.RandomState(20 + which)
	phrases = [[5], [3, 3], [1, 2], phrase_of(rng, 5, C, blank), phrase_of(rng, 9, C, blank)]
	thresholds = [-np.inf if T <= 2 else -2.5 * len(p) for p in phrases]  # (one or two frames: whatever is finite is a hit)
	want = check_c(rough(rng, 3, T, C), ragged(T), phrases, blank, thresholds, 1, 4, f'T = {T} frames, tiles of {F}')
	assert want.count[1, 0] > 0 and (want.count[0] == 0).all()


@pytest.mark.parametrize('which', range(6))
def test_edges_classes(which):
	_, P, staged = _limits()
	C = [2, 38, 64, 65, staged, staged + 1][which]
	F = _tile(C)
	T = 2 * F + 3
	rng = np.random.RandomState(30 + which)
	blank = C - 1
	phrases = [phrase_of(rng, 1 + k, C, blank, repeat = k % 2 == 0) for k in range(P + 1)]
	want = check_c(rough(rng, 3, T, C), ragged(T), phrases, blank, [-3.0 * len(p) for p in phrases], 2, 4, f'C = {C} classes (staged up to {staged}), tiles of {F}, T = {T}')
	assert want.count.sum() > 0
	# an utterance of length 0 leaves its hit rows untouched
	got = c_call(rough(rng, 1, T, C), [0], phrases, blank, -1.0, 2, 4)
	assert (got.count == 0).all() and (got.score == SENT_F).all() and (got.begin == SENT_I).all() and (got.end == SENT_I).all()
	assert np.isneginf(got.dense_score).all() and (got.dense_begin == -1).all()


def dyadic(rng, B, T, C):
	"""Multiples of 1/16 in [-4, 0], 15 % -inf, one zero per frame: ties are frequent and every sum is exact."""
	lp = -rng.randint(0, 65, size = (B, T, C)).astype(np.float32) / 16
	lp[rng.rand(B, T, C) < 0.15] = -np.inf
	b, t = np.meshgrid(np.arange(B), np.arange(T), indexing = 'ij')
	lp[b, t, rng.randint(0, C, size = (B, T))] = 0.0
	return lp


def test_dyadic_inputs_with_ties_inf_and_nan():
	rng = np.random.RandomState(40)
	B, T, C, blank = 3, 90, 6, 0
	lp = dyadic(rng, B, T, C)
	lp[0, 7, 2] = np.nan          # a NaN entry: ignored by the frame's maximum, -inf as a score
	lp[1, 30, :] = np.nan         # a frame of NaNs and ...
	lp[2, 41, :] = -np.inf        # ... a frame of -inf: no state survives either, every begin is reset
	lp[0, 50, 1:] = -np.inf       # only the blank is possible here
	phrases = [[1], [1, 2], [1, 2, 3], [1, 2, 3, 4], [2, 2], [3, 3, 3], [1, 1, 2, 2], [5, 4, 5, 4, 5], [1, 2, 3, 4, 5, 1, 2, 3]]  # prefixes of each other; equal neighbours
	want = check_c(lp, [T, T, T - 5], phrases, blank, [-0.75 * len(p) for p in phrases], 2, 8, 'dyadic, ties, -inf, NaN')
	assert np.isneginf(want.dense_score[1, :, 30]).all() and (want.dense_begin[1, :, 30] == -1).all() and np.isneginf(want.dense_score[2, :, 41]).all()
	finite = np.isfinite(want.dense_score)
	assert finite.mean() > 0.3 and want.count.sum() > 20
	# ties are really there: equal finite scores at different frames of one row
	assert any(len(set(row[np.isfinite(row)].tolist())) < np.isfinite(row).sum() for row in want.dense_score.reshape(-1, T))
	for gap in (0, 5):
		check_c(lp, None, phrases, blank, -1.0, gap, 8, f'dyadic, one threshold, min_gap {gap}, no lengths')


def speech_like(rng, B, T, C, blank, phrases, plants):
	"""Unit normal logits boosted by 6 along a path of blank / label runs, log-softmaxed; plants: (utterance, phrase index, first frame) -- two
	frames per label and a blank between labels."""
	path = np.full((B, T), blank, dtype = np.int64)
	for b in range(B):
		t = 0
		while t < T:
			run = rng.randint(2, 5)
			path[b, t:t + run] = blank if rng.rand() < 0.6 else rng.randint(0, C - 1)
			t += run
	for b, k, first in plants:
		n = 3 * len(phrases[k]) - 1
		path[b, first - 2:first + n + 2] = blank
		for j, c in enumerate(phrases[k]):
			path[b, first + 3 * j:first + 3 * j + 2] = c
	logits = rng.randn(B, T, C).astype(np.float32)
	bi, ti = np.meshgrid(np.arange(B), np.arange(T), indexing = 'ij')
	logits[bi, ti, path] += np.float32(6.0)
	return torch.log_softmax(torch.from_numpy(logits), -1).numpy()


SPEECH = {}


def speech_case():
	"""2 x 300 x 38 and its reference results per min_gap, computed once."""
	if not SPEECH:
		rng = np.random.RandomState(50)
		C, blank = 38, 37
		phrases = [[4, 9, 2, 11], [20, 21, 36, 5, 5, 7], [30, 1, 30]]
		# phrase 0 twice 4 frames apart in utterance 0 and 60 apart in utterance 1; phrase 1 the other way round; phrase 2 thrice, ends 10 frames apart
		plants = [(0, 0, 20), (0, 0, 35), (1, 0, 30), (1, 0, 101), (1, 1, 140), (1, 1, 162), (0, 1, 80), (0, 1, 200), (0, 2, 250), (0, 2, 260), (0, 2, 270)]
		lp = speech_like(rng, 2, 300, C, blank, phrases, plants)
		thresholds = [-1.0 * len(p) for p in phrases]
		SPEECH.update(lp = lp, phrases = phrases, blank = blank, thresholds = thresholds, plants = plants,
		              want = {gap: R.search(lp, [300, 280], phrases, blank, thresholds, gap, 16) for gap in (0, 1, 10)})
	return types.SimpleNamespace(**SPEECH)


@pytest.mark.parametrize('min_gap', [0, 1, 10])
def test_speech_like_inputs_with_planted_phrases(min_gap):
	from convasr_amd import ops
	s = speech_case()
	tokens, tl = _pad(s.phrases)
	lp = torch.from_numpy(s.lp).to(_dev()).permute(0, 2, 1)
	got = ops.ctc_keyword_search(lp, tokens, tl, s.blank, s.thresholds, lengths = [300, 280], min_gap = min_gap, dense = True)
	want = s.want[min_gap]
	assert got.score.shape == (2, 3, 16)
	same(types.SimpleNamespace(**{k: getattr(got, k).cpu().numpy() for k in ('count', 'score', 'begin', 'end', 'dense_score', 'dense_begin')}), want, f'speech-like, min_gap {min_gap}')
	# every planted occurrence scores exactly 0 on its span in E; the picker keeps both of a pair that lies min_gap apart
	for b, k, first in s.plants:
		last = first + 3 * len(s.phrases[k]) - 2
		assert want.dense_score[b, k, last] == 0.0 and want.dense_begin[b, k, last] == first
	found = {(b, k): [(h[1], h[2], float(h[0])) for h in want.hits[b][k]] for b in range(2) for k in range(3)}
	print(f'  min_gap {min_gap}: counts {want.count.tolist()}, hits {found}')
	# A plant whose end lies more than min_gap after the ends of the earlier plants of its row is a hit of its own, from its first frame on.  At
	# min_gap 10 it is the whole span at score 0; a smaller min_gap emits the first end frame at or above the threshold, before the span is
	# complete (the rule: a candidate waits min_gap frames for a better one, no longer).  A closer plant (phrase 2 at min_gap 10: ends exactly 10
	# apart) arrives while the earlier candidate is still held, and an equal score with another begin does not replace it.
	ends = lambda b, k: [f + 3 * len(s.phrases[k]) - 2 for bb, kk, f in s.plants if (bb, kk) == (b, k)]
	kept = 0
	for b, k, first in s.plants:
		last = first + 3 * len(s.phrases[k]) - 2
		if all(last - e > min_gap for e in ends(b, k) if e < last):
			assert any(hb == first and he <= last for hb, he, _ in found[b, k]), (b, k, first)
			assert min_gap < 10 or (first, last, 0.0) in found[b, k], (b, k, first)
			kept += 1
	assert kept == (len(s.plants) if min_gap < 10 else len(s.plants) - 2) and (min_gap < 10 or all(hb != 260 for hb, _, _ in found[0, 2]))


def test_capacity():
	from convasr_amd import ops
	rng = np.random.RandomState(60)
	C, blank, phrase = 38, 37, [3, 8, 8, 2]
	plants = [(0, 0, 10 + 40 * i) for i in range(5)]
	lp = speech_like(rng, 1, 220, C, blank, [phrase], plants)
	want = R.search(lp, None, [phrase], blank, -4.0, 5, 5)
	assert want.count.tolist() == [[5]] and (want.score == 0.0).all()
	got = c_call(lp, None, [phrase], blank, -4.0, 5, 2, dense = False)
	assert got.count.tolist() == [[5]]
	assert np.array_equal(_bits(got.score), _bits(want.score[:, :, :2])) and np.array_equal(got.begin, want.begin[:, :, :2]) and np.array_equal(got.end, want.end[:, :, :2])
	# the rest of the buffer is untouched: the rows of a phrase that is not there and of an utterance of length 0 keep the sentinel
	more = c_call(np.concatenate([lp, lp]), [220, 0], [phrase, [30, 31, 32, 33]], blank, -4.0, 5, 2, dense = False)
	assert more.count.tolist() == [[5, 0], [0, 0]] and np.array_equal(more.end[0, 0], want.end[0, 0, :2])
	for a in (more.score, more.begin, more.end):
		assert (a[0, 1] == a.dtype.type(SENT_F if a.dtype == np.float32 else SENT_I)).all() and (a[1] == a.dtype.type(SENT_F if a.dtype == np.float32 else SENT_I)).all()
	tokens, tl = _pad([phrase])
	out = ops.ctc_keyword_search(torch.from_numpy(lp).to(_dev()).permute(0, 2, 1), tokens, tl, blank, -4.0, min_gap = 5, max_hits = 2)
	assert out.score.shape == (1, 1, 5) and out.count.tolist() == [[5]]
	assert np.array_equal(_bits(out.score.cpu().numpy()), _bits(want.score)) and np.array_equal(out.begin.cpu().numpy(), want.begin) and np.array_equal(out.end.cpu().numpy(), want.end)
	assert out.end[0, 0].tolist() == [10 + 40 * i + 10 for i in range(5)]


def test_capacity_leaves_the_rest_of_the_buffer_untouched():
	rng = np.random.RandomState(61)
	C, blank, phrase = 38, 37, [3, 8, 8, 2]
	lp = speech_like(rng, 1, 220, C, blank, [phrase], [(0, 0, 10 + 40 * i) for i in range(2)])
	got = c_call(lp, None, [phrase], blank, -4.0, 5, 6, dense = False)
	assert got.count.tolist() == [[2]] and (got.score[0, 0, :2] == 0.0).all()
	assert (got.score[0, 0, 2:] == SENT_F).all() and (got.begin[0, 0, 2:] == SENT_I).all() and (got.end[0, 0, 2:] == SENT_I).all()


def test_repeatability_and_routes():
	from convasr_amd import ctc, ops
	s = speech_case()
	tokens, tl = _pad(s.phrases)
	lp = torch.from_numpy(s.lp).to(_dev())  # (B, T, C)
	bct = lp.permute(0, 2, 1)
	keys = ('count', 'score', 'begin', 'end')
	one = ops.ctc_keyword_search(bct, tokens, tl, s.blank, s.thresholds, lengths = [300, 280], min_gap = 10, dense = True)
	two = ops.ctc_keyword_search(bct, tokens, tl, s.blank, s.thresholds, lengths = [300, 280], min_gap = 10, dense = True)
	for k in keys + ('dense_score', 'dense_begin'):
		assert torch.equal(getattr(one, k).view(torch.int32), getattr(two, k).view(torch.int32)), k
	plain = ops.ctc_keyword_search(bct, tokens, tl, s.blank, s.thresholds, lengths = [300, 280], min_gap = 10)
	assert plain.dense_score is None and plain.dense_begin is None
	tbc = ctc.search(lp.permute(1, 0, 2).contiguous(), torch.from_numpy(tokens), torch.from_numpy(tl), s.blank, torch.tensor(s.thresholds), lengths = torch.tensor([300, 280]), min_gap = 10)
	via_bct = ctc.search_bct(bct, tokens.tolist(), tl.tolist(), s.blank, s.thresholds, lengths = torch.tensor([300, 280], device = _dev()), min_gap = 10)
	for other in (plain, tbc, via_bct):
		for k in keys:
			assert torch.equal(getattr(one, k).view(torch.int32), getattr(other, k).view(torch.int32)), k
	same(types.SimpleNamespace(**{k: getattr(one, k).cpu().numpy() for k in keys}), s.want[10], 'routes', dense = False)
	# blank given from the end, a scalar threshold, padding beyond the longest phrase
	wide = np.concatenate([tokens, np.full((3, 70), 99, dtype = np.int32)], axis = 1)
	neg = ops.ctc_keyword_search(bct, wide, tl, s.blank - 38, -5.0, min_gap = 3)
	want = R.search(s.lp, None, s.phrases, s.blank, -5.0, 3, 16)
	same(types.SimpleNamespace(**{k: getattr(neg, k).cpu().numpy() for k in keys}), want, 'scalar threshold', dense = False)


def test_guards(monkeypatch):
	from convasr_amd import _lib, ops
	limit, _, _ = _limits()
	lp = torch.zeros(2, 80, 8, device = _dev()).permute(0, 2, 1)  # (B, C, T), channels-last
	with pytest.raises(_lib.ConvasrHipError, match = 'labels'):
		ops.ctc_keyword_search(lp, [[1] * (limit + 1)], [limit + 1], 0, -1.0)
	ok = ops.ctc_keyword_search(lp, [[1] * limit], [limit], 0, -1.0)
	assert ok.count.shape == (2, 1)
	launched = []
	real = ops.call
	monkeypatch.setattr(ops, 'call', lambda name, *a: (launched.append(name), real(name, *a))[1])
	for tokens, lengths, kw in (([[1, 0, 2]], [3], {}),            # a label equal to the blank
	                            ([[1, 8]], [2], {}), ([[1, -1]], [2], {}),  # labels outside [0, C)
	                            ([], [], {}), (np.zeros((0, 3), dtype = np.int32), np.zeros(0, dtype = np.int32), {}),  # an empty phrase list
	                            ([[1, 2]], [0], {}),               # an empty phrase
	                            ([[1, 2]], [3], {}),               # a length beyond the row
	                            ([[1, 2], [3, 4]], [2], {}),       # lengths that do not fit the phrases
	                            ([[1, 2]], [2], dict(thresholds = [-1.0, -2.0])),  # thresholds that do not fit
	                            ([[1, 2]], [2], dict(lengths = [5])),              # lengths of another batch
	                            ([[1, 2]], [2], dict(min_gap = -1)), ([[1, 2]], [2], dict(max_hits = 0)), ([[1, 2]], [2], dict(blank = 8))):
		args = dict(dict(blank = 0, thresholds = -1.0), **kw)
		with pytest.raises(ValueError):
			ops.ctc_keyword_search(lp, tokens, lengths, args.pop('blank'), args.pop('thresholds'), **args)
	with pytest.raises(ValueError):
		ops.ctc_keyword_search(lp[0], [[1]], [1], 0, -1.0)
	assert launched == []
	assert ops.ctc_keyword_search(lp, [[1, 0]], [1], 0, -1.0).count.shape == (2, 1)  # (a blank in the padding is no label)
	assert launched == ['convasr_ctc_keyword_search']


E2E_SEED = 1  # (chosen on the GPU among 0 .. 3: the hypotheses of seeds 1 and 2 hold long words; seed 0's and 3's are short and slow)


def small_model(seed):
	"""A random-weight Wav2Letter (base width 32, 38 classes) behind transcribe.setup.  The convolutions are drawn anew as He-normal weights
	(std = sqrt(2 / fan_in), no bias): under torch's default bound of 1 / sqrt(fan_in) each of the 18 layers shrinks its input about sixfold in
	eval mode, the logits are the decoder's bias at every frame and the hypothesis is one letter."""
	import convasr_amd as ca
	torch.manual_seed(seed)
	kwargs = dict(base_width = 32)
	sd = ca.models.Wav2Letter(64, [38], check_time_dim_padded = False, **kwargs).state_dict()
	for name, w in sd.items():
		if w.ndim == 3:
			torch.nn.init.normal_(w, 0.0, (2.0 / (w.shape[1] * w.shape[2])) ** 0.5)
		elif name.startswith('decoder') and name.endswith('bias'):
			w.zero_()
	ckpt = dict(sample_rate = 16000, window_size = 0.02, window_stride = 0.01, window = 'hann_window', num_input_features = 64, model = 'Wav2Letter', model_kwargs = kwargs)
	args = types.SimpleNamespace(checkpoint = dict(args = ckpt, model_state_dict = sd), device = 'cuda:0', fp16 = None, frontend_in_model = True, model = None)
	text_pipeline, _, model, generator = ca.transcribe.setup(args)
	return args, text_pipeline, model, generator


def overlaps(a, b):
	return a['begin'] <= b['end'] and b['begin'] <= a['end']


def test_end_to_end_through_a_model():
	from convasr_amd import ops, transcribe
	try:
		args, pipeline, model, generator = small_model(E2E_SEED)
		x = torch.randn(2, 16000, generator = torch.Generator().manual_seed(E2E_SEED)) * 0.1
		xlen, begin, end = torch.ones(2), torch.tensor([0.0, 10.0]), torch.tensor([1.0, 11.0])
		hyp = transcribe.transcribe_batch(args, pipeline, model, generator, x, xlen, begin, end)
		# every word of at least 2 letters with its segment; a segment's text may hold a space that the greedy rule INSERTED after a run of blanks --
		# the model did not emit it, so it is no part of a phrase that scores 0
		words = [[dict(w, hyp = word) for w in segs for word in w['hyp'].split() if len(word) >= 2] for segs in hyp.hyp_segments]
		print('  hypotheses:', hyp.hyp)
		assert all(len(w) >= 1 for w in words)
		phrases = sorted({w['hyp'] for segs in words for w in segs})
		used = set(''.join(hyp.hyp))
		absent = ''.join(c for c in pipeline.tokenizer.alphabet if c not in used)[:4]
		assert len(absent) == 4
		out = transcribe.search_batch(args, pipeline, model, x, xlen, begin, end, phrases + [absent], threshold_per_label = -0.5, segment_extra_info = [dict(channel = 0), dict(channel = 1)])
		assert out.phrases == phrases + [absent]
		for b in range(2):
			for w in words[b]:
				match = [h for h in out.hits[b] if h['phrase'] == w['hyp'] and overlaps(h, w)]
				assert match and any(h['score'] == 0.0 and h['score_per_label'] == 0.0 for h in match), (b, w, out.hits[b])
			assert all(h['channel'] == b and begin[b] <= h['begin'] <= h['end'] <= end[b] + 1e-3 for h in out.hits[b])
			assert all(h['phrase'] != absent for h in out.hits[b])
			assert [(h['begin'], h['end']) for h in out.hits[b]] == sorted((h['begin'], h['end']) for h in out.hits[b])
		# the hits' times are the greedy generator's: max(begin, 0) + ts[frame]
		found, ts = out.found, out.ts.cpu()
		k = phrases.index(words[1][0]['hyp'])
		n = int(found.count[1, k])
		want = [(10.0 + float(ts[1, int(found.begin[1, k, j])]), 10.0 + float(ts[1, int(found.end[1, k, j])])) for j in range(n)]
		assert [(h['begin'], h['end']) for h in out.hits[1] if h['phrase'] == phrases[k]] == want
		# a long recording with given segments: the hits carry the segments' clock and channel, and equal search_batch on the gathered batch
		signal = torch.cat([x[0], x[1]]).unsqueeze(0).to(_dev())
		segments = [dict(begin = 1.0, end = 2.0, channel = 0), dict(begin = 0.0, end = 1.0, channel = 0)]
		long = transcribe.search_long(args, pipeline, model, signal, phrases, segments = segments, threshold_per_label = -0.5)
		assert [(s['begin'], s['end'], s['channel']) for s in long.segments] == [(0.0, 1.0, 0), (1.0, 2.0, 0)]
		bx, bxlen = ops.gather_segments(signal, [0, 0], [s['first'] for s in long.segments], [s['count'] for s in long.segments], multiple = 128)
		by_hand = transcribe.search_batch(args, pipeline, model, bx, bxlen, torch.tensor([0.0, 1.0], dtype = torch.float64), torch.tensor([1.0, 2.0], dtype = torch.float64), phrases,
		                                  threshold_per_label = -0.5, segment_extra_info = [dict(channel = 0)] * 2)
		assert long.hits_per_segment == by_hand.hits and sum(len(h) for h in by_hand.hits) > 0
		assert long.hits == sorted((h for hits in by_hand.hits for h in hits), key = lambda h: (h['begin'], h['end'], h['channel']))
		for seg, hits in zip(long.segments, long.hits_per_segment):
			assert all(h['channel'] == 0 and seg['begin'] <= h['begin'] <= h['end'] <= seg['end'] + 0.05 for h in hits)  # (the batch is padded to 128 samples: a stamp may pass the segment's end by a frame)
		# phrases that cannot be searched
		for bad in (['q'], [''], ['а' * 65], []):
			with pytest.raises(ValueError):
				transcribe.search_long(args, pipeline, model, signal, bad, segments = segments)
		# silence: nothing to search in, the model is not called
		quiet = transcribe.search_long(args, pipeline, None, torch.zeros(1, 16000, device = _dev()), phrases)
		assert quiet.segments == [] and quiet.hits == [] and quiet.hits_per_segment == []
	finally:
		torch.set_grad_enabled(True)  # (transcribe.setup switches autograd off for the process, like the reference)
