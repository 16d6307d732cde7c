"""csrc/vad.hip through ops.frame_peaks / vad_frames / vad_segments / gather_segments, convasr_amd/vad.py and transcribe.transcribe_long, against
the numpy restatement tests/_vad_ref.py (itself checked on the CPU by tests/test_vad_ref.py).  Everything is compared with torch.equal: every
result is a maximum, a selection, a comparison or an integer, so no tolerance is needed.  The one bound, on word times, is derived where it is
used."""
import types

import numpy as np
import pytest
import torch

import _vad_ref as R

pytestmark = pytest.mark.gpu
VF_TILE, VF_CHUNK, SEG_TILE = 8192, 8, 1024  # frames per tile of convasr_vad_frames (include/convasr_hip.h), per thread of it, per tile of the segment kernels
FRAME_LENGTHS = [1, 3, 160, 320, 480]
DTYPES = [np.float32, np.int16]


def dev():
	return torch.device('cuda:0')


def gpu(a):
	return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def same(t, a):
	a = torch.from_numpy(np.ascontiguousarray(a))
	return t.dtype == a.dtype and t.shape == a.shape and torch.equal(t.cpu(), a)


# ------------------------------------------------------------------------------------------------ frame peaks

def peak_lengths(F):
	from convasr_amd import ops
	tile = ops.frame_peak_tile(F) * F  # samples one workgroup takes per step
	return sorted({n for n in (F - 1, F, F + 1, 2 * F - 1, 2 * F + 1, 7 * F + F // 2, tile - 1, tile, tile + 1, 3 * tile + F + 1) if n >= 1})


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('F', FRAME_LENGTHS)
def test_frame_peaks(F, dtype):
	from convasr_amd import ops
	assert ops.frame_peak_tile(F) == {1: 256, 3: 256, 160: 16, 320: 8, 480: 8}[F]
	for N in peak_lengths(F):
		for C in ((1, 2, 8) if N % 2 else (2, )):  # (odd N: rows 1, 3, .. start unaligned)
			x = R.bursts(C, N, dtype, seed = F * 1000 + N + C, sample_rate = 4 * F + 3)
			got = ops.frame_peaks(gpu(x), F)
			assert same(got, R.frame_peaks(x, F)), (F, dtype, C, N)
	# a view that starts 1 element into its storage: rows aligned to the element only
	x = R.bursts(2, 2 * F + 12, dtype, seed = F, sample_rate = 4 * F + 3)
	flat = gpu(np.concatenate([x[:1, :1].reshape(-1), x.reshape(-1)]))
	assert same(ops.frame_peaks(flat[1:].view(2, -1), F), R.frame_peaks(x, F))


@pytest.mark.parametrize('F, dtype', [(1, np.float32), (3, np.int16)])
def test_frame_peaks_past_the_grid(F, dtype):
	"""More frames than the launch has workgroup steps for (8 workgroups per compute unit): the stride loop takes the rest."""
	from convasr_amd import ops
	frames = torch.cuda.get_device_properties(0).multi_processor_count * 8 * ops.frame_peak_tile(F) + 257
	x = R.bursts(1, frames * F - (F - 1), dtype, seed = 5, sample_rate = 2000)
	got = ops.frame_peaks(gpu(x), F)
	want = np.abs(x.astype(np.int32 if dtype == np.int16 else np.float32))
	want = np.pad(want, ((0, 0), (0, F - 1))).reshape(1, frames, F).max(axis = 2).astype(np.float32)  # (one vectorised maximum here: half a million frames)
	assert same(got, want / np.float32(32767) if dtype == np.int16 else want)
	assert same(got[:, :2000], R.frame_peaks(x[:, :2000 * F], F)) and same(got[:, -300:], R.frame_peaks(x[:, (frames - 300) * F:], F))


# ------------------------------------------------------------------------------------------------ level, raw mask, smoothing

def edge_mask(nF):
	"""Speech runs and gaps of 1 to 9 frames laid around the edges of the scan's tiles, waves and per-thread chunks, and at both ends."""
	m = np.zeros(nF, bool)
	for edge in (0, VF_CHUNK, 64 * VF_CHUNK, VF_TILE, 2 * VF_TILE, nF):
		for k, (off, n) in enumerate([(-20, 3), (-14, 7), (-6, 6), (1, 1), (3, 7), (11, 8), (20, 9), (36, 1), (38, 1), (46, 2)]):
			a = edge + off
			m[max(a, 0):max(min(a + n, nF), 0)] = True
	return m


@pytest.mark.parametrize('nF', [1, 2, VF_CHUNK + 1, VF_TILE - 1, VF_TILE, VF_TILE + 1, 2 * VF_TILE + 37])
def test_smoothing_on_runs_at_the_scan_tile_edges(nF):
	from convasr_amd import ops
	rng = np.random.default_rng(nF)
	mask = np.stack([edge_mask(nF), ~edge_mask(nF), rng.random(nF) < 0.5])
	peaks = np.where(mask, 0.5, 0.001).astype(np.float32)  # level 0.5 or 0.001: raw = the mask for the thresholds below, whole frames only
	for nfull in (sorted({nF, max(nF - 1, 1)}) if nF <= VF_TILE else [nF - 1]):  # (with and without a partial last frame; the longest masks with one only)
		k = R.rank(0.9, nfull)
		lev = R.level(peaks, nfull, k)
		want_raw = R.raw_mask(peaks, nfull, lev, 0.02, 0.1, 1e-9)
		assert same(ops.kth_value(gpu(peaks)[:, :nfull], k), lev)
		assert (want_raw[:, :nfull] == mask[:, :nfull]).all() and not want_raw[:, nfull:].any()
		for G in (0, 1, 7):
			for S in (0, 1, 7):
				for P in (0, 1, 7):
					raw, got = ops.vad_frames(gpu(peaks), nfull, 0.02, 0.1, 1e-9, k, G, S, P)
					assert same(raw, want_raw) and same(got, R.smooth(want_raw, G, S, P)), (nF, nfull, G, S, P)
	raw, got = ops.vad_frames(gpu(peaks), 0, 0.02, 0.1, 1e-9, 1, 7, 7, 7)  # no whole frame: all False
	assert raw.shape == got.shape == (3, nF) and not bool(raw.any()) and not bool(got.any())


@pytest.mark.parametrize('dtype', DTYPES)
def test_level_raw_and_mask_of_a_recording(dtype):
	from convasr_amd import ops
	x = R.bursts(2, 8000 * 20 + 77, dtype, seed = 11)
	for F, (abs_thr, rel_thr), G, S, P in [(160, R.THRESHOLDS[2], 50, 25, 10), (80, R.THRESHOLDS[0], 9, 30, 3), (480, R.THRESHOLDS[3], 2, 2, 400)]:
		nF, nfull = R.n_frames(x.shape[1], F)
		peaks = R.frame_peaks(x, F)
		k = R.rank(0.9, nfull)
		want_raw = R.raw_mask(peaks, nfull, R.level(peaks, nfull, k), abs_thr, rel_thr, 1e-9)
		raw, got = ops.vad_frames(ops.frame_peaks(gpu(x), F), nfull, abs_thr, rel_thr, 1e-9, k, G, S, P)
		assert 0 < want_raw.sum() < want_raw.size
		assert same(raw, want_raw) and same(got, R.smooth(want_raw, G, S, P)), (F, G, S, P)
	# an all-zero channel is all silence, whatever its neighbour holds
	x[0] = 0
	raw, got = ops.vad_frames(ops.frame_peaks(gpu(x), 160), x.shape[1] // 160, 0.0, 0.1, 1e-9, 1, 0, 0, 0)
	assert not bool(raw[0].any()) and not bool(got[0].any()) and bool(raw[1].any())


# ------------------------------------------------------------------------------------------------ segments

def check_segments(mask, peaks, F, N, M):
	from convasr_amd import ops
	got = ops.vad_segments(gpu(mask), gpu(peaks), F, N, M)
	want = R.segments(mask, peaks, F, N, M)
	assert all(t.dtype == torch.int64 and t.is_cuda for t in got)
	assert [t.tolist() for t in got] == [list(w) for w in want], (mask.shape, F, N, M)
	return want


@pytest.mark.parametrize('M', [0, 2, 3, 50])
def test_segments_of_runs_of_M_frames_and_more(M):
	m = max(M, 4)
	runs = [(3, m), (2, m + 1), (1, 5 * m), (4, 1), (1, 2), (SEG_TILE, m + 1), (2, 3)]  # (silence before, speech)
	row0 = np.concatenate([np.concatenate([np.zeros(s, bool), np.ones(n, bool)]) for s, n in runs])  # ends in speech: the last count is clipped to N
	nF = len(row0)
	mask = np.stack([row0, row0[::-1]])
	F, N = 160, nF * 160 - 37
	rng = np.random.default_rng(M)
	for peaks in (np.ones((2, nF), np.float32), rng.integers(0, 3, (2, nF)).astype(np.float32), rng.random((2, nF)).astype(np.float32)):  # constant: every candidate ties
		channel, first, count = check_segments(mask, peaks, F, N, M)
		assert first[0] == 3 * F and max(np.add(first, count)) == N and (M == 0 or max(count) <= M * F)
	check_segments(mask, np.ones((2, nF), np.float32), 1, nF, M)
	check_segments(mask[:1], np.ones((1, nF), np.float32), 3, nF * 3 - 2, M)


@pytest.mark.parametrize('M', [0, 2, 3, 50])
def test_segments_of_no_speech_all_speech_and_random_masks(M):
	from convasr_amd import ops
	nF = 2 * SEG_TILE + 5
	rng = np.random.default_rng(100 + M)
	peaks = rng.integers(0, 5, (3, nF)).astype(np.float32)
	got = ops.vad_segments(gpu(np.zeros((3, nF), bool)), gpu(peaks), 160, nF * 160, M)
	assert all(t.shape == (0, ) and t.dtype == torch.int64 for t in got)
	channel, first, count = check_segments(np.ones((3, nF), bool), peaks, 160, nF * 160 - 159, M)
	assert (len(channel) == 3) == (M == 0) and sum(count) == 3 * (nF * 160 - 159)
	check_segments(np.ones((1, nF), bool), np.ones((1, nF), np.float32), 2, nF * 2, M)
	for density in (0.5, 0.9, 0.99):
		mask = rng.random((3, nF)) < density
		mask[1] = R.smooth_row(mask[1], 3, 0, 0)
		check_segments(mask, peaks, 160, nF * 160 - 1, M)
	check_segments(np.ones((1, 1), bool), np.ones((1, 1), np.float32), 5, 3, M)
	check_segments(np.array([[True, False, True]]), np.ones((1, 3), np.float32), 5, 15, M)


# ------------------------------------------------------------------------------------------------ gather

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('multiple', [1, 128])
def test_gather_segments(dtype, multiple):
	from convasr_amd import ops
	N = 5003
	x = R.bursts(2, N, dtype, seed = 21, sample_rate = 300)
	x[:, ::7] = np.array(0.25 if dtype == np.float32 else 8191, dtype)  # (no all-zero segment)
	base = [(r % 2, 40 + r, 100 + r) for r in range(8)] + [(0, 0, 1), (1, N - 256, 256), (0, 17, 255), (1, N - 1, 1)]  # first at every residue mod 8; counts 1, Tpad - 1, Tpad; ends at N
	rng = np.random.default_rng(3)
	many = base + [(int(rng.integers(0, 2)), int(a), int(rng.integers(1, min(257, N - a + 1)))) for a in rng.integers(0, N, 65 - len(base))]
	for segs in (base, many, [(1, 1001, 130)]):
		channel, first, count = (list(v) for v in zip(*segs))
		want_x, want_len = R.gather(x, channel, first, count, multiple)
		assert want_x.shape == (len(segs), 130 if (len(segs) == 1 and multiple == 1) else 256)
		for as_tensor in (False, True):
			args = [torch.tensor(v, device = dev()) for v in (channel, first, count)] if as_tensor else [channel, first, count]
			got_x, got_len = ops.gather_segments(gpu(x), *args, multiple = multiple)
			assert same(got_x, want_x) and same(got_len, want_len), (dtype, multiple, len(segs), as_tensor)
	assert len(many) == 65


# ------------------------------------------------------------------------------------------------ vad.py

@pytest.mark.parametrize('dtype', DTYPES)
def test_detect_speech_and_segments_of_a_recording(dtype):
	from convasr_amd import vad
	sr = 8000
	x = R.bursts(2, sr * 12 + 77, dtype, seed = 31)
	x[1, :sr * 5] = x[0, sr * 2:sr * 7] // 3 if dtype == np.int16 else x[0, sr * 2:sr * 7] * np.float32(0.3)
	for window_size, aggressiveness, dilate in [(0.02, 2, None), (0.01, 0, None), (0.03, 3, None), (0.02, 1, 0.1)]:
		cfg = R.settings(sr, window_size, aggressiveness, dilate)
		peaks, _, mask = R.detect_frames(x, cfg)
		got_mask, got_peaks = vad.detect_speech_frames(gpu(x), sr, window_size, aggressiveness, dilate)
		assert same(got_mask, mask) and same(got_peaks, peaks) and 0 < mask.sum() < mask.size
		speech = vad.detect_speech(gpu(x), sr, window_size, aggressiveness, dilate)
		assert speech.is_cuda and same(speech, R.detect_speech(x, cfg)) and same(speech, np.repeat(mask, cfg['F'], axis = 1)[:, :x.shape[1]])
		assert torch.equal(speech, vad.detect_speech(gpu(x), sr, window_size, aggressiveness, dilate))  # two runs are bit-equal
		for max_duration in (1.0, None):
			M = R.frames_of(max_duration, window_size) if max_duration else 0
			channel, first, count = R.segments(mask, peaks, cfg['F'], x.shape[1], M)
			got = vad.segments(gpu(x), sr, window_size, aggressiveness, dilate, max_duration = max_duration, audio_path = 'a.wav')
			want = [dict(audio_path = 'a.wav', begin = a / sr, end = (a + n) / sr, channel = c, first = a, count = n) for c, a, n in zip(channel, first, count)]
			assert got == want and len(want) >= 2 and (not M or max(count) <= M * cfg['F'])
			assert got == vad.segments(gpu(x), sr, window_size, aggressiveness, dilate, max_duration = max_duration, audio_path = 'a.wav')
	# overrides reach the kernels
	cfg = dict(R.settings(sr, 0.02, 2), abs_thr = 0.3, G = 3, S = 4, P = 0, percentile = 0.5)
	got_mask, _ = vad.detect_speech_frames(gpu(x), sr, 0.02, 2, abs_thr = 0.3, gap_frames = 3, speech_frames = 4, pad_frames = 0, percentile = 0.5)
	assert same(got_mask, R.detect_frames(x, cfg)[2])
	# shorter than a frame: nothing is speech, and there are no segments
	short = gpu(x[:, :159])
	assert not bool(vad.detect_speech(short, sr, 0.02, 2).any()) and vad.detect_speech(short, sr, 0.02, 2).shape == (2, 159) and vad.segments(short, sr) == []


def test_refusals():
	from convasr_amd import ops, vad
	from convasr_amd._lib import ConvasrHipError
	d = dev()
	ok = torch.zeros(2, 1000, device = d)
	for bad in (torch.zeros(9, 100, device = d), torch.zeros(1, 0, device = d), torch.zeros(100, device = d), torch.zeros(1, 100, device = d, dtype = torch.float64)):
		with pytest.raises(ValueError):
			vad.detect_speech(bad, 8000, 0.02, 2)
		with pytest.raises(ValueError):
			vad.segments(bad, 8000)
	for call in (lambda: vad.detect_speech(ok, 8000, 0.0001, 2), lambda: vad.detect_speech(ok, 8000, 0.02, 5), lambda: vad.segments(ok, 8000, max_duration = 0.02),
	             lambda: vad.detect_speech_frames(ok, 8000, 0.02, 2, gap_frames = -1), lambda: ops.frame_peaks(torch.zeros(3, device = d), 10),
	             lambda: ops.gather_segments(ok, [0], [0, 1], [5]), lambda: ops.gather_segments(ok, [], [], []), lambda: ops.vad_frames(torch.zeros(2, 10, device = d, dtype = torch.float64), 10, .1, .1, 0, 1, 0, 0, 0),
	             lambda: ops.vad_segments(torch.zeros(2, 10, device = d), torch.zeros(2, 10, device = d), 10, 100, 0)):
		with pytest.raises(ValueError):
			call()
	mask, peaks = torch.ones(2, 10, dtype = torch.bool, device = d), torch.ones(2, 10, device = d)
	for call in (lambda: ops.frame_peaks(torch.zeros(9, 100, device = d), 10), lambda: ops.frame_peaks(torch.zeros(1, 0, device = d), 10), lambda: ops.frame_peaks(ok, 0), lambda: ops.frame_peaks(ok, 65537),
	             lambda: ops.vad_segments(mask, peaks, 10, 100, 1), lambda: ops.vad_segments(mask, peaks, 10, 101, 0), lambda: ops.vad_frames(peaks, 8, .1, .1, 0, 1, 0, 0, 0),
	             lambda: ops.vad_frames(peaks, 10, .1, .1, 0, 1, -1, 0, 0), lambda: ops.gather_segments(ok, [0], [990], [11]), lambda: ops.gather_segments(ok, [2], [0], [5]),
	             lambda: ops.gather_segments(ok, [0], [-1], [5]), lambda: ops.gather_segments(ok, [0], [0], [0]), lambda: ops.gather_segments(ok, [0], [0], [1 << 40]),
	             lambda: vad.detect_speech(ok.cpu(), 8000, 0.02, 2), lambda: vad.segments(ok.cpu(), 8000), lambda: ops.frame_peaks(ok.cpu(), 10), lambda: ops.vad_frames(peaks.cpu(), 10, .1, .1, 0, 1, 0, 0, 0),
	             lambda: ops.vad_segments(mask.cpu(), peaks.cpu(), 10, 100, 0), lambda: ops.gather_segments(ok.cpu(), [0], [0], [5])):
		with pytest.raises(ConvasrHipError):
			call()
	torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ transcribe_long

def recording_model(pipeline, seen):
	"""A model that records the batches it is given and answers with log-probs that depend on their shape only: one frame per 16 samples, and
	floor(xlen * (frames - 1)) + 1 valid frames, so that the last valid frame's time stamp, (frames_valid - 1) / (frames - 1) of the padded
	duration, does not lie past xlen of it."""
	def model(x, xlen):
		seen.append((x, xlen))
		frames = x.shape[-1] // 16
		gen = torch.Generator().manual_seed(3)
		log_probs = torch.randn(x.shape[0], pipeline.tokenizer.vocab_size, frames, generator = gen).log_softmax(dim = 1).to(x.device)
		return log_probs, log_probs, (xlen.double() * (frames - 1)).floor().to(torch.int64) + 1
	return model


def by_hand(transcribe, args, pipeline, x, segs, sr, seen = None):
	"""What transcribe_long must return for the segments (channel, first, count) in channel-then-time order: the restatement's batches -- longest
	first, a stable sort, chunks of args.batch_size -- through transcribe_batch, the results put back in the segments' order."""
	from convasr_amd.transcript_generators import GreedyCTCGenerator
	channel, first, count = segs
	n = len(channel)
	order = sorted(range(n), key = lambda i: -count[i])
	hyp_segments, hyp, calls = [None] * n, [None] * n, []
	for at in range(0, n, args.batch_size):
		idx = order[at:at + args.batch_size]
		bx, bxlen = R.gather(x, [channel[i] for i in idx], [first[i] for i in idx], [count[i] for i in idx], args.batch_time_padding_multiple)
		calls.append((bx, bxlen))
		begin, end = torch.tensor([first[i] / sr for i in idx], dtype = torch.float64), torch.tensor([(first[i] + count[i]) / sr for i in idx], dtype = torch.float64)
		out = transcribe.transcribe_batch(args, pipeline, recording_model(pipeline, []), GreedyCTCGenerator(), gpu(bx), gpu(bxlen), begin, end, segment_extra_info = [dict(channel = channel[i]) for i in idx])
		for i, words, text in zip(idx, out.hyp_segments, out.hyp):
			hyp_segments[i], hyp[i] = words, text
	transcript = sorted([w for words in hyp_segments for w in words], key = lambda w: (w['begin'], w['end'], w['channel']))
	text = [' '.join(filter(bool, [hyp[i].strip() for i in sorted(range(n), key = lambda i: (first[i], count[i])) if channel[i] == c])) for c in range(x.shape[0])]
	return types.SimpleNamespace(calls = calls, hyp_segments = hyp_segments, hyp = hyp, transcript = transcript, text = text)


def check_long(out, want, seen, segs, sr, multiple):
	channel, first, count = segs
	assert [(s['channel'], s['first'], s['count']) for s in out.segments] == list(zip(channel, first, count))
	assert [(s['begin'], s['end']) for s in out.segments] == [(a / sr, (a + n) / sr) for a, n in zip(first, count)]
	assert len(seen) == len(want.calls) and all(same(x, bx) and same(xlen, bxlen) for (x, xlen), (bx, bxlen) in zip(seen, want.calls))
	assert out.hyp_segments == want.hyp_segments and out.hyp == want.hyp and out.transcript == want.transcript and out.text == want.text
	assert sum(len(words) for words in out.hyp_segments) == len(out.transcript) > 0
	# A stamp is begin + fp32(fp32(D) * linspace[t]) with D = Tpad / sr the batch's padded duration and t a valid frame, so exactly at most
	# begin + count / sr = end (recording_model's length rule).  In fp32: D and the product are rounded once each (2^-24 relative), and torch's
	# linspace over [0, 1] is start + step * i or end - step * (steps - 1 - i), off by at most 2^-23 absolute: 2^-21 D covers the three.
	slack = 2.0 ** -21 * (max(count) + multiple) / sr
	for seg, words in zip(out.segments, out.hyp_segments):
		assert all(w['channel'] == seg['channel'] and seg['begin'] <= w['begin'] <= w['end'] <= seg['end'] + slack for w in words)


def test_transcribe_long():
	from convasr_amd import diarization, transcribe
	from convasr_amd.transcript_generators import CharTokenizerLegacy, GreedyCTCGenerator
	sr = 8000
	pipeline = transcribe.TextPipeline(CharTokenizerLegacy('abc'))
	args = types.SimpleNamespace(device = 'cuda:0', sample_rate = sr, batch_size = 4, batch_time_padding_multiple = 128, vad_max_duration = 1.0)
	x = R.bursts(2, sr * 10 + 77, np.float32, seed = 41)
	seen = []
	out = transcribe.transcribe_long(args, pipeline, recording_model(pipeline, seen), GreedyCTCGenerator(), gpu(x))
	cfg = R.settings(sr, 0.02, 2)
	peaks, _, mask = R.detect_frames(x, cfg)
	segs = R.segments(mask, peaks, cfg['F'], x.shape[1], 50)
	assert len(segs[0]) > 2 * args.batch_size and len(set(segs[0])) == 2 and len(set(segs[2])) > 3
	check_long(out, by_hand(transcribe, args, pipeline, x, segs, sr), seen, segs, sr, 128)
	# other settings from args; an int16 signal
	args2 = types.SimpleNamespace(device = 'cuda:0', sample_rate = sr, batch_size = 64, batch_time_padding_multiple = 1, vad_max_duration = 0.5, vad_window_size = 0.01, vad_aggressiveness = 0)
	pcm = R.bursts(2, sr * 6 + 5, np.int16, seed = 42)
	seen = []
	out = transcribe.transcribe_long(args2, pipeline, recording_model(pipeline, seen), GreedyCTCGenerator(), gpu(pcm))
	cfg = R.settings(sr, 0.01, 0)
	peaks, _, mask = R.detect_frames(pcm, cfg)
	segs = R.segments(mask, peaks, cfg['F'], pcm.shape[1], 50)
	check_long(out, by_hand(transcribe, args2, pipeline, pcm, segs, sr), seen, segs, sr, 1)
	# given segments, out of order and with ends beyond N: the dataset's slice rule
	N = x.shape[1]
	given = [dict(begin = 9.5, end = 100.0, channel = 1, ref = 'x'), dict(begin = 0.5, end = 1.25, channel = 0), dict(begin = 0.0, end = 0.0, channel = 1), dict(begin = 3.0, end = N / sr, channel = 0),
	         dict(begin = 2.0001, end = 2.5, channel = 0)]
	seen = []
	out = transcribe.transcribe_long(args, pipeline, recording_model(pipeline, seen), GreedyCTCGenerator(), gpu(x), segments = given)
	rows = sorted((g['channel'], ) + R.segment_samples(g['begin'], g['end'], sr, N) + (g['begin'], g['end']) for g in given)
	segs = tuple([r[k] for r in rows] for k in range(3))
	assert segs[2] == [int(1.25 * sr) + 1 - int(0.5 * sr), int(2.5 * sr) + 1 - int(2.0001 * sr), N - 3 * sr, 1, N - int(9.5 * sr)]
	assert [(s['begin'], s['end']) for s in out.segments] == [(r[3], r[4]) for r in rows] and out.segments[-1]['ref'] == 'x'
	want = by_hand(transcribe, args, pipeline, x, segs, sr)
	assert len(seen) == 2 and all(same(a, bx) and same(b, bxlen) for (a, b), (bx, bxlen) in zip(seen, want.calls))
	assert out.hyp == want.hyp and [[w['hyp'] for w in words] for words in out.hyp_segments] == [[w['hyp'] for w in words] for words in want.hyp_segments]
	# a diarization's segments: channel = speaker - 1
	turns = diarization.diarize(gpu(x), sr, kernel_size_smooth_silence = 512, kernel_size_smooth_speaker = 512)
	assert len(turns) >= 2
	seen = []
	out = transcribe.transcribe_long(args, pipeline, recording_model(pipeline, seen), GreedyCTCGenerator(), gpu(x), segments = [dict(t, channel = t['speaker'] - 1) for t in turns])
	rows = sorted((t['speaker'] - 1, ) + R.segment_samples(t['begin'], t['end'], sr, N) for t in turns)
	segs = tuple([r[k] for r in rows] for k in range(3))
	want = by_hand(transcribe, args, pipeline, x, segs, sr)
	assert all(same(a, bx) and same(b, bxlen) for (a, b), (bx, bxlen) in zip(seen, want.calls)) and len(seen) == len(want.calls) and out.hyp == want.hyp
	assert all(s['speaker'] == s['channel'] + 1 for s in out.segments)
	# silence: empty lists, and the model is not called
	seen = []
	out = transcribe.transcribe_long(args, pipeline, recording_model(pipeline, seen), GreedyCTCGenerator(), torch.zeros(2, sr * 3, device = dev()))
	assert seen == [] and out.segments == [] and out.hyp_segments == [] and out.hyp == [] and out.transcript == [] and out.text == ['', '']


def test_transcribe_long_reads_a_file(tmp_path):
	import os
	from convasr_amd import audio, transcribe
	from convasr_amd.transcript_generators import CharTokenizerLegacy, GreedyCTCGenerator
	wav = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'audio_stereo.wav')
	pipeline = transcribe.TextPipeline(CharTokenizerLegacy('abc'))
	for mono, channels in ((True, 1), (False, 2)):
		args = types.SimpleNamespace(device = 'cuda:0', sample_rate = 16000, mono = mono, vad_window_size = 0.002, vad_aggressiveness = 0)
		signal, sr = audio.read_audio(wav, 16000, mono = mono)
		seen = []
		out = transcribe.transcribe_long(args, pipeline, recording_model(pipeline, seen), GreedyCTCGenerator(), wav)
		x = signal.cpu().numpy()
		cfg = R.settings(sr, 0.002, 0)
		peaks, _, mask = R.detect_frames(x, cfg)
		segs = R.segments(mask, peaks, cfg['F'], x.shape[1], R.frames_of(15.0, 0.002))
		assert signal.shape[0] == channels and [(s['channel'], s['first'], s['count']) for s in out.segments] == list(zip(*segs))
		if segs[0]:
			args.batch_size, args.batch_time_padding_multiple = 64, 128
			want = by_hand(transcribe, args, pipeline, x, segs, sr)
			assert all(same(a, bx) for (a, _), (bx, _) in zip(seen, want.calls)) and out.hyp == want.hyp
		assert len(out.text) == channels
