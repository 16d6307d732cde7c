"""The numpy restatement of the speech-activity detector (tests/_vad_ref.py) on hand-written cases, and the host rules of convasr_amd/vad.py
(presets, segment_samples, upsample) and models.silence_space_mask on the CPU.  tests/test_vad_gpu.py compares the kernels with the restatement."""
import numpy as np
import pytest
import torch

import _vad_ref as R


def row(text):
	return np.array([ch == '#' for ch in text])


def text(mask):
	return ''.join('#' if v else '.' for v in mask)


def test_a_gap_shorter_than_G_is_filled_and_a_gap_of_G_is_not():
	assert text(R.smooth_row(row('##...##'), 4, 0, 0)) == '#######'  # a gap of G - 1 frames
	assert text(R.smooth_row(row('##...##'), 3, 0, 0)) == '##...##'  # a gap of G frames
	assert text(R.smooth_row(row('...##..'), 9, 0, 0)) == '...##..'  # silence that touches an end has speech on one side only
	assert text(R.smooth_row(row('#.#..#'), 2, 0, 0)) == '###..#'


def test_a_run_shorter_than_S_is_removed_and_a_run_of_S_is_kept():
	assert text(R.smooth_row(row('..##...'), 0, 3, 0)) == '.......'  # S - 1 frames
	assert text(R.smooth_row(row('..##...'), 0, 2, 0)) == '..##...'  # S frames
	assert text(R.smooth_row(row('#...###..##'), 0, 3, 0)) == '....###....'  # a short run at either end of the recording goes too
	assert text(R.smooth_row(row('#.#.#'), 2, 4, 0)) == '#####'  # step 2 sees the result of step 1: one run of 5


def test_pads_merge_and_clip_at_both_ends():
	assert text(R.smooth_row(row('..#....#..'), 0, 0, 2)) == '##########'  # [0, 5) and [5, 10) meet
	assert text(R.smooth_row(row('.#......#.'), 0, 0, 2)) == '####..####'  # clipped at 0 and at nF
	assert text(R.smooth_row(row('...#......'), 0, 0, 1)) == '..###.....'
	assert text(R.smooth_row(row('#.#....'), 0, 2, 1)) == '.......'  # step 3 pads what step 2 left: nothing


def test_a_partial_last_frame_is_never_raw_speech_but_the_pad_reaches_it():
	x = np.zeros((1, 10), np.float32)
	x[0, 4:] = 0.5
	peaks = R.frame_peaks(x, 4)  # frames [0, 4), [4, 8), [8, 10): the last one partial, and loud
	assert peaks.tolist() == [[0.0, 0.5, 0.5]]
	raw = R.raw_mask(peaks, 2, R.level(peaks, 2, 2), 0.02, 0.1, 1e-9)
	assert raw.tolist() == [[False, True, False]]
	assert R.smooth(raw, 0, 0, 1).tolist() == [[True, True, True]]
	assert R.segments(R.smooth(raw, 0, 0, 1), peaks, 4, 10, 0) == ([0], [0], [10])  # count = min(b F, N) - a F


def test_the_cut_takes_the_lowest_index_among_ties_inside_its_window():
	peaks = np.ones(20, np.float32)
	assert R.cut_run(0, 20, peaks, 6) == [(0, 3), (3, 6), (6, 9), (9, 12), (12, 15), (15, 20)]  # all ties: a + ceil(M / 2) every time; the rest of 5 <= M stays
	peaks[4] = peaks[5] = 0.25
	assert R.cut_run(0, 20, peaks, 6)[0] == (0, 4)  # the lower of two equal minima
	peaks[6] = 0.0  # in neither window: [3, 6) for a = 0, then [7, 10) for a = 4, where every candidate ties
	assert R.cut_run(0, 20, peaks, 6)[:2] == [(0, 4), (4, 7)]


def test_the_cut_window_excludes_its_upper_end():
	peaks = np.ones(10, np.float32)
	peaks[4] = 0.0  # a + M for a = 0, M = 4: outside [2, 4)
	assert R.cut_run(0, 10, peaks, 4) == [(0, 2), (2, 4), (4, 6), (6, 10)]
	assert R.cut_run(0, 5, np.array([1, 1, 1, .5, 1], np.float32), 4) == [(0, 3), (3, 5)]
	assert R.cut_run(3, 7, peaks, 4) == [(3, 7)] and R.cut_run(0, 10, peaks, 0) == [(0, 10)]


@pytest.mark.parametrize('M', [0, 2, 3, 7, 50])
def test_segments_have_1_to_M_frames_and_tile_the_mask(M):
	rng = np.random.default_rng(M)
	for trial in range(60):
		nF = int(rng.integers(1, 200))
		mask = R.smooth(rng.random((2, nF)) < rng.uniform(0.2, 0.98), int(rng.integers(0, 4)), 0, 0)
		peaks = rng.integers(0, 4, (2, nF)).astype(np.float32)  # few values: many ties
		segs = R.segment_frames(mask, peaks, M)
		cover = np.zeros_like(mask, dtype = np.int32)
		for c, a, b in segs:
			assert 1 <= b - a and (M == 0 or b - a <= M)
			cover[c, a:b] += 1
		assert (cover == mask.astype(np.int32)).all()
		assert segs == sorted(segs)
		starts = {(c, a) for c, a, b in segs}
		for c in range(2):
			for a, b in R.runs_of(mask[c]):
				assert (c, a) in starts and (M != 0 or (c, a, b) in segs)


def test_rank_and_level_for_one_and_two_whole_frames():
	assert R.rank(0.9, 1) == 1 and R.rank(0.9, 2) == 1 and R.rank(0.9, 10) == 9 and R.rank(0.9, 180000) == 162000
	peaks = np.array([[0.5, 0.25, 9.0]], np.float32)
	assert R.level(peaks, 1, 1).tolist() == [0.5] and R.level(peaks, 2, 1).tolist() == [0.25] and R.level(peaks, 2, 2).tolist() == [0.5]


def test_an_all_zero_channel_is_all_silence():
	x = np.zeros((2, 64), np.float32)
	x[1, 16:48] = 0.5
	peaks, raw, mask = R.detect_frames(x, dict(F = 8, abs_thr = 0.02, rel_thr = 0.1, percentile = 0.9, eps = 1e-9, G = 2, S = 2, P = 1))
	assert not raw[0].any() and not mask[0].any()
	assert text(raw[1]) == '..####..' and text(mask[1]) == '.######.'
	# with abs_thr = 0 the relative test alone decides: 0 / (eps + 0) = 0 < rel_thr
	assert not R.raw_mask(peaks, 8, R.level(peaks, 8, 7), 0.0, 0.1, 1e-9)[0].any()


def test_int16_full_scale_negative_peak():
	pcm = np.array([[0, -32768, 5, 32767]], np.int16)
	peaks = R.frame_peaks(pcm, 2)
	assert peaks.dtype == np.float32 and peaks[0, 0] == np.float32(32768) / np.float32(32767) and peaks[0, 0] > 1 and peaks[0, 1] == 1.0
	assert R.frame_peaks(np.array([[-3, 2, 1]], np.int16), 2).tolist() == [[np.float32(3) / np.float32(32767), np.float32(1) / np.float32(32767)]]


@pytest.mark.parametrize('window_size, want', [(0.01, (100, 50, 20)), (0.02, (50, 25, 10)), (0.03, (33, 17, 7))])
def test_seconds_to_frames_of_the_presets(window_size, want):
	from convasr_amd import vad
	cfg = R.settings(16000, window_size, 2)
	assert (cfg['G'], cfg['S'], cfg['P']) == want and cfg['F'] == int(window_size * 16000)
	assert vad.settings(16000, window_size, 2) == cfg
	for a in range(4):
		assert vad.settings(8000, window_size, a) == R.settings(8000, window_size, a)
	assert vad.settings(8000, window_size, 3)['abs_thr'] == 0.05 and vad.settings(8000, window_size, 3)['rel_thr'] == 0.2
	assert vad.settings(8000, window_size, 1, window_size_dilate = 0.5)['P'] == int(0.5 / window_size) // 2 == R.settings(8000, window_size, 1, 0.5)['P']
	over = vad.settings(8000, window_size, 0, abs_thr = 0.3, min_gap = 2.0, speech_frames = 4, pad_frames = 0, percentile = 0.5, eps = 1e-3)
	assert over == dict(cfg, F = int(window_size * 8000), abs_thr = 0.3, rel_thr = 0.02, percentile = 0.5, eps = 1e-3, G = int(round(2.0 / window_size)), S = 4, P = 0)
	with pytest.raises(ValueError):
		vad.settings(8000, window_size, 4)
	with pytest.raises(ValueError):
		vad.settings(8000, 0.0001, 2)  # F = 0
	with pytest.raises(ValueError):
		vad.settings(8000, window_size, 2, pad_frames = -1)


def test_segment_samples_is_the_dataset_slice():
	from convasr_amd import vad
	N, sr = 1000, 8000
	signal = np.arange(2 * N).reshape(2, N)
	for begin, end in [(0.0, 0.01), (0.0123, 0.0456), (0.1, 0.12499), (0.1, 0.125), (0.1, 0.2), (0.12, 7.0), (0.0, N / sr), (0.03, 0.03)]:
		piece = signal[1, int(begin * sr):1 + int(end * sr)]  # datasets.py:261-262
		first, count = vad.segment_samples(begin, end, sr, N)
		assert (first, count) == R.segment_samples(begin, end, sr, N) == (int(begin * sr), len(piece)) and first + count <= N
		assert signal[1, first:first + count].tolist() == piece.tolist()


def test_upsample_and_silence_space_mask_on_the_cpu():
	from convasr_amd import models, vad
	gen = torch.Generator().manual_seed(0)
	speech = torch.rand(2, 37, generator = gen) < 0.5
	log_probs = torch.randn(2, 6, 91, generator = gen).log_softmax(dim = 1)
	up = vad.upsample(speech, log_probs)
	want = torch.nn.functional.interpolate(speech[:, None, :].float(), (91, )).squeeze(1).round().bool()
	assert up.dtype == torch.bool and up.shape == (2, 91) and torch.equal(up, want)
	blank, space = 5, 3
	got = models.silence_space_mask(log_probs, up, blank, space)
	assert got.dtype == torch.bool and got.shape == log_probs.shape
	for b in range(2):
		for t in range(91):
			silent = (not bool(up[b, t])) and int(log_probs[b, :, t].argmax()) == blank
			assert got[b, :, t].tolist() == [silent and c != space for c in range(6)]
	assert bool(got.any()) and not bool(got[:, space].any())


def test_argument_envelope_is_checked_before_any_launch():
	"""Every entry point of csrc/vad.hip refuses arguments outside its envelope with CONVASR_EINVAL and a message naming it.  The checks run
	before any launch and nothing is dereferenced, so this needs no GPU."""
	import ctypes
	from convasr_amd import _lib
	lib = _lib.load()
	p = ctypes.c_void_p(4096)  # any non-NULL, aligned value: never dereferenced
	f32, i16 = _lib.dtype_code(torch.float32), _lib.dtype_code(torch.int16)

	def refused(name, *args):
		return getattr(lib, name)(*args) == -1 and name.replace('convasr_', '').encode() in lib.convasr_last_error()

	for dt, C, N, F in [(f32, 9, 100, 10), (f32, 0, 100, 10), (i16, 1, 0, 10), (f32, 1, (1 << 28) + 1, 10), (i16, 1, 100, 0), (f32, 1, 100, 65537), (1, 1, 100, 10)]:
		assert refused('convasr_frame_peak', p, dt, C, N, F, p, None), (dt, C, N, F)
	assert refused('convasr_frame_peak', None, f32, 1, 100, 10, p, None)
	assert lib.convasr_frame_peak_tile(0) == -1 and lib.convasr_frame_peak_tile(65537) == -1
	assert [lib.convasr_frame_peak_tile(F) for F in (1, 16, 17, 160, 320, 480, 65536)] == [256, 256, 128, 16, 8, 8, 4]
	frames = lambda C, nF, nfull, G = 1, S = 1, P = 1, ws = 1 << 20: (p, p, C, nF, nfull, 0.1, 0.1, 1e-9, G, S, P, p, p, p, ws, None)
	for bad in (frames(9, 10, 10), frames(1, 0, 0), frames(1, 10, 0), frames(1, 10, 8), frames(1, 10, 11), frames(1, 10, 10, G = -1), frames(1, 10, 10, S = -1), frames(1, 10, 10, P = -1),
	            frames(2, 100, 100, ws = 512)):
		assert refused('convasr_vad_frames', *bad), bad
	assert lib.convasr_vad_frames_workspace_bytes(9, 10) == -1 and lib.convasr_vad_frames_workspace_bytes(1, 0) == -1 and lib.convasr_vad_segments_workspace_bytes(1, (1 << 28) + 1) == -1
	assert lib.convasr_vad_frames_workspace_bytes(2, 100) == 1024 and lib.convasr_vad_segments_workspace_bytes(2, 100) == 512
	for C, nF, M, ws in [(9, 10, 0, 1 << 20), (1, 0, 0, 1 << 20), (1, 10, 1, 1 << 20), (1, 10, -2, 1 << 20), (1, 1000, 0, 256)]:
		assert refused('convasr_vad_segments_count', p, p, C, nF, M, p, ws, None), (C, nF, M, ws)
	for C, nF, F, N, total in [(9, 10, 4, 40, 1), (1, 10, 0, 40, 1), (1, 10, 4, 41, 1), (1, 10, 4, 40, 0), (1, 10, 4, 40, 11)]:
		assert refused('convasr_vad_segments_write', p, C, nF, F, N, p, 1 << 20, total, p, p, p, None), (C, nF, F, N, total)
	seg = lambda *rows: (ctypes.c_int64 * (3 * len(rows[0])))(*[v for r in rows for v in r])
	gather = lambda host, B, N = 100, C = 2, Tpad = 128, dt = f32: (p, dt, C, N, host, p, B, p, Tpad, None)
	for bad in (gather(seg([0], [90], [11]), 1), gather(seg([0, 1], [0, 100], [100, 1]), 2), gather(seg([2], [0], [5]), 1), gather(seg([-1], [0], [5]), 1), gather(seg([0], [-1], [5]), 1),
	            gather(seg([0], [0], [0]), 1), gather(seg([0], [0], [100]), 1, Tpad = 99), gather(seg([0], [0], [5]), 0), gather(seg([0], [0], [5]), 1, C = 9), gather(seg([0], [0], [5]), 1, N = 0),
	            gather(None, 1), gather(seg([0], [0], [5]), 1, dt = 1)):
		assert refused('convasr_gather_segments', *bad)
