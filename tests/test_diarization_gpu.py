"""convasr_amd.diarization on the GPU: against every case of the reference's outputs (tests/golden/diarization.npz) exactly -- values, dtypes,
shapes -- and against the numpy restatement (tests/_diar_ref.py, itself held to the same goldens by tests/test_diarization.py) on inputs too
long for a fixture, on lengths that straddle every tile the kernels use, and op by op."""
import os

import numpy as np
import pytest
import torch

import _diar_ref as R
import _diar_synth as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = S.load_golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'diarization.npz'))


def gpu_select(x, **params):
	from convasr_amd import diarization as D
	speaker_id, mask = D.select_speaker(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), **params)
	assert speaker_id.dtype == torch.float32 and mask.dtype == torch.bool and speaker_id.device == mask.device == torch.device(DEV)
	return speaker_id.cpu().numpy(), mask.cpu().numpy()


def check_select(x, **params):
	got_id, got_mask = gpu_select(x, **params)
	want_id, want_mask = R.select_speaker(x, **params)
	assert got_id.shape == want_id.shape and got_mask.shape == want_mask.shape, (x.shape, params)
	assert np.array_equal(got_id, want_id) and np.array_equal(got_mask, want_mask), (x.shape, params)
	return got_id, got_mask


@pytest.mark.parametrize('case', GOLDEN['select'], ids = [c[0] for c in GOLDEN['select']])
def test_select_speaker_equals_the_reference(case):
	name, spec, params, digest, speaker_id, mask = case
	x = S.make(spec)
	assert S.digest(x) == digest, 'the input generator drifted: regenerate tests/golden/diarization.npz'
	got_id, got_mask = gpu_select(x, **params)
	assert got_id.shape == speaker_id.shape and got_mask.shape == mask.shape
	assert np.array_equal(got_id, speaker_id) and np.array_equal(got_mask, mask)


def test_rle1d_equals_the_reference():
	from convasr_amd import models
	for x, starts, lengths, values in GOLDEN['rle']:
		s, l, v = models.rle1d(torch.from_numpy(x).to(DEV))
		assert s.dtype == l.dtype == torch.int64 and v.dtype == torch.from_numpy(x).dtype and s.device == torch.device(DEV)
		assert np.array_equal(s.cpu().numpy(), starts) and np.array_equal(l.cpu().numpy(), lengths) and np.array_equal(v.cpu().numpy(), values)


def test_speaker_error_equals_the_reference():
	from convasr_amd import diarization as D
	for c in GOLDEN['speaker_error']:
		err, perm = D.speaker_error(c['ref'], c['hyp'], 2, sample_rate = c['sample_rate'], hyp_speaker_mapping = c['hyp_speaker_mapping'],
		                            ignore_silence_and_overlapped_speech = c['ignore_silence_and_overlapped_speech'], device = DEV)
		assert isinstance(err, float) and perm == c['perm']
		assert (err != err) if c['err'] is None else err == c['err'], (err, c['err'])


def test_speaker_error_counts_against_the_restatement():
	from convasr_amd import ops
	rng = np.random.default_rng(5)
	for n in (1, 63, 4096, 4097, 1_000_003):
		rm, hm = rng.random((3, n)) < 0.4, rng.random((3, n)) < 0.4
		perms = [[0, 1, 2], [0, 2, 1], [0, 0, 1], [0, 2, 2]]
		got = ops.speaker_error_counts(torch.from_numpy(rm).to(DEV), torch.from_numpy(hm).to(DEV), perms)
		assert got.dtype == torch.int64 and got.shape == (4, 7)
		assert got.cpu().tolist() == [R.speaker_error_counts(rm, hm, p) for p in perms]


@pytest.mark.parametrize('seconds', [600, 3600])
def test_long_recordings_against_the_restatement(seconds):
	x = S.call_signal(100 + seconds, seconds * 8000)
	got_id, got_mask = check_select(x, **S.REF_PARAMS)
	assert got_mask.shape == (3, seconds * 8000 + 2) and len(S.rle(got_mask[1])[0]) > seconds // 20


def test_two_hours_at_16_khz_and_beyond_against_the_restatement():
	"""N = 2^27 + 4097 samples per channel (2.3 hours at 16 kHz, half the envelope): the signal is 1 GiB, the second channel's row starts past
	2^29 bytes and the workspace passes 2^31 bytes several times over, so every offset that must be 64-bit is exercised.  The input is a
	10-minute recording repeated (generating it sample by sample is host time only)."""
	from convasr_amd import ops
	N = (1 << 27) + 4097
	base = S.call_signal(55, 600 * 8000)
	x = np.ascontiguousarray(np.tile(base, (1, N // base.shape[1] + 1))[:, :N])
	t = torch.from_numpy(x).to(DEV)
	want = R.sliding_max(np.abs(x), 4096)
	got = ops.sliding_max(t, 4096, absolute = True).cpu().numpy()
	assert got.shape == want.shape == (2, N + 1) and np.array_equal(got, want)
	del got, want
	speaker_id, mask = __import__('convasr_amd').diarization.select_speaker(t, **S.REF_PARAMS)
	want_id, want_mask = R.select_speaker(x, **S.REF_PARAMS)
	assert tuple(mask.shape) == want_mask.shape == (3, N + 2)
	assert np.array_equal(speaker_id.cpu().numpy(), want_id) and np.array_equal(mask.cpu().numpy(), want_mask)
	starts, lengths, values = ops.rle1d(mask[2])
	ws, wl, wv = S.rle(want_mask[2])
	assert np.array_equal(starts.cpu().numpy(), ws) and np.array_equal(lengths.cpu().numpy(), wl) and np.array_equal(values.cpu().numpy(), wv)


def test_random_windows_on_lengths_around_every_tile():
	from convasr_amd import ops
	rng = np.random.default_rng(11)
	windows = [1, 2, 3, 64, 127, 128, 2047, 2048, 2049, 4096, 8191, 16383, 16384] + [int(k) for k in rng.integers(1, 16385, size = 6)]
	for n_case, K in enumerate(windows):
		tile = ops.sliding_max_tile(K)
		assert 1 <= tile <= 31744  # (the library's own answer decides the lengths below)
		for n in (1, 2, 3):
			for delta in (-1, 0, 1):
				L = n * tile + delta  # of the OUTPUT; the input is shorter by one for an even window
				Lin = L - (1 - K % 2)
				if Lin < 1 or (n == 3 and n_case % 3):
					continue
				x = S.pcm_to_float(rng.integers(-3000, 3001, size = (2, Lin)).astype(np.int16))
				for kw, want in ((dict(absolute = True), R.sliding_max(np.abs(x), K)), (dict(minimum = True), R.sliding_min(x, K)), ({}, R.sliding_max(x, K))):
					got = ops.sliding_max(torch.from_numpy(x).to(DEV), K, **kw).cpu().numpy()
					assert got.shape == want.shape == (2, L) and np.array_equal(got, want), (K, Lin, kw)
	# whole select_speaker calls with random windows (odd and even, 1 to 16384) on random lengths
	for _ in range(8):
		ks = [int(k) for k in rng.integers(1, 16385, size = 3)]
		N = int(rng.integers(1, 200_000))
		x = S.call_signal(int(rng.integers(1 << 30)), N)
		check_select(x, kernel_size_smooth_silence = ks[0], kernel_size_smooth_signal = ks[1], kernel_size_smooth_speaker = ks[2], silence_absolute_threshold = 0.05,
		             silence_relative_threshold = 0.2)


def test_kth_value_against_partition():
	from convasr_amd import ops
	rng = np.random.default_rng(12)
	for L in (1, 2, 100, 8191, 8193, 300_001):
		for x in (np.abs(S.pcm_to_float(rng.integers(-32768, 32768, size = (2, L)).astype(np.int16))), rng.random((2, L)).astype(np.float32) ** 8,
		          np.zeros((2, L), dtype = np.float32), np.full((2, L), 0.25, dtype = np.float32)):
			t = torch.from_numpy(x).to(DEV)
			for k in sorted({1, L, (L + 1) // 2, max(1, int(0.9 * L)), min(L, 2)}):
				got = ops.kth_value(t, k)
				assert got.dtype == torch.float32 and got.shape == (2,)
				assert np.array_equal(got.cpu().numpy(), R.kth_value(x, k)), (L, k)
	x = rng.random((5, 1000)).astype(np.float32)
	assert np.array_equal(ops.kth_value(torch.from_numpy(x).to(DEV), 500).cpu().numpy(), R.kth_value(x, 500))


def test_sign_prefix_sum_around_the_scan_tile():
	from convasr_amd import ops
	SCAN_TILE = ops.scan_tile()  # elements per workgroup of the prefix sums, asked of the library so the lengths follow it
	rng = np.random.default_rng(13)
	for L in (1, 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE, 1024 * SCAN_TILE - 1, 1024 * SCAN_TILE + 1, 1025 * SCAN_TILE + 7, 5_000_000):
		d = rng.integers(0, 3, size = (2, L)).astype(np.float32)
		if L > 10 * SCAN_TILE:
			d[0, : L // 2] = 2  # a long one-sided stretch: the sums of many tiles add up
		got = ops.sign_prefix_sum(torch.from_numpy(d).to(DEV))
		assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), R.sign_prefix_sum(d)), L


def test_rle1d_on_long_masks():
	from convasr_amd import models, ops
	SCAN_TILE = ops.scan_tile()
	rng = np.random.default_rng(14)
	n = 10_000_000
	few = np.zeros(n, dtype = bool)
	for b in np.sort(rng.integers(0, n, size = 100)).reshape(-1, 2):
		few[b[0]:b[1]] = True
	many = rng.random(n) < 0.05
	for x in (few, many, many.astype(np.int64) * 3 - 1, np.cumsum(many).astype(np.float32) % 7, many.astype(np.int32), many.astype(np.int16), np.zeros(n, dtype = bool)):
		s, l, v = models.rle1d(torch.from_numpy(x).to(DEV))
		ws, wl, wv = S.rle(x)
		assert v.dtype == torch.from_numpy(x).dtype and len(ws) == len(s)
		assert np.array_equal(s.cpu().numpy(), ws) and np.array_equal(l.cpu().numpy(), wl) and np.array_equal(v.cpu().numpy(), wv)
	assert 50 <= len(S.rle(few)[0]) <= 120 and 500_000 <= len(S.rle(many)[0]) <= 2_000_000
	for n in (1, 2, SCAN_TILE, SCAN_TILE + 1):
		x = np.arange(n) % 2 == 0
		s, l, v = models.rle1d(torch.from_numpy(x).to(DEV))
		assert s.cpu().tolist() == list(range(n)) and l.cpu().tolist() == [1] * n and v.cpu().tolist() == x.tolist()
	with pytest.raises(ValueError):
		models.rle1d(torch.zeros(2, 2, device = DEV))
	with pytest.raises(ValueError):
		models.rle1d(torch.zeros(0, device = DEV))
	with pytest.raises(ValueError):
		models.rle1d(torch.zeros(4, dtype = torch.float64, device = DEV))


def test_diarize_end_to_end():
	from convasr_amd import diarization as D
	from convasr_amd.transcript_generators import Transcript
	x = S.call_signal(21, 60 * 8000)
	transcript = D.diarize(torch.from_numpy(x).to(DEV), 8000, audio_path = 'call.wav')
	_, mask = R.select_speaker(x, **S.REF_PARAMS)
	want = [seg for speaker in (1, 2) for seg in D.segments_from_runs(speaker, *[a.tolist() for a in S.rle(mask[speaker])], 8000, audio_path = 'call.wav')]
	assert isinstance(transcript, Transcript) and len(transcript) > 10 and list(transcript) == want
	assert all(type(s['begin']) is float and s['speaker_name'] == ' AB'[s['speaker']] for s in transcript)
	assert [s['speaker'] for s in transcript] == sorted(s['speaker'] for s in transcript)
	bare = D.diarize(torch.from_numpy(x).to(DEV), 8000)
	assert [dict(s, audio_path = 'call.wav') for s in bare] == want and 'audio_path' not in bare[0]
	# a non-contiguous signal is made contiguous
	wide = torch.from_numpy(np.ascontiguousarray(np.repeat(x, 2, axis = 1))).to(DEV)
	assert list(D.diarize(wide[:, ::2], 8000, audio_path = 'call.wav')) == want


def test_two_calls_in_a_row_on_different_lengths():
	a, b = S.call_signal(31, 300_000), S.call_signal(32, 77_777)
	first = gpu_select(a, **S.REF_PARAMS)
	second = gpu_select(b, **S.REF_PARAMS)
	again = gpu_select(a, **S.REF_PARAMS)
	for got, x in ((first, a), (second, b), (again, a)):
		want = R.select_speaker(x, **S.REF_PARAMS)
		assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
