"""The numpy restatement of the diarization ops (tests/_diar_ref.py) against the reference's outputs (tests/golden/diarization.npz), exactly;
the host-side pieces of convasr_amd.diarization; the envelope errors that need no device."""
import os

import numpy as np
import pytest
import torch

import _diar_ref as R
import _diar_synth as S

GOLDEN = S.load_golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'diarization.npz'))


@pytest.mark.parametrize('case', GOLDEN['select'], ids = [c[0] for c in GOLDEN['select']])
def test_restatement_equals_the_reference_select_speaker(case):
	name, spec, params, digest, speaker_id, mask = case
	x = S.make(spec)
	assert S.digest(x) == digest, 'the input generator drifted: regenerate tests/golden/diarization.npz'
	got_id, got_mask = R.select_speaker(x, **params)
	assert got_id.dtype == np.float32 and got_mask.dtype == bool
	assert got_id.shape == speaker_id.shape and got_mask.shape == mask.shape
	assert np.array_equal(got_id, speaker_id) and np.array_equal(got_mask, mask)


def test_golden_lengths_grow_with_even_windows():
	by_name = {c[0]: c for c in GOLDEN['select']}
	assert by_name['ref_30s'][5].shape == (3, 240002) and by_name['odd_windows'][5].shape == (3, 40001) and by_name['tiny_1'][5].shape == (3, 3)


def test_restatement_equals_the_reference_speaker_error():
	assert len(GOLDEN['speaker_error']) >= 100
	for c in GOLDEN['speaker_error']:
		err, perm = R.speaker_error(c['ref'], c['hyp'], sample_rate = c['sample_rate'], hyp_speaker_mapping = c['hyp_speaker_mapping'],
		                            ignore_silence_and_overlapped_speech = c['ignore_silence_and_overlapped_speech'])
		assert perm == c['perm']
		assert (err != err) if c['err'] is None else err == c['err'], (err, c['err'])


def test_rle_of_the_generator_equals_the_reference():
	for x, starts, lengths, values in GOLDEN['rle']:
		s, l, v = S.rle(x)
		assert np.array_equal(s, starts) and np.array_equal(l, lengths) and np.array_equal(v, values) and v.dtype == values.dtype


def test_sliding_max_restatement_against_a_tap_loop():
	rng = np.random.default_rng(0)
	for L, K in [(1, 1), (1, 8), (5, 2), (17, 3), (100, 7), (100, 64), (100, 1000), (1000, 128), (999, 129)]:
		x = rng.integers(-5, 6, size = (2, L)).astype(np.float32)
		p = np.pad(x, ((0, 0), (K // 2, K // 2)), constant_values = -np.inf)
		want = np.stack([p[:, i:i + K].max(axis = 1) for i in range(p.shape[1] - K + 1)], axis = 1)
		assert np.array_equal(R.sliding_max(x, K), want), (L, K)
		assert R.sliding_max(x, K).shape[1] == R.out_len(L, K)


def test_convert_speaker_id():
	from convasr_amd import diarization as D
	bipole = torch.tensor([1.0, 0.0, -1.0])
	assert D.convert_speaker_id(bipole, from_bipole = True).tolist() == [1.0, 0.0, 2.0]
	assert D.convert_speaker_id(torch.tensor([1.0, 0.0, 2.0]), to_bipole = True).tolist() == [1.0, 0.0, -1.0]


def test_speaker_mask_equals_the_restatement():
	from convasr_amd import diarization as D
	tr = S.random_transcript(3, 20.0, 12)
	got = D.speaker_mask(tr, 2, 20.0, 100)
	assert got.dtype == torch.bool and np.array_equal(got.numpy(), R.speaker_mask(tr, 2, 20.0, 100))
	assert D.compute_duration(tr, [dict(begin = 0.0, end = 25.0, speaker = 1)]) == 25.0


def test_segments_from_runs():
	from convasr_amd import diarization as D
	segs = D.segments_from_runs(2, [0, 4000, 12000], [4000, 8000, 4000], [False, True, False], 8000, audio_path = 'a.wav')
	assert segs == [dict(audio_path = 'a.wav', begin = 0.5, end = 1.5, speaker = 2, speaker_name = 'B')]
	assert list(segs[0]) == ['audio_path', 'begin', 'end', 'speaker', 'speaker_name']
	assert D.segments_from_runs(1, [0], [10], [True], 10) == [dict(begin = 0.0, end = 1.0, speaker = 1, speaker_name = 'A')]
	assert D.default_speaker_names[:4] == '_ABC'


def test_envelope_errors_that_need_no_device():
	from convasr_amd import _lib, diarization as D, models, ops
	x = torch.zeros(2, 100)
	kw = dict(kernel_size_smooth_silence = 5, kernel_size_smooth_signal = 5, kernel_size_smooth_speaker = 5)
	for bad, text in [(torch.zeros(3, 100), '(2, N)'), (torch.zeros(100), '(2, N)'), (torch.zeros(2, 0), '1 to'), (torch.zeros(2, 100, dtype = torch.float64), 'float32')]:
		with pytest.raises(ValueError, match = text.replace('(', r'\(').replace(')', r'\)')):
			D.select_speaker(bad, **kw)
	for name in kw:
		for K in (0, 16385, 2.5):
			with pytest.raises(ValueError, match = name + '.*16384'):
				D.select_speaker(x, **dict(kw, **{name: K}))
	with pytest.raises(ValueError, match = 'normalization_percentile'):
		D.select_speaker(x, normalization_percentile = 0.001, **kw)
	with pytest.raises(ValueError, match = 'normalization_percentile'):
		D.select_speaker(x, normalization_percentile = 1.5, **kw)
	# a CPU tensor is refused before any launch: there is no host path
	with pytest.raises(_lib.ConvasrHipError, match = 'cpu'):
		D.select_speaker(x, **kw)
	with pytest.raises(_lib.ConvasrHipError, match = 'cpu'):
		D.diarize(x, 8000)
	for fn in (lambda: models.rle1d(torch.zeros(5)), lambda: ops.sliding_max(x, 3), lambda: ops.kth_value(x, 1), lambda: ops.sign_prefix_sum(x),
	           lambda: ops.speaker_error_counts(torch.zeros(3, 4, dtype = torch.bool), torch.zeros(3, 4, dtype = torch.bool), [[0, 1, 2]])):
		with pytest.raises(_lib.ConvasrHipError, match = 'cpu'):
			fn()
	with pytest.raises(ValueError, match = 'num_speakers'):
		D.speaker_error([], [], 3)


def test_c_abi_envelope_is_checked_before_any_launch():
	"""The entry points refuse what lies outside their envelope with an error code and a message naming the limit (no GPU is touched)."""
	import ctypes
	from convasr_amd import _lib
	lib = _lib.load()
	p = ctypes.c_void_p(4096)  # any non-NULL, aligned value: never dereferenced
	err = lambda: lib.convasr_last_error().decode()
	assert lib.convasr_sliding_max(p, p, 2, 100, 16385, 0, None) < 0 and '16384' in err()
	assert lib.convasr_sliding_max(p, p, 2, 0, 3, 0, None) < 0 and 'length' in err()
	assert lib.convasr_sliding_max(p, p, 2, (1 << 28) + 1, 3, 0, None) < 0 and str(1 << 28) in err()
	assert lib.convasr_sliding_max(p, p, 2, 100, 3, 4, None) < 0 and 'flags' in err()
	assert lib.convasr_sliding_max_out_len(100, 4096) == 101 and lib.convasr_sliding_max_out_len(100, 127) == 100 and lib.convasr_sliding_max_out_len(100, 0) == -1
	assert lib.convasr_sliding_max_tile(128) == 7936 - 127 and lib.convasr_sliding_max_tile(4096) == 31744 - 4095
	assert lib.convasr_scan_tile() == 2048
	assert lib.convasr_kth_value(p, p, p, 1 << 20, 2, 100, 0, None) < 0 and 'k = 0' in err()
	assert lib.convasr_kth_value(p, p, p, 1 << 20, 2, 100, 101, None) < 0 and 'k = 101' in err()
	assert lib.convasr_kth_value(p, p, p, 16, 2, 100, 5, None) < 0 and 'workspace' in err()
	assert lib.convasr_select_speaker_out_len(240000, 4096, 128, 4096) == 240002 and lib.convasr_select_speaker_out_len(40001, 33, 127, 255) == 40001
	assert lib.convasr_select_speaker_out_len(100, 4096, 128, 16385) == -1 and '16384' in err()
	two_hours = 2 * 3600 * 16000
	assert 0 < lib.convasr_select_speaker_workspace_bytes(two_hours, 4096, 128, 4096) < 40 * two_hours
	assert lib.convasr_select_speaker(p, p, p, p, 1 << 40, 100, 5, 5, 5, 0.1, 0.1, 1e-9, 0, None) < 0 and 'normalization_percentile' in err()
	assert lib.convasr_select_speaker(p, p, p, p, 16, 100, 5, 5, 5, 0.1, 0.1, 1e-9, 50, None) < 0 and 'workspace' in err()
	assert lib.convasr_select_speaker(p, p, p, p, 1 << 40, (1 << 28) + 1, 5, 5, 5, 0.1, 0.1, 1e-9, 50, None) < 0 and str(1 << 28) in err()
	assert lib.convasr_rle1d_count(p, 3, 0, 100, p, 1 << 20, None) < 0 and 'bytes' in err()
	assert lib.convasr_rle1d_count(p, 8, 1, 100, p, 1 << 20, None) < 0
	assert lib.convasr_rle1d_count(p, 1, 0, 0, p, 1 << 20, None) < 0 and 'elements' in err()
	assert lib.convasr_rle1d_write(p, 1, 0, 100, p, 1 << 20, 101, p, p, p, None) < 0 and 'runs' in err()
	perms = (ctypes.c_int32 * 3)(0, 1, 3)
	assert lib.convasr_speaker_error_counts(p, p, perms, 1, 100, p, p, 1 << 20, None) < 0 and 'row 3' in err()
	assert lib.convasr_speaker_error_counts(p, p, perms, 9, 100, p, p, 1 << 20, None) < 0 and '8' in err()
