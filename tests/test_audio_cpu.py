"""The host side of convasr_amd.audio against the reference's own read_audio (tests/golden/audio_read.npz, written by
tests/golden/make_golden_audio.py with sample_rate = None): decode, offset / duration slice, the s2f scaling, the mono mean the kernel takes,
the empty result, the errors.  No GPU: everything goes through audio.decode_audio and the one-liners."""
import json
import os

import numpy as np
import pytest
import torch

import _resample_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope = 'module')
def cases():
	g = np.load(os.path.join(GOLDEN, 'audio_read.npz'), allow_pickle = False)
	return [(m, g[m['name']]) for m in json.loads(str(g['meta']))]


def decode(audio, m, **extra):
	kwargs = {k: v for k, v in m['kwargs'].items() if k != 'mono'}
	return audio.decode_audio(os.path.join(GOLDEN, m['file']), None, **dict(kwargs, **extra))


def test_decode_and_slice_equal_the_references(cases, capsys):
	"""decode_audio returns the samples as stored, (T, C); what read_audio does to them afterwards on the GPU is restated here in numpy (s2f,
	the ascending-order fp32 mean) and must give the reference's arrays bit for bit -- which pins both rules for the kernel."""
	from convasr_amd import audio
	assert len(cases) == 15
	for m, want in cases:
		signal, rate = decode(audio, m)
		assert rate == m['sample_rate'], m['name']
		assert signal.ndim == 2 and signal.dtype in (np.int16, np.float32), m['name']
		got = signal.T
		if signal.dtype == np.int16 and m['kwargs'].get('dtype') != 'int16':
			got = R.decode_int16(signal)
			assert np.array_equal(got, audio.s2f(signal.T)) and audio.s2f(signal.T).dtype == np.float32
		if m['kwargs'].get('mono') and got.shape[0] > 1:
			got = R.mono_mean(got)
		assert got.dtype == want.dtype and got.shape == want.shape == tuple(m['shape']) and np.array_equal(got, want), m['name']
	assert 'Error when reading' in capsys.readouterr().out  # the unreadable path reports like the reference


def test_slices_follow_the_int_rule_at_the_files_own_rate(cases):
	from convasr_amd import audio
	whole = audio.decode_audio(os.path.join(GOLDEN, 'audio_stereo.wav'), None)[0]
	assert whole.shape == (331, 2) and whole.dtype == np.int16
	by_name = {m['name']: (m, a) for m, a in cases}
	for name, lo, hi in (('slice', 98, 235), ('offset_only', 249, 331), ('slice_raw', 98, 235)):
		signal, _ = decode(audio, by_name[name][0])
		assert np.array_equal(signal, whole[lo:hi]), name
	assert decode(audio, by_name['duration_only'][0])[0].shape == (93, 1)
	raw = audio.decode_audio(None, None, raw_bytes = whole.astype('<i2').tobytes(), raw_sample_rate = 8000, raw_num_channels = 2)
	assert raw[1] == 8000 and np.array_equal(raw[0], whole)


def test_unreadable_and_empty_files_give_the_empty_result(tmp_path, capsys):
	from convasr_amd import audio
	signal, rate = audio.decode_audio(str(tmp_path / 'missing.wav'), 16000)
	assert signal.shape == (0, 1) and signal.dtype == np.float32 and rate == 16000
	(tmp_path / 'garbage.wav').write_bytes(b'not a wav file at all')
	signal, rate = audio.decode_audio(str(tmp_path / 'garbage.wav'), 8000)
	assert signal.shape == (0, 1) and rate == 8000
	(tmp_path / 'empty.raw').write_bytes(b'')
	signal, rate = audio.decode_audio(str(tmp_path / 'empty.raw'), 8000, raw_sample_rate = 8000, raw_num_channels = 2)
	assert signal.shape == (0, 2) and signal.dtype == np.int16 and rate == 8000
	capsys.readouterr()


@pytest.mark.parametrize('backend', ['soundfile', 'ffmpeg', 'sox'])
def test_other_backends_are_refused_by_name(backend):
	from convasr_amd import audio
	wav = os.path.join(GOLDEN, 'audio_stereo.wav')
	with pytest.raises(NotImplementedError, match = backend):
		audio.decode_audio(wav, None, backend = backend)
	with pytest.raises(NotImplementedError, match = backend):
		audio.read_audio(wav, 16000, backend = backend)
	with pytest.raises(NotImplementedError, match = 'ffmpeg'):
		audio.decode_audio('speech.mp3', None)


def test_one_liners(tmp_path):
	from convasr_amd import audio
	assert audio.is_audio('a/b.WAV') and audio.is_audio('x.opus') and not audio.is_audio('x.txt') and not audio.is_audio('wav')
	x = np.array([[-32768, -1, 0, 1, 32767]], dtype = np.int16)
	f = audio.s2f(x)
	assert f.dtype == np.float32 and f[0, 4] == 1.0 and f[0, 0] == np.float32(-32768) / np.float32(32767)
	assert np.array_equal(audio.f2s(f)[0, 1:], x[0, 1:]) and audio.f2s(f).dtype == np.int16
	assert audio.compute_duration(os.path.join(GOLDEN, 'audio_stereo.wav')) == 331 / 8000
	assert audio.compute_duration(os.path.join(GOLDEN, 'audio_mono.wav')) == 257 / 44100
	assert audio.compute_duration(os.path.join(GOLDEN, 'audio_pcm.raw'), raw_sample_rate = 8000, raw_num_channels = 2) == 331 / 8000
	# write_audio (scipy backend) and back: f2s truncates towards zero, so the samples come back within one step
	signal = torch.from_numpy(audio.s2f(audio.decode_audio(os.path.join(GOLDEN, 'audio_stereo.wav'), None)[0].T))
	path = audio.write_audio(str(tmp_path / 'out.wav'), signal, 8000)
	back, rate = audio.decode_audio(path, None)
	assert rate == 8000 and back.dtype == np.int16 and np.array_equal(back, audio.f2s(signal.t().numpy()))
	assert audio.decode_audio(audio.write_audio(str(tmp_path / 'mono.wav'), signal, 8000, mono = True), None)[0].shape == (331, 1)
	with pytest.raises(NotImplementedError, match = 'soundfile'):
		audio.write_audio(str(tmp_path / 'out.flac'), signal, 8000, backend = 'soundfile')


def test_resample_envelope_is_checked_before_any_launch():
	"""The C entry point refuses C = 9 and a ratio whose table exceeds 2^22 entries with CONVASR_EUNSUPPORTED before it touches a device (so
	this runs without one), and names odd arguments."""
	import ctypes
	from convasr_amd import _lib, ops
	lib = _lib.load()
	p = ctypes.c_void_p(4096)  # any non-NULL value: never dereferenced
	taps = lib.convasr_resample_taps(8000, 16000, 64.0, ops.RESAMPLE_ROLLOFF)
	assert taps == 136 and lib.convasr_resample_taps(44100, 16000, 64.0, ops.RESAMPLE_ROLLOFF) == 374 and lib.convasr_resample_taps(16000, 16000, 64.0, 0.9) == 0
	assert lib.convasr_resample(p, _lib.I16, 100, 9, 0, p, taps, 8000, 16000, p, 200, 0, None) == -3 and b'channels' in lib.convasr_last_error()
	assert lib.convasr_resample_taps(44101, 16000, 64.0, ops.RESAMPLE_ROLLOFF) == -3 and b'2^22' in lib.convasr_last_error()
	assert lib.convasr_resample(p, _lib.F32, 100, 1, 0, p, 374, 44101, 16000, p, ops.resample_out_len(100, 44101, 16000), 0, None) == -3
	assert lib.convasr_resample(p, _lib.I16, 1 << 39, 2, 0, p, taps, 8000, 16000, p, 1 << 40, 0, None) == -3 and b'2^40' in lib.convasr_last_error()
	assert lib.convasr_resample(p, _lib.I16, 100, 2, 0, p, taps, 8000, 16000, p, 199, 0, None) == -1 and b'T_out' in lib.convasr_last_error()
	assert lib.convasr_resample(p, _lib.BF16, 100, 2, 0, p, taps, 8000, 16000, p, 200, 0, None) == -1
	assert lib.convasr_resample(p, _lib.I16, 100, 2, 0, p, taps + 1, 8000, 16000, p, 200, 0, None) == -1
	assert lib.convasr_resample(p, _lib.I16, 100, 2, 0, p, taps, 0, 16000, p, 200, 0, None) == -1
	assert lib.convasr_resample(p, _lib.I16, 0, 2, 0, p, taps, 8000, 16000, p, 0, 0, None) == 0  # nothing to do, nothing launched
	assert lib.convasr_resample_tile() == 256 and lib.convasr_resample_out_len(4097, 44100, 16000) == 1487 and lib.convasr_resample_out_len(-1, 8000, 16000) == -1
	with pytest.raises(_lib.ConvasrHipError):
		ops.resample_table(44101, 16000)
	with pytest.raises(_lib.ConvasrHipError):
		ops.resample(torch.zeros(2, 100), 8000, 16000)  # a CPU tensor: there is no CPU path
