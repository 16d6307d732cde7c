"""diarization.npz: the reference's select_speaker (diarization.py:58-99), models.rle1d (models.py:777-785) and speaker_error
(diarization.py:175-201) on generated inputs, produced by importing the reference's own modules.

What the reference imports but is not installed is stubbed with empty modules (pyannote and its submodules with a dummy
DiarizationErrorRate, webrtcvad, audio, vis, librosa, soundfile, onnxruntime, apex, ...): none of it is reached by the three functions.

Inputs are not stored: each case keeps the recipe tests/_diar_synth.make() regenerates it from, its parameters, a SHA-256 of the input and the
two outputs run-length encoded (both are piecewise constant).  Cases: the reference's `ref` parameters (128 / 4096 / 4096, 0.05, 0.2) on 30 s
and 120 s of 8 kHz audio; odd windows 127 / 33 / 255 on N = 40001; N in {1, 2, 3, 100} under windows far larger than N; all zeros; two
identical channels; one channel silent; kernel_size_smooth_speaker 1 and 3 on a sign pattern with +1 0 -1, -1 0 +1, +1 0 +1 and a 0 at both
ends; thresholds exactly on values that occur; percentiles 0.5, 0.9 and 1.0 (the largest with int(p * L1) == L1).  speaker_error on hand-made
and random transcripts, both ignore_silence_and_overlapped_speech values, a given mapping.  rle1d on bool / int64 / float32 vectors.

    python tests/golden/make_golden_diarization.py <path of the reference checkout>          (writes next to this file)
"""
import importlib.machinery
import io
import json
import contextlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _diar_synth as S  # noqa: E402
import _diar_ref as R  # noqa: E402


def stub(name, **attrs):
	mod = types.ModuleType(name)
	mod.__spec__ = importlib.machinery.ModuleSpec(name, None)
	mod.__path__ = []
	for k, v in attrs.items():
		setattr(mod, k, v)
	sys.modules[name] = mod
	parent, _, child = name.rpartition('.')
	if parent:
		setattr(sys.modules[parent], child, mod)
	return mod


def import_reference(path):
	for name in ('pyannote', 'pyannote.core', 'pyannote.database', 'pyannote.database.util', 'pyannote.metrics', 'webrtcvad', 'audio', 'vis', 'librosa', 'librosa.filters',
	             'librosa.util', 'soundfile', 'onnxruntime', 'apex', 'scipy.io.wavfile'):
		try:
			importlib.import_module(name)
		except Exception:
			stub(name)
	try:
		importlib.import_module('pyannote.metrics.diarization')
	except Exception:
		stub('pyannote.metrics.diarization', DiarizationErrorRate = lambda *a, **k: None)
	sys.path.insert(0, path)
	import diarization
	import models
	return diarization, models


def select_cases():
	ref = S.REF_PARAMS
	small = dict(ref, kernel_size_smooth_silence = 16, kernel_size_smooth_signal = 64, kernel_size_smooth_speaker = 128)
	unit = dict(kernel_size_smooth_silence = 1, kernel_size_smooth_signal = 1, silence_absolute_threshold = 0.2, silence_relative_threshold = 0.5, eps = 1e-9, normalization_percentile = 0.9)
	pattern = [0, 1, 0, -1, -1, -1, 0, 1, 1, 0, 1, -1, 0, 0, 1, 0]
	levels = [[0.25, 0.125, 40], [0.5, 0.25, 40], [0.125, 0.5, 40], [0.25, 0.25, 40], [0.0, 0.25, 40], [0.5, 0.0, 40]]
	cases = [
		('ref_30s', ['call', 1, 240000], ref),
		('ref_120s', ['call', 2, 960000], ref),
		('odd_windows', ['call', 3, 40001], dict(ref, kernel_size_smooth_signal = 127, kernel_size_smooth_silence = 33, kernel_size_smooth_speaker = 255)),
		('zeros', ['zeros', 5000], ref),
		('identical_channels', ['identical', 4, 30000], ref),
		('one_channel_silent', ['one_silent', 5, 30000], ref),
		('signs_k1', ['signs', pattern], dict(unit, kernel_size_smooth_speaker = 1)),
		('signs_k3', ['signs', pattern], dict(unit, kernel_size_smooth_speaker = 3)),
		('signs_k2', ['signs', pattern], dict(unit, kernel_size_smooth_speaker = 2)),
		('thresholds_on_values', ['levels', levels], dict(kernel_size_smooth_silence = 3, kernel_size_smooth_signal = 3, kernel_size_smooth_speaker = 3, silence_absolute_threshold = 0.25,
		                                                  silence_relative_threshold = 0.5, eps = 0.0, normalization_percentile = 0.9)),
		('thresholds_on_values_eps', ['levels', levels], dict(kernel_size_smooth_silence = 5, kernel_size_smooth_signal = 1, kernel_size_smooth_speaker = 4, silence_absolute_threshold = 0.125,
		                                                      silence_relative_threshold = 0.25, eps = 1e-9, normalization_percentile = 0.5)),
		('all_even_small', ['call', 6, 20000], small),
	]
	cases += [(f'tiny_{n}', ['call', 10 + n, n], ref) for n in (1, 2, 3, 100)]
	cases += [(f'percentile_{p}', ['call', 6, 20000], dict(small, normalization_percentile = p)) for p in (0.5, 0.9, 1.0)]
	# a threshold placed exactly on a value of the eroded signal of a recording (the `<` is strict)
	x = S.make(['call', 8, 30000])
	eroded = R.sliding_min(R.sliding_max(np.abs(x), 16), 16)
	value = float(np.sort(eroded[0])[len(eroded[0]) // 2])
	assert value > 0 and int((eroded == np.float32(value)).sum()) > 0
	cases.append(('threshold_on_a_recorded_value', ['call', 8, 30000], dict(small, silence_absolute_threshold = value, silence_relative_threshold = 0.0)))
	return cases


def speaker_error_cases():
	seg = lambda b, e, s: dict(begin = b, end = e, speaker = s)
	a = [seg(0.0, 1.0, 1), seg(1.0, 2.5, 2), seg(3.0, 4.0, 1), seg(3.5, 5.0, 2)]
	b = [seg(0.1, 1.2, 2), seg(1.2, 2.4, 1), seg(2.9, 4.1, 2), seg(3.6, 5.5, 1)]
	pairs = [(a, a), (a, b), (b, a), (a, [seg(0.0, 5.0, 1)]), ([seg(0.0, 2.0, 1), seg(0.0, 2.0, 2)], [seg(0.0, 2.0, 1)]), ([seg(0.0, 1.0, 1)], [seg(0.0, 1.0, 2)])]
	pairs += [(S.random_transcript(20 + i, 60.0, 30), S.random_transcript(40 + i, 60.0, 30)) for i in range(4)]
	pairs.append((S.random_transcript(70, 600.0, 300), S.random_transcript(71, 600.0, 300)))
	cases = []
	for ref, hyp in pairs:
		for ignore in (True, False):
			for mapping in (None, [[0, 2, 1]], [[0, 1, 2]]):
				for sample_rate in (8000, 100):
					cases.append(dict(ref = ref, hyp = hyp, sample_rate = sample_rate, hyp_speaker_mapping = mapping, ignore_silence_and_overlapped_speech = ignore))
	return cases


def rle_inputs():
	rng = np.random.default_rng(9)
	return [np.array([True]), np.array([False, False, False]), np.array([True, False] * 50), rng.random(1000) < 0.1, rng.integers(0, 3, 1000).astype(np.int64),
	        np.array([7], dtype = np.int64), np.full(300, -5, dtype = np.int64), np.arange(257, dtype = np.int64) // 3, np.round(rng.random(500) * 3).astype(np.float32),
	        np.array([0.0, -0.0, 1.5, 1.5, 2.0], dtype = np.float32), np.tile(np.array([1.0, 2.0], dtype = np.float32), 64)]


def main():
	if len(sys.argv) < 2 and 'CONVASR_REFERENCE' not in os.environ:
		sys.exit('usage: make_golden_diarization.py <path of the reference checkout>   (or CONVASR_REFERENCE)')
	diarization, models = import_reference(sys.argv[1] if len(sys.argv) > 1 else os.environ['CONVASR_REFERENCE'])
	arrays, meta = {}, dict(select = [], speaker_error = [], n_rle = 0)
	for i, (name, spec, params) in enumerate(select_cases()):
		x = S.make(spec)
		speaker_id, mask = diarization.select_speaker(torch.from_numpy(x.copy()), **params)
		assert speaker_id.dtype == torch.float32 and mask.dtype == torch.bool
		_, arrays[f's{i}_id_lengths'], arrays[f's{i}_id_values'] = S.rle(speaker_id.numpy())
		for r in range(3):
			_, arrays[f's{i}_m{r}_lengths'], arrays[f's{i}_m{r}_values'] = S.rle(mask[r].numpy())
		meta['select'].append(dict(name = name, spec = spec, params = params, digest = S.digest(x)))
		print(name, x.shape, tuple(mask.shape), [len(arrays[f's{i}_m{r}_lengths']) for r in range(3)], flush = True)
	for c in speaker_error_cases():
		with contextlib.redirect_stdout(io.StringIO()):
			err, perm = diarization.speaker_error(c['ref'], c['hyp'], 2, sample_rate = c['sample_rate'], hyp_speaker_mapping = c['hyp_speaker_mapping'],
			                                      ignore_silence_and_overlapped_speech = c['ignore_silence_and_overlapped_speech'])
		meta['speaker_error'].append(dict(c, err = None if err != err else err, perm = list(perm)))
	for i, x in enumerate(rle_inputs()):
		starts, lengths, values = models.rle1d(torch.from_numpy(x))
		arrays[f'r{i}_x'], arrays[f'r{i}_starts'], arrays[f'r{i}_lengths'], arrays[f'r{i}_values'] = x, starts.numpy(), lengths.numpy(), values.numpy()
		meta['n_rle'] += 1
	path = os.path.join(HERE, 'diarization.npz')
	np.savez_compressed(path, meta = np.array(json.dumps(meta)), **arrays)
	print('diarization.npz', len(meta['select']), 'select_speaker cases,', len(meta['speaker_error']), 'speaker_error cases,', meta['n_rle'], 'rle1d cases,', os.path.getsize(path) // 1024, 'KB')


if __name__ == '__main__':
	main()
