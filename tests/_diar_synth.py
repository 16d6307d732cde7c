"""Synthetic two-channel call recordings for the diarization tests and their golden generator: int16 PCM from numpy.random.default_rng(seed),
converted to float32 by dividing by float32 32767 (so values tie often).  Alternating speaker turns of 0.25-4 s, 10 % cross-talk on the
other channel, 25 % of the turns are pauses, 10 % overlapped speech, a noise floor.  digest() is what the goldens store of an input."""
import hashlib

import numpy as np


def call_signal(seed, n, sample_rate = 8000):
	"""(2, n) float32."""
	rng = np.random.default_rng(seed)
	pcm = rng.integers(-40, 41, size = (2, n)).astype(np.float64)  # the noise floor
	t, speaker = 0, int(rng.integers(0, 2))
	while t < n:
		length = int(rng.uniform(0.25, 4.0) * sample_rate)
		end = min(n, t + length)
		kind = rng.random()
		if kind >= 0.25:  # not a pause
			level = rng.uniform(3000, 20000)
			voice = rng.normal(0.0, level, size = end - t) * (0.6 + 0.4 * np.sin(np.arange(end - t) * (2 * np.pi * 3.1 / sample_rate)))
			pcm[speaker, t:end] += voice
			pcm[1 - speaker, t:end] += 0.1 * voice  # cross-talk
			if kind >= 0.9:  # overlapped speech
				pcm[1 - speaker, t:end] += rng.normal(0.0, rng.uniform(3000, 20000), size = end - t)
		t, speaker = end, 1 - speaker
	return pcm_to_float(np.clip(np.rint(pcm), -32768, 32767).astype(np.int16))


def pcm_to_float(pcm):
	return (pcm.astype(np.float32) / np.float32(32767)).astype(np.float32)


def digest(signal):
	a = np.ascontiguousarray(signal, dtype = np.float32)
	return hashlib.sha256(str(a.shape).encode() + a.tobytes()).hexdigest()


def sign_pattern_signal(signs):
	"""(2, n) float32 whose channel-0-minus-channel-1 sign is `signs` (+1 / 0 / -1), both channels loud enough not to be silent."""
	s = np.asarray(signs)
	x = np.full((2, len(s)), 0.5, dtype = np.float32)
	x[0, s > 0] = 0.75
	x[1, s < 0] = 0.75
	x[1, 1::2] *= -1  # the sign of a sample must not matter
	return x


def random_transcript(seed, duration, n_segments):
	rng = np.random.default_rng(seed)
	out = []
	for _ in range(n_segments):
		begin = float(rng.uniform(0, duration * 0.95))
		out.append(dict(begin = round(begin, 3), end = round(min(duration, begin + float(rng.uniform(0.05, duration / 5))), 3), speaker = int(rng.integers(1, 3))))
	return out


def rle(a):
	"""numpy run-length encoding -> (starts, lengths, values)."""
	a = np.asarray(a)
	starts = np.concatenate(([0], np.flatnonzero(a[1:] != a[:-1]) + 1)).astype(np.int64)
	lengths = np.diff(np.concatenate((starts, [len(a)]))).astype(np.int64)
	return starts, lengths, a[starts]


def unrle(lengths, values):
	return np.repeat(np.asarray(values), np.asarray(lengths))


def levels_signal(levels):
	"""levels: [(level of channel 0, level of channel 1, samples), ...] -> (2, n) float32 of constant stretches."""
	return np.concatenate([np.stack([np.full(n, a, dtype = np.float32), np.full(n, b, dtype = np.float32)]) for a, b, n in levels], axis = 1)


def make(spec):
	"""The input of a golden case from its stored recipe [kind, *args]."""
	kind, args = spec[0], spec[1:]
	if kind == 'call':
		return call_signal(*args)
	if kind == 'zeros':
		return np.zeros((2, args[0]), dtype = np.float32)
	if kind == 'identical':
		x = call_signal(*args)
		x[1] = x[0]
		return x
	if kind == 'one_silent':
		x = call_signal(*args)
		x[1] = 0
		return x
	if kind == 'signs':
		return sign_pattern_signal(args[0])
	if kind == 'levels':
		return levels_signal(args[0])
	raise ValueError(kind)


PARAMS = ('kernel_size_smooth_silence', 'kernel_size_smooth_signal', 'kernel_size_smooth_speaker', 'silence_absolute_threshold', 'silence_relative_threshold', 'eps',
          'normalization_percentile')
REF_PARAMS = dict(kernel_size_smooth_silence = 4096, kernel_size_smooth_signal = 128, kernel_size_smooth_speaker = 4096, silence_absolute_threshold = 0.05,
                  silence_relative_threshold = 0.2, eps = 1e-9, normalization_percentile = 0.9)


def load_golden(path):
	"""diarization.npz -> dict(select = [(name, spec, params, digest, speaker_id, mask)], speaker_error = [...], rle = [(x, starts, lengths, values)])."""
	import json
	z = np.load(path, allow_pickle = False)
	meta = json.loads(str(z['meta']))
	select = []
	for i, c in enumerate(meta['select']):
		speaker_id = unrle(z[f's{i}_id_lengths'], z[f's{i}_id_values']).astype(np.float32)
		mask = np.stack([unrle(z[f's{i}_m{r}_lengths'], z[f's{i}_m{r}_values']).astype(bool) for r in range(3)])
		select.append((c['name'], c['spec'], c['params'], c['digest'], speaker_id, mask))
	rle_cases = [(z[f'r{i}_x'], z[f'r{i}_starts'], z[f'r{i}_lengths'], z[f'r{i}_values']) for i in range(meta['n_rle'])]
	return dict(select = select, speaker_error = meta['speaker_error'], rle = rle_cases)
