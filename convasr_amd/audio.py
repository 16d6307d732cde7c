"""MI355X-native mirror of the reference's audio.py: read_audio, resample, write_audio, compute_duration, is_audio, s2f / f2s.

* decode_audio(...) -> (signal (T, C) int16 / float32 numpy array as the file holds it, its sample rate): the host half of read_audio
  (audio.py:34-111): wav through scipy.io.wavfile, .raw / raw_bytes, then the offset / duration slice.  No device is touched.
* read_audio(...): decode_audio, ONE copy of the raw interleaved samples to the GPU (int16: no float intermediate on the host), then int16 ->
  float, de-interleave, mono mix and the change of sample rate in one launch (ops.resample, csrc/resample.hip).
* resample(signal, sample_rate_, sample_rate): the band-limited rational resampler of include/convasr_hip.h.  The reference calls
  librosa.resample here; this resampler is defined by this project and unpinned against librosa: the same output length and timing, its own
  filter (the 'kaiser_best' parameters of resampy evaluated at the exact rational phases).

Out of scope: decoding through soundfile, ffmpeg or sox (NotImplementedError naming the backend), extract_meta."""
import os

import numpy as np
import torch

from . import ops

AUDIO_FILE_EXTENSIONS = {'.mp3', '.m4a', '.amr', '.gsm', '.wav', '.mp4', '.opus', '.ogg', '.webm', '.3gp'}

smax = torch.iinfo(torch.int16).max
f2s_numpy = f2s = lambda signal, max = np.float32(smax): np.multiply(signal, max).astype('int16')
s2f_numpy = s2f = lambda signal, max = np.float32(smax): np.divide(signal, max, dtype = 'float32')


def _check_backend(audio_path, backend):
	assert backend in [None, 'scipy', 'soundfile', 'ffmpeg', 'sox']
	if audio_path is None or audio_path.endswith('.raw'):
		return
	if backend in ('soundfile', 'ffmpeg', 'sox'):
		raise NotImplementedError(f'audio backend {backend!r} is not implemented: wav files through scipy and raw PCM only')
	if not audio_path.endswith('.wav'):
		raise NotImplementedError(f"audio backend 'ffmpeg' (what the reference decodes {os.path.splitext(audio_path)[-1] or audio_path!r} files with) is not implemented: wav files through scipy and raw PCM only")


def decode_audio(audio_path, sample_rate = None, offset = 0, duration = None, raw_dtype = 'int16', dtype = 'float32', byte_order = 'little', backend = None, raw_bytes = None,
                 raw_sample_rate = None, raw_num_channels = None):
	"""The host half of read_audio: (signal (T, C) int16 or float32 as stored, interleaved; the file's own sample rate), sliced by offset /
	duration at that rate with the reference's int(...) rule.  An unreadable or malformed file gives the reference's empty result: a (0, 1)
	array of `dtype` at `sample_rate` (audio.py:102-104)."""
	import scipy.io.wavfile
	assert dtype in [None, 'int16', 'float32']
	_check_backend(audio_path, backend)
	try:
		if audio_path is None or audio_path.endswith('.raw'):
			if audio_path is not None:
				with open(audio_path, 'rb') as f:
					raw_bytes = f.read()
			sample_rate_, signal = raw_sample_rate, np.frombuffer(raw_bytes, dtype = raw_dtype).reshape(-1, raw_num_channels)
		else:
			sample_rate_, signal = scipy.io.wavfile.read(audio_path)
			signal = signal[:, None] if len(signal.shape) == 1 else signal
	except Exception:
		print(f'Error when reading [{audio_path}]')
		sample_rate_, signal = sample_rate, np.empty(shape = (0, 1), dtype = dtype)
	if offset or duration is not None:
		signal = signal[slice(int(offset * sample_rate_) if offset else None, int((offset + duration) * sample_rate_) if duration is not None else None)]
	assert signal.dtype in [np.int16, np.float32], f'{audio_path}: samples of {signal.dtype}, int16 and float32 PCM only'
	return signal, sample_rate_


def read_audio(audio_path, sample_rate, offset = 0, duration = None, mono = True, raw_dtype = 'int16', dtype = 'float32', byte_order = 'little', backend = None, raw_bytes = None,
               raw_sample_rate = None, raw_num_channels = None, device = None):
	"""audio.read_audio (audio.py:17-128) with everything after the decode on the GPU.  Returns (signal (C, T) on `device` (default: the
	current GPU), sample rate): float32 scaled by 1 / 32767 from int16 PCM, the mean over channels with mono, at `sample_rate` unless that is
	None.  dtype 'int16' (or None on an int16 file) returns the samples as stored, and raises with a rate change or a mono mix of several
	channels, as the reference's asserts do."""
	signal, sample_rate_ = decode_audio(audio_path, sample_rate, offset = offset, duration = duration, raw_dtype = raw_dtype, dtype = dtype, byte_order = byte_order, backend = backend,
	                                    raw_bytes = raw_bytes, raw_sample_rate = raw_sample_rate, raw_num_channels = raw_num_channels)
	device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
	num_channels = signal.shape[1]
	change = sample_rate is not None and sample_rate_ != sample_rate
	x = torch.from_numpy(np.ascontiguousarray(signal)).to(device)  # the one copy: the samples as the file holds them
	if signal.dtype == np.int16 and dtype != 'float32':
		if (mono and num_channels > 1) or change:
			raise AssertionError('read_audio: a mono mix or a change of sample rate needs dtype = \'float32\' (audio.py:120, 151)')
		return x.t().contiguous(), sample_rate_
	if x.dtype == torch.float32:
		x = x.t().contiguous()  # planar (C, T)
	return ops.resample(x, sample_rate_, sample_rate if change else sample_rate_, mono = bool(mono and num_channels > 1)), (sample_rate if change else sample_rate_)


def resample(signal, sample_rate_, sample_rate):
	"""audio.resample (audio.py:150-159): (C, T) float32 -> ((C, ceil(T * sample_rate / sample_rate_)) float32, sample_rate).  A GPU tensor
	stays on its GPU; a CPU tensor is moved to the current device and the result is LEFT THERE (there is no CPU path).  The filter is this
	project's (include/convasr_hip.h), unpinned against librosa."""
	assert signal.dtype == torch.float32
	if not signal.is_cuda:
		signal = signal.to(torch.device('cuda', torch.cuda.current_device()))
	return ops.resample(signal, sample_rate_, sample_rate), sample_rate


def write_audio(audio_path, signal, sample_rate, mono = False, backend = None, format = 'wav'):
	"""audio.write_audio (audio.py:131-147), scipy backend: (C, T) float32 on any device -> 16-bit PCM wav."""
	import scipy.io.wavfile
	assert backend in [None, 'scipy', 'soundfile']
	if backend == 'soundfile' or not (backend == 'scipy' or not audio_path or audio_path.endswith('.wav')):
		raise NotImplementedError("audio backend 'soundfile' is not implemented: wav files through scipy only")
	assert signal.dtype == torch.float32
	signal = signal if (not mono or len(signal) == 1) else signal.mean(dim = 0, keepdim = True)
	scipy.io.wavfile.write(audio_path, sample_rate, f2s_numpy(signal.t().cpu().numpy()))
	return audio_path


def is_audio(audio_path):
	return os.path.splitext(audio_path)[-1].lower() in AUDIO_FILE_EXTENSIONS


def compute_duration(audio_path, backend = None, raw_dtype = 'int16', raw_sample_rate = None, raw_num_channels = None):
	"""Seconds of audio in a wav file (audio.py:165-176) or, given its format, in a .raw file (from the file's size)."""
	assert backend in [None, 'scipy', 'ffmpeg', 'sox']
	if audio_path.endswith('.raw'):
		return os.path.getsize(audio_path) // (np.dtype(raw_dtype).itemsize * raw_num_channels) / raw_sample_rate
	_check_backend(audio_path, backend)
	signal, sample_rate = decode_audio(audio_path, None, dtype = None, backend = 'scipy')
	return signal.shape[0] / sample_rate
