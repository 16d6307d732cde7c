"""audio_read.npz and the four small audio files next to it: the reference's own audio.read_audio (audio.py:17-128) with sample_rate = None
(decode, offset / duration slice, int16 -> float, mono mean; no resampling: that is librosa's, and this project's resampler is its own).

The files are generated here from a seed: audio_stereo.wav (2 channels, int16, 8 kHz, 331 samples, the extreme values included),
audio_mono.wav (1 channel, int16, 44.1 kHz, 257 samples), audio_float.wav (2 channels, float32, 16 kHz, 200 samples) and audio_pcm.raw (the
stereo samples as headerless little-endian int16).  What the reference imports but is not installed (librosa, soundfile) is stubbed with empty
modules; its scipy and raw paths do not reach them.

    python tests/golden/make_golden_audio.py <path of the reference checkout>          (writes next to this file)
"""
import contextlib
import importlib
import importlib.machinery
import io
import json
import os
import sys
import types

import numpy as np
import scipy.io.wavfile

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [
	('stereo', 'audio_stereo.wav', dict(mono = False)),
	('stereo_mono', 'audio_stereo.wav', dict(mono = True)),
	('stereo_int16', 'audio_stereo.wav', dict(mono = False, dtype = 'int16')),
	('mono', 'audio_mono.wav', dict(mono = True)),
	('mono_int16', 'audio_mono.wav', dict(mono = False, dtype = 'int16')),
	('float', 'audio_float.wav', dict(mono = False)),
	('float_mono', 'audio_float.wav', dict(mono = True)),
	('raw', 'audio_pcm.raw', dict(mono = False, raw_sample_rate = 8000, raw_num_channels = 2)),
	('raw_mono', 'audio_pcm.raw', dict(mono = True, raw_sample_rate = 8000, raw_num_channels = 2)),
	('slice', 'audio_stereo.wav', dict(mono = False, offset = 0.0123, duration = 0.0171)),      # int(98.4) : int(235.2)
	('slice_mono', 'audio_stereo.wav', dict(mono = True, offset = 0.00631, duration = 0.02003)),  # int(50.48) : int(210.72)
	('offset_only', 'audio_stereo.wav', dict(mono = False, offset = 0.03119)),                  # int(249.52) :
	('duration_only', 'audio_mono.wav', dict(mono = True, duration = 0.00211)),                 # : int(93.051)
	('slice_raw', 'audio_pcm.raw', dict(mono = False, offset = 0.0123, duration = 0.0171, raw_sample_rate = 8000, raw_num_channels = 2)),
	('unreadable', 'no_such_file.wav', dict(mono = True)),
]


def stub(name):
	mod = types.ModuleType(name)
	mod.__spec__ = importlib.machinery.ModuleSpec(name, None)
	mod.__path__ = []
	sys.modules[name] = mod


def write_files():
	rng = np.random.default_rng(14)
	stereo = rng.integers(-32768, 32768, (331, 2)).astype(np.int16)
	stereo[:4] = [[32767, -32768], [-32768, 32767], [32767, 32767], [-32768, -32768]]
	stereo[4:6] = [[0, 1], [-1, 0]]
	scipy.io.wavfile.write(os.path.join(HERE, 'audio_stereo.wav'), 8000, stereo)
	scipy.io.wavfile.write(os.path.join(HERE, 'audio_mono.wav'), 44100, rng.integers(-32768, 32768, 257).astype(np.int16))
	scipy.io.wavfile.write(os.path.join(HERE, 'audio_float.wav'), 16000, rng.uniform(-1, 1, (200, 2)).astype(np.float32))
	with open(os.path.join(HERE, 'audio_pcm.raw'), 'wb') as f:
		f.write(stereo.astype('<i2').tobytes())


def main():
	if len(sys.argv) < 2 and 'CONVASR_REFERENCE' not in os.environ:
		sys.exit('usage: make_golden_audio.py <path of the reference checkout>   (or CONVASR_REFERENCE)')
	for name in ('librosa', 'soundfile'):
		try:
			importlib.import_module(name)
		except Exception:
			stub(name)
	sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else os.environ['CONVASR_REFERENCE'])
	import audio
	write_files()
	arrays, meta = {}, []
	for name, file, kwargs in CASES:
		with contextlib.redirect_stdout(io.StringIO()):
			signal, rate = audio.read_audio(os.path.join(HERE, file), sample_rate = None, **kwargs)
		arrays[name] = signal.numpy()
		meta.append(dict(name = name, file = file, kwargs = kwargs, sample_rate = rate, dtype = str(arrays[name].dtype), shape = list(arrays[name].shape)))
		print(name, arrays[name].shape, arrays[name].dtype, rate)
	path = os.path.join(HERE, 'audio_read.npz')
	np.savez_compressed(path, meta = np.array(json.dumps(meta)), **arrays)
	print('audio_read.npz', len(meta), 'cases,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
	main()
