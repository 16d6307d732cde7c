"""Timing of ops.resample / audio.read_audio on the GPU (README row, profiles/r09_resample.json).

    python scratch/resample_time.py --out DIR [--quick]

(a) ops.resample on 5 min and 60 min of stereo int16 audio, 8,000 -> 16,000, 48,000 -> 16,000 and 44,100 -> 16,000: medians of 7 runs after 2
    warm-up runs, device events; bytes = int16 in + fp32 out, taps per output from the table;
(b) audio.read_audio end to end for the 60 min stereo 48 kHz wav (host clock around a call that ends in a synchronise), the wav read, the
    host-to-device copy of the int16 samples and the kernel timed apart;
(c) one core of the same host: scipy.signal.resample_poly on the 5 min signal (both channels) and the float64 restatement
    tests/_resample_ref.py on a short signal (one channel; its length is in the record)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _resample_ref as R  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, the MI355X specification


def gpu_ms(fn, warmup = 2, runs = 7):
	for _ in range(warmup):
		fn()
	torch.cuda.synchronize()
	times = []
	for _ in range(runs):
		a, b = torch.cuda.Event(enable_timing = True), torch.cuda.Event(enable_timing = True)
		a.record()
		fn()
		b.record()
		torch.cuda.synchronize()
		times.append(a.elapsed_time(b))
	return dict(median_ms = statistics.median(times), min_ms = min(times), max_ms = max(times), runs = runs)


def main():
	p = argparse.ArgumentParser()
	p.add_argument('--out', required = True)
	p.add_argument('--quick', action = 'store_true', help = 'seconds instead of minutes of audio (a rehearsal of the script)')
	args = p.parse_args()
	import convasr_amd as ca
	from convasr_amd import ops, audio
	os.makedirs(args.out, exist_ok = True)
	assert torch.cuda.is_available(), 'a measurement needs the GPU'
	d = torch.device('cuda:0')
	torch.set_num_threads(1)
	minute = 1 if args.quick else 60
	record = dict(device = torch.cuda.get_device_name(0), note = "the runtime names the MI355X 'AMD Radeon Graphics'", kernel = [], host = [])
	gen = torch.Generator(device = d).manual_seed(1)
	for sr_in, sr_out in ((8000, 16000), (48000, 16000), (44100, 16000)):
		taps = ops.resample_table(sr_in, sr_out).shape[0]
		for minutes in (5, 60):
			T_in = sr_in * minutes * minute
			pcm = torch.randint(-32768, 32768, (T_in, 2), generator = gen, device = d, dtype = torch.int16)
			for mono in (False, True):
				t = gpu_ms(lambda: ops.resample(pcm, sr_in, sr_out, mono = mono))
				T_out = ops.resample_out_len(T_in, sr_in, sr_out)
				rows = 1 if mono else 2
				nbytes = pcm.numel() * 2 + rows * T_out * 4
				sec = t['median_ms'] * 1e-3
				record['kernel'].append(dict(t, sr_in = sr_in, sr_out = sr_out, minutes = minutes * minute / 60, channels = 2, mono = mono, T_in = T_in, T_out = T_out, taps = taps, bytes = nbytes,
				                             bytes_per_s = nbytes / sec, fraction_of_hbm_peak = nbytes / sec / HBM_PEAK, fma_per_s = rows * T_out * taps / sec))
				print(record['kernel'][-1], flush = True)
			del pcm
	# (b) read_audio end to end, one hour of stereo 48 kHz
	T_in = 48000 * 60 * minute
	rng = np.random.default_rng(2)
	with tempfile.TemporaryDirectory() as tmp:
		import scipy.io.wavfile
		path = os.path.join(tmp, 'hour.wav')
		scipy.io.wavfile.write(path, 48000, rng.integers(-32768, 32768, (T_in, 2), dtype = np.int16))
		whole, read, copy, kernel = [], [], [], []
		for i in range(5):
			torch.cuda.synchronize()
			t0 = time.perf_counter()
			signal, _ = audio.read_audio(path, 16000, mono = True)
			torch.cuda.synchronize()
			whole.append(time.perf_counter() - t0)
			del signal
			t0 = time.perf_counter()
			samples, _ = audio.decode_audio(path, 16000)
			read.append(time.perf_counter() - t0)
			t0 = time.perf_counter()
			x = torch.from_numpy(samples).to(d)
			torch.cuda.synchronize()
			copy.append(time.perf_counter() - t0)
			t0 = time.perf_counter()
			ops.resample(x, 48000, 16000, mono = True)
			torch.cuda.synchronize()
			kernel.append(time.perf_counter() - t0)
			del x, samples
		med = lambda v: statistics.median(v[1:]) * 1e3  # (the first pass warms the file cache and the allocator)
		record['read_audio'] = dict(file = '60 min stereo int16 at 48 kHz -> mono 16 kHz' if not args.quick else 'quick', bytes = T_in * 4, whole_ms = med(whole), wav_read_ms = med(read), h2d_copy_ms = med(copy),
		                            kernel_ms = med(kernel), h2d_share = med(copy) / med(whole), runs = 4)
		print(record['read_audio'], flush = True)
	# (c) one core of this host
	import scipy.signal
	for sr_in, sr_out in ((8000, 16000), (48000, 16000), (44100, 16000)):
		L, M = R.ratio(sr_in, sr_out)
		x = rng.uniform(-1, 1, (2, sr_in * 5 * minute)).astype(np.float32)
		t0 = time.perf_counter()
		scipy.signal.resample_poly(x, L, M, axis = 1)
		poly = time.perf_counter() - t0
		seconds = 10 if sr_in == 8000 else 2
		t0 = time.perf_counter()
		R.resample(x[:1, :sr_in * seconds], sr_in, sr_out)
		rest = time.perf_counter() - t0
		record['host'].append(dict(sr_in = sr_in, sr_out = sr_out, resample_poly_5min_stereo_s = poly, restatement_s = rest, restatement_signal_s = seconds, restatement_channels = 1, threads = 1))
		print(record['host'][-1], flush = True)
	with open(os.path.join(args.out, 'r09_resample.json'), 'w') as f:
		json.dump(record, f, indent = 1)


if __name__ == '__main__':
	main()
