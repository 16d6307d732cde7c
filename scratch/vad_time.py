"""Timing of the speech-activity path on the GPU (README row, DESIGN.md 7g, profiles/r14_vad.json).

    python scratch/vad_time.py --leg kernels --out DIR   ops.frame_peaks, vad.segments and ops.gather_segments on 5 and 60 minutes at 8 and 16 kHz, mono
                                                         and stereo, int16 and float32
    python scratch/vad_time.py --leg numpy --out DIR     the numpy restatement (tests/_vad_ref.py) on one CPU core, 5 minutes at 8 kHz, mono
    python scratch/vad_time.py --leg long --out DIR      transcribe.transcribe_long against transcribe.transcribe_file on one synthetic hour at 16 kHz,
                                                         Wav2Letter, fused eval, bf16, random weights: end to end and the model's share
    python scratch/vad_time.py --leg merge --out DIR     DIR/vad_*.json -> DIR/r14_vad.json
Each leg is one process, to be run under its own `timeout`.  Kernel times are medians of 7 runs after 2 warm-up runs, device events around the
call on one device; end-to-end times are host clocks around work that ends in a synchronise.  Bytes are what a pass must read and write,
computed from the shapes; the share is against 8 TB/s."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _vad_ref as R  # noqa: E402

HBM_PEAK = 8.0e12


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


def host_ms(fn, warmup = 2, runs = 7):
	for _ in range(warmup):
		fn()
	times = []
	for _ in range(runs):
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		fn()
		torch.cuda.synchronize()
		times.append(1e3 * (time.perf_counter() - t0))
	return dict(median_ms = statistics.median(times), min_ms = min(times), max_ms = max(times), runs = runs)


def with_bytes(t, nbytes):
	return dict(t, bytes = int(nbytes), share_of_hbm_peak = nbytes / (t['median_ms'] * 1e-3) / HBM_PEAK)


def talk(channels, seconds, rate, seed = 7):
	"""Bursts of noise of 2 to 12 s and of varying loudness between gaps of 1.5 to 6 s of faint noise: one minute per channel, tiled to the
	length (generating an hour sample by sample is host time only).  float32 in [-1, 1]."""
	rng = np.random.default_rng(seed)
	minute = np.zeros((channels, 60 * rate), np.float32)
	for c in range(channels):
		at = int(rng.uniform(0, 2) * rate)
		while at < minute.shape[1]:
			n = int(rng.uniform(2, 12) * rate)
			piece = minute[c, at:at + n]
			piece[:] = rng.uniform(-1, 1, len(piece)) * rng.uniform(0.1, 0.9)
			at += n + int(rng.uniform(1.5, 6) * rate)
	minute += (rng.uniform(-1, 1, minute.shape) * 0.002).astype(np.float32)
	return np.tile(minute, (1, (seconds + 59) // 60))[:, :seconds * rate]


def as_dtype(x, dtype):
	return x if dtype == 'float32' else np.round(x * 32767).astype(np.int16)


def leg_kernels(out):
	from convasr_amd import ops, vad
	res = dict(device = torch.cuda.get_device_name(0), window_size = 0.02, aggressiveness = 2, max_duration = 15.0, cases = [])
	for minutes in (5, 60):
		for rate in (8000, 16000):
			for channels in (1, 2):
				for dtype in ('int16', 'float32'):
					x = torch.from_numpy(as_dtype(talk(channels, 60 * minutes, rate), dtype)).cuda()
					F, N = int(0.02 * rate), x.shape[1]
					case = dict(minutes = minutes, sample_rate = rate, channels = channels, dtype = dtype, N = N, frame_len = F, frames = -(-N // F))
					case['frame_peaks'] = with_bytes(gpu_ms(lambda: ops.frame_peaks(x, F)), x.numel() * x.element_size() + 4 * channels * case['frames'])
					peaks = ops.frame_peaks(x, F)
					k = max(1, int(0.9 * (N // F)))
					case['vad_frames'] = gpu_ms(lambda: ops.vad_frames(peaks, N // F, 0.02, 0.1, 1e-9, k, 50, 25, 10))
					mask = ops.vad_frames(peaks, N // F, 0.02, 0.1, 1e-9, k, 50, 25, 10)[1]
					case['vad_segments_op'] = host_ms(lambda: ops.vad_segments(mask, peaks, F, N, 750))
					case['segments_end_to_end'] = host_ms(lambda: vad.segments(x, rate))
					segs = vad.segments(x, rate)
					case['segments'] = len(segs)
					case['share_of_samples_kept'] = sum(s['count'] for s in segs) / (channels * N)
					chunk = sorted(segs, key = lambda s: -s['count'])[:64]
					cols = [[s[key] for s in chunk] for key in ('channel', 'first', 'count')]
					gx, _ = ops.gather_segments(x, *cols)
					case['gather_segments_64_longest'] = with_bytes(gpu_ms(lambda: ops.gather_segments(x, *cols)), sum(cols[2]) * x.element_size() + 4 * gx.numel())
					case['gather_shape'] = list(gx.shape)
					print(json.dumps(case), flush = True)
					res['cases'].append(case)
					del x, peaks, mask, gx
	json.dump(res, open(os.path.join(out, 'vad_kernels.json'), 'w'), indent = 1)


def leg_numpy(out):
	x = talk(1, 300, 8000)
	cfg = R.settings(8000, 0.02, 2)
	times = []
	for _ in range(3):
		t0 = time.perf_counter()
		peaks, _, mask = R.detect_frames(x, cfg)
		R.segments(mask, peaks, cfg['F'], x.shape[1], 750)
		times.append(time.perf_counter() - t0)
	res = dict(minutes = 5, sample_rate = 8000, channels = 1, what = 'tests/_vad_ref.py detect_frames + segments, one process (numpy, one core)', median_s = statistics.median(times), runs = times)
	print(json.dumps(res), flush = True)
	json.dump(res, open(os.path.join(out, 'vad_numpy.json'), 'w'), indent = 1)


def leg_long(out, minutes):
	import convasr_amd as ca
	from convasr_amd import transcribe
	from convasr_amd.transcript_generators import CharTokenizerLegacy, GreedyCTCGenerator
	rate, device = 16000, torch.device('cuda', 0)
	torch.manual_seed(1)
	torch.set_grad_enabled(False)
	pipeline = transcribe.TextPipeline(CharTokenizerLegacy(transcribe.RU_ALPHABET))
	frontend = ca.models.LogFilterBankFrontend(64, rate, 0.02, 0.01, 'hann_window')
	model = ca.models.Wav2Letter(64, [pipeline.tokenizer.vocab_size], frontend = frontend, check_time_dim_padded = False, compute_dtype = torch.bfloat16,
	                             dict = lambda logits, log_probs, olen, **kwargs: (log_probs[0], logits[0], olen[0]))
	model.to(device)
	model.train()
	model(torch.rand(2, rate * 2, device = device) * 2 - 1, torch.ones(2, device = device))  # (running statistics that are not the initial ones)
	model.eval()
	model.fuse_conv_bn_eval()
	spans = []

	def timed_model(x, xlen):
		a, b = torch.cuda.Event(enable_timing = True), torch.cuda.Event(enable_timing = True)
		a.record()
		y = model(x, xlen)
		b.record()
		spans.append((a, b, tuple(x.shape)))
		return y

	args = types.SimpleNamespace(device = 'cuda:0', sample_rate = rate, mono = True, batch_size = 64)
	pcm = as_dtype(talk(1, 60 * minutes, rate), 'int16')
	res = dict(device = torch.cuda.get_device_name(0), model = 'Wav2Letter, fused eval, bf16, random weights', minutes = minutes, sample_rate = rate, samples = int(pcm.shape[1]), batch_size = 64)
	with tempfile.TemporaryDirectory() as tmp:
		path = os.path.join(tmp, 'hour.wav')
		with wave.open(path, 'wb') as w:
			w.setnchannels(1)
			w.setsampwidth(2)
			w.setframerate(rate)
			w.writeframes(pcm.tobytes())
		for name, route in (('transcribe_long', transcribe.transcribe_long), ('transcribe_file', transcribe.transcribe_file)):
			def run():
				del spans[:]
				torch.cuda.synchronize()
				t0 = time.perf_counter()
				result = route(args, pipeline, timed_model, GreedyCTCGenerator(), path)
				torch.cuda.synchronize()
				return 1e3 * (time.perf_counter() - t0), sum(a.elapsed_time(b) for a, b, _ in spans), result
			try:
				first = run()
				runs = [run() for _ in range(7 if first[0] < 4000 else 3)] if first[0] < 60000 else [first]
				whole, inside = statistics.median(r[0] for r in runs), statistics.median(r[1] for r in runs)
				res[name] = dict(first_call_ms = first[0], end_to_end_median_ms = whole, model_median_ms = inside, model_share = inside / whole, runs = len(runs), model_calls = len(spans),
				                 largest_batch = list(max((s[2] for s in spans), key = lambda s: s[0] * s[1])), samples_through_the_model = sum(s[2][0] * s[2][1] for s in spans))
				if name == 'transcribe_long':
					res[name].update(segments = len(first[2].segments), share_of_samples_kept = sum(s['count'] for s in first[2].segments) / pcm.shape[1], words = len(first[2].transcript))
				else:
					res[name].update(words = sum(len(h) for h in first[2].hyp_segments))
			except (ca._lib.ConvasrHipError, torch.cuda.OutOfMemoryError, ValueError) as e:  # (an envelope refusal or an allocation failure is a result here: the hour as ONE row is the parent's route; anything else ends the leg)
				res[name] = dict(not_measured = f'{type(e).__name__}: {e}'[:600])
			print(json.dumps({name: res[name]}), flush = True)
			json.dump(res, open(os.path.join(out, 'vad_long.json'), 'w'), indent = 1)


def leg_merge(out):
	res = json.load(open(os.path.join(out, 'vad_kernels.json')))
	for name, key in (('vad_numpy.json', 'numpy_one_core'), ('vad_long.json', 'transcribe_long_against_transcribe_file')):
		res[key] = json.load(open(os.path.join(out, name))) if os.path.exists(os.path.join(out, name)) else 'not measured'
	json.dump(res, open(os.path.join(out, 'r14_vad.json'), 'w'), indent = 1)


if __name__ == '__main__':
	ap = argparse.ArgumentParser()
	ap.add_argument('--leg', required = True, choices = ['kernels', 'numpy', 'long', 'merge'])
	ap.add_argument('--minutes', type = int, default = 60)
	ap.add_argument('--out', default = os.path.join(ROOT, 'profiles'))
	args = ap.parse_args()
	os.makedirs(args.out, exist_ok = True)
	if args.leg in ('kernels', 'long'):
		assert torch.cuda.is_available(), 'this leg measures on the GPU'
	dict(kernels = lambda: leg_kernels(args.out), numpy = lambda: leg_numpy(args.out), long = lambda: leg_long(args.out, args.minutes), merge = lambda: leg_merge(args.out))[args.leg]()
