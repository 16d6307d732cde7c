"""Timing of the keyword search on the GPU (README row, profiles/r16_keyword_search.json).  Legs, each a process of its own under a time limit
(--leg all starts them one after the other and stops at the first that fails):
  kernel  convasr_ctc_keyword_search by DEVICE EVENTS around the C call, buffers allocated outside, on seeded speech-like log-probs (runs of 3
          frames, 60 % blanks, 3 % spaces; 38 classes): 64 x 753 frames with K = 64 phrases of 12 labels (with and without the dense outputs), and
          1 x 180,000 frames (an hour) with K = 1 and K = 1,000.  Beside each: ops.argmax on the same log-probs -- the floor of ONE read of them.
          A wave walks its utterance frame by frame, so time / T is what a frame costs a wave; in cycles at the shader clock a sampler thread reads
          from the card's hwmon freq1_input while the K = 1 hour runs back to back (not readable: the figure is left out, not assumed).
  numpy   tests/_kws_ref.py search_dense + pick on one core, at a REDUCED shape: 1 x 7,530 frames x 38 classes, one phrase of 12 labels.
  long    transcribe.search_long end to end on one synthetic hour at 16 kHz (scratch/vad_time.py's talk), Wav2Letter, fused eval, bf16, random
          weights, 8 phrases: WALL CLOCK between two device synchronisations, host work included, and the model's share by device events.
  merge   the legs' files into r16_keyword_search.json.
Medians of 7 after 2 warm-ups, with min and max.  Usage: python scratch/keyword_search_time.py --leg all --out DIR"""
import argparse
import glob
import json
import os
import statistics
import subprocess
import sys
import threading
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from convasr_amd import ops  # noqa: E402
from convasr_amd.transcribe import RU_ALPHABET  # noqa: E402
from convasr_amd.transcript_generators import CharTokenizerLegacy  # noqa: E402
from greedy_segments_time import speech_like, stats  # noqa: E402

WARMUP, RUNS = 2, 7
LIMITS = dict(kernel = 420, numpy = 300, long = 540)  # seconds per leg


def events(fns, warmup = WARMUP, runs = RUNS):
	"""Device-event times (ms) of every callable in fns, alternating; the callables only enqueue."""
	times = {k: [] for k in fns}
	for rep in range(warmup + runs):
		marks = {}
		for k, fn in fns.items():
			a, b = torch.cuda.Event(enable_timing = True), torch.cuda.Event(enable_timing = True)
			a.record()
			fn()
			b.record()
			marks[k] = (a, b)
		torch.cuda.synchronize()
		if rep >= warmup:
			for k, (a, b) in marks.items():
				times[k].append(a.elapsed_time(b))
	return times


def shader_clock_file():
	props = torch.cuda.get_device_properties(0)
	bus = '%04x:%02x:%02x' % (getattr(props, 'pci_domain_id', 0), props.pci_bus_id, props.pci_device_id)
	for card in glob.glob('/sys/class/drm/card*'):
		if os.path.realpath(card + '/device').split('/')[-1].startswith(bus):
			for path in glob.glob(card + '/device/hwmon/hwmon*/freq1_input'):
				return path
	return None


def clock_while(fn, seconds = 1.0):
	"""Median of the shader clock (MHz) sampled every ~2 ms while fn is enqueued back to back for about `seconds`; None when it cannot be read."""
	path = shader_clock_file()
	if path is None:
		return None
	samples, stop = [], []

	def sampler():
		while not stop:
			try:
				samples.append(int(open(path).read()) / 1e6)
			except (OSError, ValueError):
				return
			time.sleep(0.002)
	th = threading.Thread(target = sampler)
	th.start()
	t0 = time.perf_counter()
	while time.perf_counter() - t0 < seconds:
		fn()
		torch.cuda.synchronize()
	stop.append(1)
	th.join()
	return dict(median_mhz = statistics.median(samples), min_mhz = min(samples), max_mhz = max(samples), samples = len(samples), source = 'hwmon freq1_input') if samples else None


def log_probs_like(B, T, tok, d):
	C = tok.vocab_size
	path = speech_like(B, T, tok, B + T)
	g = torch.Generator().manual_seed(B + T)
	logits = torch.randn(B, T, C, generator = g) * 2
	logits.scatter_add_(2, path.unsqueeze(-1), torch.full((B, T, 1), 5.0))
	return torch.log_softmax(logits, -1).to(d), path  # (B, T, C) contiguous = the channels-last memory of a (B, C, T) tensor


def phrases_from(path, tok, K, L, seed):
	"""K phrases of L labels: every fourth one cut out of the collapsed path of utterance 0 (it IS said), the others random letters."""
	rng = np.random.RandomState(seed)
	said = [c for c, prev in zip(path[0].tolist(), [-1] + path[0].tolist()) if c != prev and c != tok.eps_id]
	said = [c for c, prev in zip(said, [-1] + said) if c != prev]
	rows = []
	for k in range(K):
		at = rng.randint(0, max(1, len(said) - L))
		rows.append(said[at:at + L] if k % 4 == 0 and len(said) >= L else rng.randint(0, len(tok.alphabet), size = L).tolist())
	return torch.tensor(rows, dtype = torch.int32)


def measure(B, T, K, L, tok, d, dense_too, clock):
	C = tok.vocab_size
	lp, path = log_probs_like(B, T, tok, d)
	tokens = phrases_from(path, tok, K, L, K + T).to(d)
	tl = torch.full((K, ), L, dtype = torch.int32, device = d)
	thr = torch.full((K, ), -1.0 * L, dtype = torch.float32, device = d)
	olen = torch.full((B, ), T, dtype = torch.int64, device = d)
	H = 16
	count = torch.empty(B, K, dtype = torch.int32, device = d)
	score = torch.empty(B, K, H, dtype = torch.float32, device = d)
	begin, end = torch.empty(B, K, H, dtype = torch.int32, device = d), torch.empty(B, K, H, dtype = torch.int32, device = d)
	idx = torch.empty(B, T, dtype = torch.int64, device = d)
	P, S = ops.ptr, ops.stream_ptr
	fns = dict(keyword_search = lambda: ops.call('convasr_ctc_keyword_search', P(lp), P(olen), P(tokens), P(tl), P(thr), P(count), P(score), P(begin), P(end), None, None, B, T, C, K, L, H, tok.eps_id, 10, S()),
	           argmax = lambda: ops.call('convasr_argmax', P(lp), P(idx), B * T, C, S()))
	if dense_too:
		ds, db = torch.empty(B, K, T, dtype = torch.float32, device = d), torch.empty(B, K, T, dtype = torch.int32, device = d)
		fns['keyword_search_dense'] = lambda: ops.call('convasr_ctc_keyword_search', P(lp), P(olen), P(tokens), P(tl), P(thr), P(count), P(score), P(begin), P(end), P(ds), P(db), B, T, C, K, L, H, tok.eps_id, 10, S())
	times = events(fns)
	med = statistics.median(times['keyword_search'])
	out = dict(B = B, T = T, classes = C, phrases = K, labels = L, waves = B * K, workgroups = B * -(-K // ops.ctc_keyword_search_limits()[1]), tile_frames = ops.ctc_keyword_search_tile_frames(C),
	           device_events = {k: stats(v) for k, v in times.items()}, hits = int(count.sum()), most_hits_per_row = int(count.max()),
	           log_prob_bytes = 4 * B * T * C, keyword_search_over_argmax = med / statistics.median(times['argmax']),
	           microseconds_per_frame_per_wave = 1e3 * med / T, frames_per_second_per_wave = T / (med * 1e-3), frames_per_second_all_waves = B * K * T / (med * 1e-3))
	if clock:
		out['shader_clock_while_running'] = clock_while(fns['keyword_search'])
		if out['shader_clock_while_running']:
			out['cycles_per_frame_per_wave_at_that_clock'] = out['microseconds_per_frame_per_wave'] * out['shader_clock_while_running']['median_mhz']
	return out


def leg_kernel(out):
	d = torch.device('cuda:0')
	tok = CharTokenizerLegacy(RU_ALPHABET)
	res = dict(device = torch.cuda.get_device_name(0),
	           note = "the runtime names the MI355X 'AMD Radeon Graphics'; device_events: torch.cuda.Event pairs around the C entry points, alternating, medians of 7 after 2 warm-ups; a wave owns one (utterance, phrase) and walks its T frames one after the other, so time / T is a frame's cost to a wave",
	           shapes = [])
	for B, T, K, dense_too, clock in ((64, 753, 64, True, False), (1, 180000, 1, False, True), (1, 180000, 1000, False, False)):
		res['shapes'].append(measure(B, T, K, 12, tok, d, dense_too, clock))
		print(json.dumps(res['shapes'][-1]), flush = True)
		json.dump(res, open(os.path.join(out, 'kws_kernel.json'), 'w'), indent = 1)


def leg_numpy(out):
	import _kws_ref as R
	tok = CharTokenizerLegacy(RU_ALPHABET)
	T = 7530
	lp, path = log_probs_like(1, T, tok, 'cpu')
	phrase = phrases_from(path, tok, 1, 12, 1)[0].tolist()
	lp = lp[0].numpy()
	times = []
	for _ in range(3):
		t0 = time.perf_counter()
		score, begin = R.search_dense(lp, T, phrase, tok.eps_id)
		hits = R.pick(score, begin, T, -12.0, 10)
		times.append(time.perf_counter() - t0)
	res = dict(what = 'tests/_kws_ref.py search_dense + pick, one process (numpy, one core)', B = 1, T = T, classes = tok.vocab_size, phrases = 1, labels = 12, hits = len(hits),
	           median_s = statistics.median(times), runs = times, microseconds_per_frame = 1e6 * statistics.median(times) / T)
	print(json.dumps(res), flush = True)
	json.dump(res, open(os.path.join(out, 'kws_numpy.json'), 'w'), indent = 1)


def leg_long(out, minutes):
	import convasr_amd as ca
	from convasr_amd import transcribe
	from vad_time import as_dtype, talk
	rate, device = 16000, torch.device('cuda', 0)
	torch.manual_seed(1)
	torch.set_grad_enabled(False)
	pipeline = transcribe.TextPipeline(CharTokenizerLegacy(RU_ALPHABET))
	frontend = ca.models.LogFilterBankFrontend(64, rate, 0.02, 0.01, 'hann_window')
	model = ca.models.Wav2Letter(64, [pipeline.tokenizer.vocab_size], frontend = frontend, check_time_dim_padded = False, compute_dtype = torch.bfloat16,
	                             dict = lambda logits, log_probs, olen, **kwargs: (log_probs[0], logits[0], olen[0]))
	model.to(device)
	model.train()
	model(torch.rand(2, rate * 2, device = device) * 2 - 1, torch.ones(2, device = device))  # (running statistics that are not the initial ones)
	model.eval()
	model.fuse_conv_bn_eval()
	spans, searches = [], []

	def timed_model(x, xlen):
		a, b = torch.cuda.Event(enable_timing = True), torch.cuda.Event(enable_timing = True)
		a.record()
		y = model(x, xlen)
		b.record()
		spans.append((a, b, tuple(x.shape)))
		return y
	real_search = ops.ctc_keyword_search

	def timed_search(*a, **k):
		e = torch.cuda.Event(enable_timing = True), torch.cuda.Event(enable_timing = True)
		e[0].record()
		r = real_search(*a, **k)
		e[1].record()
		searches.append(e)
		return r
	ops.ctc_keyword_search = timed_search
	args = types.SimpleNamespace(device = 'cuda:0', sample_rate = rate, mono = True, batch_size = 64)
	signal = torch.from_numpy(as_dtype(talk(1, 60 * minutes, rate), 'int16')).to(device)
	phrases = ['добрый день', 'спасибо', 'договор', 'перезвоните', 'до свидания', 'оператор', 'номер телефона', 'да']

	def run():
		del spans[:], searches[:]
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		result = transcribe.search_long(args, pipeline, timed_model, signal, phrases)
		torch.cuda.synchronize()
		return 1e3 * (time.perf_counter() - t0), sum(a.elapsed_time(b) for a, b, _ in spans), sum(a.elapsed_time(b) for a, b in searches), result
	runs = [run() for _ in range(WARMUP + RUNS)]
	first, runs = runs[0], runs[WARMUP:]
	res = dict(device = torch.cuda.get_device_name(0), model = 'Wav2Letter, fused eval, bf16, random weights', minutes = minutes, sample_rate = rate, samples = int(signal.shape[1]), batch_size = 64,
	           phrases = len(phrases), what = 'transcribe.search_long on a (1, N) int16 device tensor; wall clock between two device synchronisations, host work included',
	           first_call_ms = first[0], end_to_end = stats([r[0] for r in runs]), model_device_events = stats([r[1] for r in runs]),
	           search_calls_device_events_with_their_host_part = stats([r[2] for r in runs]), model_calls = len(spans), segments = len(first[3].segments), hits = len(first[3].hits),
	           share_of_samples_kept = sum(s['count'] for s in first[3].segments) / signal.shape[1])
	print(json.dumps(res), flush = True)
	json.dump(res, open(os.path.join(out, 'kws_long.json'), 'w'), indent = 1)


def leg_merge(out):
	res = json.load(open(os.path.join(out, 'kws_kernel.json')))
	for name, key in (('kws_numpy.json', 'numpy_one_core_reduced_shape'), ('kws_long.json', 'search_long_one_hour')):
		res[key] = json.load(open(os.path.join(out, name))) if os.path.exists(os.path.join(out, name)) else 'not measured'
	res['which_clock'] = dict(shapes = 'DEVICE EVENTS around the C entry points, one MI355X, medians of 7 after 2 warm-ups with min and max', numpy_one_core_reduced_shape = 'host wall clock, one core of the same machine, 3 runs',
	                          search_long_one_hour = 'WALL CLOCK between two device synchronisations, host work included, medians of 7 after 2 warm-ups with min and max; the model and the search calls inside it by device events')
	json.dump(res, open(os.path.join(out, 'r16_keyword_search.json'), 'w'), indent = 1)


if __name__ == '__main__':
	ap = argparse.ArgumentParser()
	ap.add_argument('--leg', required = True, choices = ['kernel', 'numpy', 'long', 'merge', 'all'])
	ap.add_argument('--minutes', type = int, default = 60)
	ap.add_argument('--out', default = os.path.join(ROOT, 'profiles'))
	a = ap.parse_args()
	os.makedirs(a.out, exist_ok = True)
	if a.leg == 'all':
		for leg in ('kernel', 'numpy', 'long'):
			r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', leg, '--minutes', str(a.minutes), '--out', a.out], timeout = LIMITS[leg])
			if r.returncode != 0:
				sys.exit(f'leg {leg} ended with status {r.returncode}: nothing more is started')
		leg_merge(a.out)
	elif a.leg == 'merge':
		leg_merge(a.out)
	elif a.leg == 'numpy':
		leg_numpy(a.out)
	else:
		assert torch.cuda.is_available(), 'this leg measures on the GPU'
		leg_kernel(a.out) if a.leg == 'kernel' else leg_long(a.out, a.minutes)
