"""Timing of the diarization path on the GPU (README row, profiles/r07_diarization.json).

    python scratch/diar_time.py --leg ours  --out DIR      select_speaker end to end and op by op, 5 min / 60 min at 8 kHz, 60 min at 16 kHz,
                                                           and the same N at kernel_size_smooth_silence 128 / 4096 / 16384
    python scratch/diar_time.py --leg numpy --out DIR      the numpy restatement (tests/_diar_ref.py) on one CPU core, 5 min at 8 kHz
    python scratch/diar_time.py --leg torch --seconds S --out DIR   the reference's formulation (F.max_pool1d / kthvalue / F.avg_pool1d at stride 1)
                                                           as torch ops on the same GPU, S seconds of 8 kHz audio
    python scratch/diar_time.py --leg merge --out DIR      DIR/*.json -> DIR/r07_diarization.json
Each leg is one process, to be run under its own `timeout`; times are medians over repeated runs after a warm-up, device events around
the calls.  Bytes are what each pass must read and write, computed from the shapes; the bandwidth share is against 8 TB/s."""
import argparse
import glob
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _diar_ref as R  # noqa: E402
import _diar_synth as S  # noqa: E402

HBM_PEAK = 8.0e12
REF = S.REF_PARAMS


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


def with_bytes(t, nbytes):
	return dict(t, bytes = int(nbytes), share_of_hbm_peak = nbytes / (t['median_ms'] * 1e-3) / HBM_PEAK)


def signal(seconds, rate):
	"""A 60 s recording tiled to the length (generating an hour sample by sample is host time only)."""
	base = S.call_signal(77, 60 * rate, rate)
	return torch.from_numpy(np.ascontiguousarray(np.tile(base, (1, (seconds + 59) // 60))[:, :seconds * rate]))


def leg_ours(out):
	from convasr_amd import diarization as D, ops
	res = dict(device = torch.cuda.get_device_name(0), cases = [])
	for seconds, rate in ((300, 8000), (3600, 8000), (3600, 16000)):
		x = signal(seconds, rate).cuda()
		N = x.shape[1]
		case = dict(seconds = seconds, sample_rate = rate, N = N, by_silence_window = {})
		for Ksil in (128, 4096, 16384):
			p = dict(REF, kernel_size_smooth_silence = Ksil)
			case['by_silence_window'][str(Ksil)] = gpu_ms(lambda: D.select_speaker(x, **p))
		case['select_speaker'] = case['by_silence_window']['4096']
		smoothed = ops.sliding_max(x, 128, absolute = True)
		dilated = ops.sliding_max(x, 4096, absolute = True)
		k = int(0.9 * smoothed.shape[1])
		case['ops'] = dict(
			sliding_max_abs_128 = with_bytes(gpu_ms(lambda: ops.sliding_max(x, 128, absolute = True)), 16 * N),
			sliding_max_abs_4096 = with_bytes(gpu_ms(lambda: ops.sliding_max(x, 4096, absolute = True)), 16 * N),
			sliding_max_abs_16384 = with_bytes(gpu_ms(lambda: ops.sliding_max(x, 16384, absolute = True)), 16 * N),
			sliding_min_4096 = with_bytes(gpu_ms(lambda: ops.sliding_max(dilated, 4096, minimum = True)), 16 * N),
			kth_value = with_bytes(gpu_ms(lambda: ops.kth_value(smoothed, k)), 3 * 8 * N),
			sign_prefix_sum = with_bytes(gpu_ms(lambda: ops.sign_prefix_sum(smoothed)), 2 * 8 * N + 4 * N),
		)
		parts = sum(case['ops'][n]['median_ms'] for n in ('sliding_max_abs_128', 'sliding_max_abs_4096', 'sliding_min_4096', 'kth_value', 'sign_prefix_sum'))
		case['ops']['combine_by_difference_ms'] = case['select_speaker']['median_ms'] - parts
		case['select_speaker'] = with_bytes(case['select_speaker'], (16 + 16 + 16 + 24 + 20 + 12 + 8 + 7) * N)
		mask = D.select_speaker(x, **REF)[1]
		case['rle1d_mask_row'] = gpu_ms(lambda: ops.rle1d(mask[1]))
		case['diarize'] = gpu_ms(lambda: D.diarize(x, rate), runs = 5)
		print(json.dumps(case), flush = True)
		res['cases'].append(case)
		del x, smoothed, dilated, mask
	json.dump(res, open(os.path.join(out, 'ours.json'), 'w'), indent = 1)


def leg_numpy(out):
	torch.set_num_threads(1)
	x = signal(300, 8000).numpy()
	times = []
	for _ in range(3):
		t0 = time.perf_counter()
		R.select_speaker(x, **REF)
		times.append(time.perf_counter() - t0)
	res = dict(seconds = 300, sample_rate = 8000, what = 'tests/_diar_ref.py select_speaker, one process (numpy, one core)', median_s = statistics.median(times), runs = times)
	print(json.dumps(res), flush = True)
	json.dump(res, open(os.path.join(out, 'numpy.json'), 'w'), indent = 1)


def stride1_pool(rows, window, kind):
	"""One stride-1 pooling of every row of a (C, L) tensor with padding window // 2: 'max' through F.max_pool1d, 'mean' through F.avg_pool1d."""
	import torch.nn.functional as F
	pool = F.max_pool1d if kind == 'max' else F.avg_pool1d
	return pool(rows[:, None, :], window, stride = 1, padding = window // 2)[:, 0, :]


def torch_formulation(signal, kernel_size_smooth_silence, kernel_size_smooth_signal, kernel_size_smooth_speaker, silence_absolute_threshold, silence_relative_threshold, eps,
                      normalization_percentile):
	"""The baseline outside the package: the same quantities through torch's O(N x K) ops on the signal's device -- three max_pool1d calls,
	one kthvalue, one avg_pool1d, all at stride 1.  Returns the per-channel silence flags and the smoothed speaker sign (enough to time)."""
	magnitude = torch.abs(signal)
	envelope = stride1_pool(magnitude, kernel_size_smooth_signal, 'max')
	rank = int(normalization_percentile * envelope.shape[1])
	level = torch.kthvalue(envelope, rank, dim = 1).values[:, None]
	dilated = stride1_pool(magnitude, kernel_size_smooth_silence, 'max')
	closed = torch.neg(stride1_pool(torch.neg(dilated), kernel_size_smooth_silence, 'max'))
	quiet = torch.logical_or(closed < silence_absolute_threshold, closed / (level + eps) < silence_relative_threshold)
	louder = torch.sign(envelope[0] - envelope[1])
	speaker = torch.sign(stride1_pool(louder[None, :], kernel_size_smooth_speaker, 'mean')[0])
	return quiet, speaker


def leg_torch(out, seconds):
	x = signal(seconds, 8000).cuda()
	t0 = time.perf_counter()
	torch_formulation(x, **REF)
	torch.cuda.synchronize()
	first = time.perf_counter() - t0
	res = dict(seconds = seconds, sample_rate = 8000, what = 'F.max_pool1d / kthvalue / F.avg_pool1d at stride 1 on the GPU', first_call_s = first)
	if first < 20:
		res.update(gpu_ms(lambda: torch_formulation(x, **REF), warmup = 1, runs = 3))
	print(json.dumps(res), flush = True)
	json.dump(res, open(os.path.join(out, f'torch_{seconds}.json'), 'w'), indent = 1)


def leg_merge(out):
	res = json.load(open(os.path.join(out, 'ours.json')))
	res['numpy_one_core'] = json.load(open(os.path.join(out, 'numpy.json'))) if os.path.exists(os.path.join(out, 'numpy.json')) else 'not measured'
	res['torch_pooling_on_gpu'] = [json.load(open(p)) for p in sorted(glob.glob(os.path.join(out, 'torch_*.json')), key = lambda p: int(p.rsplit('_', 1)[1][:-5]))]
	json.dump(res, open(os.path.join(out, 'r07_diarization.json'), 'w'), indent = 1)


if __name__ == '__main__':
	ap = argparse.ArgumentParser()
	ap.add_argument('--leg', required = True, choices = ['ours', 'numpy', 'torch', 'merge'])
	ap.add_argument('--seconds', type = int, default = 300)
	ap.add_argument('--out', default = os.path.join(ROOT, 'profiles'))
	args = ap.parse_args()
	os.makedirs(args.out, exist_ok = True)
	if args.leg != 'merge' and args.leg != 'numpy':
		assert torch.cuda.is_available(), 'this leg measures on the GPU'
	dict(ours = lambda: leg_ours(args.out), numpy = lambda: leg_numpy(args.out), torch = lambda: leg_torch(args.out, args.seconds), merge = lambda: leg_merge(args.out))[args.leg]()
