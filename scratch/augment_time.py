"""Timing of the training-time augmentation on the GPU (README row, profiles/r17_augment.json).

    python scratch/augment_time.py --out DIR [--quick]

Medians of 7 runs after 2 warm-up runs, device events around the C calls (the Python wrappers' allocations included: they launch nothing).
(a) the waveform pass on 64 x 15 s at 16 kHz with the speed table (0.9, 1.0, 1.1) and a noise bank, and with speed 1.0 only (gain, no noise),
    against a clone() of the same tensor: the one-read-one-write floor;
(b) SpecAugment on 64 x 64 x 1,501 log-mel features against its clone();
(c) one Wav2Letter bf16 training step on the benchmark batch with and without both augmentations, in the same process, alternating: the step
    without augmentation is the code path that exists without this module."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
	p.add_argument('--quick', action = 'store_true', help = 'a small batch (a rehearsal of the script)')
	args = p.parse_args()
	import convasr_amd as ca
	from convasr_amd import augment, ops
	os.makedirs(args.out, exist_ok = True)
	assert torch.cuda.is_available(), 'a measurement needs the GPU'
	d = torch.device('cuda:0')
	B, secs = (8, 2) if args.quick else (64, 15)
	T = 16000 * secs
	g = torch.Generator().manual_seed(1)
	record = dict(device = torch.cuda.get_device_name(0), note = "the runtime names the MI355X 'AMD Radeon Graphics'", batch = B, seconds = secs)

	# (a) waveforms: utterances of 70 to 90 % of the padded length, so that every speed fits
	x = (torch.rand(B, T, generator = g) * 2 - 1).to(d)
	xlen = (0.7 + 0.2 * torch.rand(B, generator = g)).to(d)
	keys = torch.arange(B, dtype = torch.int64, device = d)
	noise = (torch.rand(16, 16000 * 10, generator = g) * 0.2 - 0.1).to(d)
	nbytes = 2 * x.numel() * 4
	floor = gpu_ms(lambda: x.clone())
	record['waveform'] = dict(bytes = nbytes, clone = dict(floor, bytes_per_s = nbytes / (floor['median_ms'] * 1e-3)))
	for name, aug in (('speed_gain_noise', augment.WaveformAugment(seed = 1, noise = noise, noise_prob = 1.0)), ('speed_one_gain', augment.WaveformAugment(seed = 1, speed = (1.0, )))):
		t = gpu_ms(lambda: aug(x, xlen, keys, epoch = 1))
		params, _ = aug.params(xlen, keys, T, epoch = 1)
		resampled = int(params['out_len'][params['step'] != ops.AUG_ONE].sum())
		sec = t['median_ms'] * 1e-3
		record['waveform'][name] = dict(t, over_clone = t['median_ms'] / floor['median_ms'], bytes_per_s = nbytes / sec, fraction_of_hbm_peak = nbytes / sec / HBM_PEAK, taps = aug.taps, resampled_outputs = resampled,
		                                lds_reads_per_s = resampled * aug.taps * 3 / sec, fma_per_s = resampled * aug.taps * 2 / sec)
		print(name, record['waveform'][name], flush = True)

	# (b) SpecAugment
	F, frames = 64, 1 + T // 160
	feats = torch.randn(B, F, frames, generator = g).to(d)
	spec = augment.SpecAugment(seed = 1).to(d)
	spec.set_keys(keys, 1)
	nbytes = 2 * feats.numel() * 4
	floor = gpu_ms(lambda: feats.clone())
	record['spec_augment'] = dict(shape = [B, F, frames], bytes = nbytes, clone = dict(floor, bytes_per_s = nbytes / (floor['median_ms'] * 1e-3)))
	for fill in ('mean', 0.0):
		spec.fill = fill
		t = gpu_ms(lambda: spec(feats, xlen))
		record['spec_augment'][f'fill_{fill}'] = dict(t, over_clone = t['median_ms'] / floor['median_ms'], bytes_per_s = nbytes / (t['median_ms'] * 1e-3))
		print('spec', fill, record['spec_augment'][f'fill_{fill}'], flush = True)
	spec.fill = 'mean'

	# (c) one training step, alternating plain / augmented
	torch.manual_seed(1)
	fe = ca.models.LogFilterBankFrontend(64, 16000, 0.02, 0.01, 'hann_window')
	model = ca.models.Wav2Letter(64, [38], frontend = fe, dropout = 0.2, check_time_dim_padded = False, compute_dtype = torch.bfloat16).to(d).train()
	opt = ca.train.SGD(ca.train.FlatParameters(model), lr = 1e-2, momentum = 0.9, weight_decay = 1e-3)
	y = torch.randint(0, 37, (B, 1, 10 * secs), generator = g).to(d)
	ylen = torch.full((B, 1), 5 * secs, dtype = torch.long, device = d)
	wave = augment.WaveformAugment(seed = 1, noise = noise)
	min_out_len = ylen[:, 0] * 320

	def plain():
		model.feature_transform = None
		ca.train.train_step(model, opt, x, xlen, y, ylen)

	def augmented():
		model.feature_transform = spec
		spec.set_keys(keys, 1)
		xa, xla = wave(x, xlen, keys, epoch = 1, min_out_len = min_out_len)
		ca.train.train_step(model, opt, xa, xla, y, ylen)

	for fn in (plain, augmented, plain, augmented):
		fn()
	torch.cuda.synchronize()
	times = dict(plain = [], augmented = [])
	for _ in range(7):
		for name, fn in (('plain', plain), ('augmented', augmented)):
			a, b = torch.cuda.Event(enable_timing = True), torch.cuda.Event(enable_timing = True)
			a.record()
			fn()
			b.record()
			torch.cuda.synchronize()
			times[name].append(a.elapsed_time(b))
	med = {k: statistics.median(v) for k, v in times.items()}
	record['train_step'] = dict(model = 'Wav2Letter bf16, eager train_step', plain_ms = med['plain'], augmented_ms = med['augmented'], plain_min_max = [min(times['plain']), max(times['plain'])],
	                            augmented_min_max = [min(times['augmented']), max(times['augmented'])], cost_share_of_step = (med['augmented'] - med['plain']) / med['plain'], runs = 7)
	print(record['train_step'], flush = True)
	with open(os.path.join(args.out, 'r17_augment.json'), 'w') as f:
		json.dump(record, f, indent = 1)


if __name__ == '__main__':
	main()
