"""Timing of the room reverberation on the GPU (README row, profiles/r20_reverb.json).

    python scratch/reverb_time.py --out DIR [--quick]
    rocprofv3 --kernel-trace --stats -d DIR/trace -- python scratch/reverb_time.py --out DIR --trace    (a run of its own: the three kernels' shares)

Medians of 7 runs after 2 warm-up runs with min - max, device events around the calls, everything in one process and alternating where two things
are compared.  Two workloads: 64 x 15 s at 16 kHz with 8,000-tap impulse responses and 64 x 15 s at 8 kHz with 3,200-tap ones.  For each:
(a) ops.augment_reverb (three launches; every utterance reverberated, each with its own row of a 32-row bank of equal lengths) against a clone()
    of the batch and against the torch.fft whole-batch formulation on the same device -- rfft of the padded batch, one shared impulse response
    (the only case it can express), irfft, the same shift and cut;
(b) the largest difference between the two on one shared impulse response, so that the timed results are known to agree;
and, at 16 kHz, (c) one eager Wav2Letter bf16 training step with the waveform augmentation without and with the bank, alternating, and the plain
step without any augmentation: the code path that exists without this module."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alternate(fns, warmup = 2, runs = 7):
	for _ in range(warmup):
		for fn in fns.values():
			fn()
	torch.cuda.synchronize()
	times = {k: [] for k in fns}
	for _ in range(runs):
		for name, fn in fns.items():
			a, b = torch.cuda.Event(enable_timing = True), torch.cuda.Event(enable_timing = True)
			a.record()
			fn()
			b.record()
			torch.cuda.synchronize()
			times[name].append(a.elapsed_time(b))
	return {k: dict(median_ms = statistics.median(v), min_ms = min(v), max_ms = max(v), runs = runs) for k, v in times.items()}


def main():
	p = argparse.ArgumentParser()
	p.add_argument('--out', required = True)
	p.add_argument('--quick', action = 'store_true', help = 'a small batch (a rehearsal of the script)')
	p.add_argument('--trace', action = 'store_true', help = 'only 20 calls of ops.augment_reverb on the 16 kHz workload, for a kernel trace; writes nothing')
	args = p.parse_args()
	import convasr_amd as ca
	from convasr_amd import augment, ops
	os.makedirs(args.out, exist_ok = True)
	assert torch.cuda.is_available(), 'a measurement needs the GPU'
	d = torch.device('cuda:0')
	B, secs = (8, 2) if args.quick else (64, 15)
	g = torch.Generator().manual_seed(1)
	Bk = ops.reverb_block()
	record = dict(device = torch.cuda.get_device_name(0), note = "the runtime names the MI355X 'AMD Radeon Graphics'", batch = B, seconds = secs, block = Bk, workloads = {})

	for rate, taps in ((16000, 8000), (8000, 3200)):
		T = rate * secs
		y = (torch.rand(B, T, generator = g) - 0.5).to(d)
		out_len = (T * (0.7 + 0.3 * torch.rand(B, generator = g))).long()
		params = torch.zeros(B, 8, dtype = torch.int64)
		params[:, 0], params[:, 1], params[:, 2], params[:, 3], params[:, 6], params[:, 7] = -1, ops.AUG_ONE, -1, -1, out_len, out_len
		params = params.to(d)
		y = y * (torch.arange(T, device = d)[None, :] < params[:, 7:8])
		R = 32
		bank = torch.randn(R, taps, generator = g) * torch.exp(-6.9 * torch.arange(taps) / taps)
		bank[:, 0] = 4.0
		bank = bank / bank.pow(2).sum(dim = 1, keepdim = True).sqrt()
		lengths, delays = torch.full((R,), taps, dtype = torch.int64), ops.rir_delays(bank, torch.full((R,), taps))
		rir, dl, dd = bank.to(d), lengths.to(d), delays.to(d)
		rows = (torch.arange(B) % R).to(d)
		shared = torch.zeros(B, dtype = torch.int64, device = d)
		nf = 1 << (T + taps - 1).bit_length()

		def hip(r = rows):
			return ops.augment_reverb(y, params, r, rir, dl, dd, host = (lengths, delays))[0]

		def fft():
			Hs = torch.fft.rfft(rir[0], nf)
			return torch.fft.irfft(torch.fft.rfft(y, nf) * Hs, nf)[:, :T] * (torch.arange(T, device = d)[None, :] < params[:, 7:8])

		if args.trace:
			for _ in range(20):
				hip()
			torch.cuda.synchronize()
			return
		diff = float((hip(shared) - fft()).abs().max())
		t = alternate(dict(clone = lambda: y.clone(), reverb = hip, torch_fft = fft))
		P = -(-taps // Bk)
		blocks = int(((out_len + Bk - 1) // Bk + 1).div(2, rounding_mode = 'floor').sum())
		w = dict(sample_rate = rate, T = T, taps = taps, parts = P, fft_points = 2 * Bk, forward_ffts = blocks + 2 * B * P, inverse_ffts = blocks, workspace_bytes = int(ops._cached_query('convasr_augment_reverb_workspace_bytes', B, T, taps)),
		         spectra_bytes_read_by_apply = blocks * P * 2 * (2 * Bk) * 8, max_abs_difference_to_torch_fft_shared_rir = diff, **t)
		w['reverb_over_clone'] = t['reverb']['median_ms'] / t['clone']['median_ms']
		w['reverb_over_torch_fft'] = t['reverb']['median_ms'] / t['torch_fft']['median_ms']
		record['workloads'][f'{rate}Hz_{taps}taps'] = w
		print(rate, taps, w, flush = True)
		del y

	# (c) one training step at 16 kHz: plain, augmented without a bank, augmented with one
	rate, taps = 16000, 8000
	T = rate * secs
	torch.manual_seed(1)
	x = (torch.rand(B, T, generator = g) * 2 - 1).to(d)
	xlen = (0.7 + 0.2 * torch.rand(B, generator = g)).to(d)
	keys = torch.arange(B, dtype = torch.int64, device = d)
	noise = (torch.rand(16, rate * 10, generator = g) * 0.2 - 0.1).to(d)
	fe = ca.models.LogFilterBankFrontend(64, rate, 0.02, 0.01, 'hann_window')
	model = ca.models.Wav2Letter(64, [38], frontend = fe, dropout = 0.2, check_time_dim_padded = False, compute_dtype = torch.bfloat16).to(d).train()
	opt = ca.train.SGD(ca.train.FlatParameters(model), lr = 1e-2, momentum = 0.9, weight_decay = 1e-3)
	lab = torch.randint(0, 37, (B, 1, 10 * secs), generator = g).to(d)
	lablen = torch.full((B, 1), 5 * secs, dtype = torch.long, device = d)
	bank, lengths = augment.synthetic_rirs(32, rate, rt60 = (0.5, 0.5))
	dry = augment.WaveformAugment(seed = 1, noise = noise)
	wet = augment.WaveformAugment(seed = 1, noise = noise, rir = bank.to(d), rir_lengths = lengths, reverb_prob = 1.0)
	min_out_len = lablen[:, 0] * 320

	def step(wave):
		def run():
			if wave is None:
				ca.train.train_step(model, opt, x, xlen, lab, lablen)
			else:
				xa, xla = wave(x, xlen, keys, epoch = 1, min_out_len = min_out_len)
				ca.train.train_step(model, opt, xa, xla, lab, lablen)
		return run

	t = alternate(dict(plain = step(None), augmented = step(dry), augmented_reverb = step(wet)))
	launches = alternate(dict(waveform = lambda: dry(x, xlen, keys, epoch = 1, min_out_len = min_out_len), waveform_reverb = lambda: wet(x, xlen, keys, epoch = 1, min_out_len = min_out_len)))
	record['train_step'] = dict(model = 'Wav2Letter bf16, eager train_step', rir_taps = int(lengths.max()), reverb_prob = 1.0, **t, augmentation_alone = launches,
	                            reverb_share_of_step = (t['augmented_reverb']['median_ms'] - t['augmented']['median_ms']) / t['plain']['median_ms'])
	print(record['train_step'], flush = True)
	with open(os.path.join(args.out, 'r20_reverb.json'), 'w') as f:
		json.dump(record, f, indent = 1)


if __name__ == '__main__':
	main()
