"""Timing of the star-token CTC loss on the GPU (README row, DESIGN, profiles/r21_star_ctc.json).
  * convasr_star_ctc_loss (both launches, with the gradient) at 64 x 753 frames, 150 labels, 38 classes for the gaps 'ends', 'words'
    (a space every sixth label) and 'all', against convasr_ctc_loss on the same tensors: DEVICE EVENTS around the C entry points, output
    buffers and workspaces allocated outside, alternating in one process;
  * one eager Wav2Letter bf16 training step (SGD, dropout 0.2) on the benchmark batch with and without model.ctc_star (gaps 'words'):
    DEVICE EVENTS around train_step, alternating.
Medians of 7 after 2 warm-ups, with min and max.  Usage: python scratch/star_ctc_time.py --out DIR"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import convasr_amd as ca  # noqa: E402
from convasr_amd import ctc, ops  # noqa: E402

WARMUP, RUNS = 2, 7
SPACE, PENALTY, ENTER = 36, -0.5, -1.0


def stats(ms):
	return dict(median_ms = statistics.median(ms), min_ms = min(ms), max_ms = max(ms), runs = len(ms))


def events(fns):
	"""Device-event times (ms) of every callable in fns, alternating, WARMUP + RUNS rounds; the callables only enqueue."""
	times = {k: [] for k in fns}
	for rep in range(WARMUP + RUNS):
		marks = {}
		for k, fn in fns.items():
			a, b = torch.cuda.Event(enable_timing = True), torch.cuda.Event(enable_timing = True)
			a.record()
			fn()
			b.record()
			marks[k] = (a, b)
		torch.cuda.synchronize()
		if rep >= WARMUP:
			for k, (a, b) in marks.items():
				times[k].append(a.elapsed_time(b))
	return times


def kernels(B, T, C, S, d):
	g = torch.Generator().manual_seed(0)
	lp = ops.as_cl((torch.randn(B, C, T, generator = g) * 2).log_softmax(dim = 1).to(d))
	y = torch.randint(0, C - 2, (B, S), generator = g)
	y[:, 5::6] = SPACE
	y = y.to(d)
	olen, ylen = torch.full((B, ), T, dtype = torch.int64, device = d), torch.full((B, ), S, dtype = torch.int64, device = d)
	nll, frames, grad = torch.empty(B, dtype = torch.float32, device = d), torch.empty(B, S + 1, dtype = torch.float32, device = d), ops.empty_cl(B, C, T, torch.float32, d)
	ws_star = torch.empty(ops._query('convasr_star_ctc_workspace_bytes', B, T, C, S), dtype = torch.uint8, device = d)
	ws_plain = torch.empty(ops._cached_query('convasr_ctc_workspace_bytes', B, T, S), dtype = torch.uint8, device = d)
	P, St = ops.ptr, ops.stream_ptr
	masks = {mode: ctc.star_gaps(y, ylen, mode, space = SPACE).contiguous() for mode in ctc.STAR_GAP_MODES}
	fns = dict(ctc_loss = lambda: ops.call('convasr_ctc_loss', P(lp), P(y), P(olen), P(ylen), P(nll), P(grad), P(ws_plain), B, T, C, S, C - 1, St()))
	for mode, m in masks.items():
		fns['star_' + mode] = lambda m = m: ops.call('convasr_star_ctc_loss', P(lp), P(y), P(olen), P(ylen), P(m), PENALTY, ENTER, P(nll), P(grad), P(frames), P(ws_star), B, T, C, S, C - 1, St())
	t = events(fns)
	med = {k: statistics.median(v) for k, v in t.items()}
	return dict(B = B, T = T, classes = C, labels = S, states = {mode: int(2 * (S + int(m[0].sum())) + 1) for mode, m in masks.items()}, penalty = PENALTY, enter = ENTER,
	            workspace_bytes = dict(star = ws_star.numel(), plain = ws_plain.numel()), device_events = {k: stats(v) for k, v in t.items()},
	            over_ctc_loss = {k: med[k] / med['ctc_loss'] for k in med if k != 'ctc_loss'})


def step(d):
	torch.manual_seed(0)
	fe = ca.models.LogFilterBankFrontend(64, 16000, 0.02, 0.01, 'hann_window')
	model = ca.models.Wav2Letter(64, [38], frontend = fe, dropout = 0.2, check_time_dim_padded = False, compute_dtype = torch.bfloat16).to(d).train()
	opt = ca.train.SGD(ca.train.FlatParameters(model), lr = 1e-4, momentum = 0.9, weight_decay = 1e-3)
	g = torch.Generator().manual_seed(1)
	x = (torch.rand(64, 16000 * 15, generator = g) * 2 - 1).to(d)
	xlen = torch.ones(64, device = d)
	y = torch.randint(0, 36, (64, 1, 150), generator = g)
	y[:, 0, 5::6] = SPACE
	y = y.to(d)
	ylen = torch.full((64, 1), 150, dtype = torch.long, device = d)
	star = ctc.StarCTC('words', penalty = PENALTY, enter = ENTER, space = SPACE)
	it = [0]

	def run(option):
		model.ctc_star = option
		ca.train.train_step(model, opt, x, xlen, y, ylen, iteration = it[0])
		it[0] += 1
	t = events(dict(plain = lambda: run(None), with_star = lambda: run(star)))
	med = {k: statistics.median(v) for k, v in t.items()}
	return dict(model = 'Wav2Letter', dtype = 'bfloat16', batch = 64, seconds = 15, gaps = 'words', device_events = {k: stats(v) for k, v in t.items()}, with_star_over_plain = med['with_star'] / med['plain'],
	            added_ms = med['with_star'] - med['plain'])


if __name__ == '__main__':
	ap = argparse.ArgumentParser()
	ap.add_argument('--out', required = True)
	args = ap.parse_args()
	d = torch.device('cuda:0')
	res = dict(device = torch.cuda.get_device_name(0),
	           note = "the runtime names the MI355X 'AMD Radeon Graphics'; device_events: torch.cuda.Event pairs around the C entry points (kernels) or around train_step (step), alternating in one process; medians of 7 after 2 warm-ups",
	           warmup = WARMUP, kernels = kernels(64, 753, 38, 150, d), step = step(d))
	os.makedirs(args.out, exist_ok = True)
	with open(os.path.join(args.out, 'r21_star_ctc.json'), 'w') as f:
		json.dump(res, f, indent = 1)
	print(json.dumps(res))
