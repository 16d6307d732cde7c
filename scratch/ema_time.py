"""Timing of the weight average on the GPU (README row, DESIGN, profiles/r23_ema.json).  Wav2Letter of the benchmark (66.5M parameters,
bf16 compute, SGD, dropout 0.2) on the benchmark batch, 64 x 15 s:
  * WeightEMA.update (one launch over the arena: reads w and e, writes e and the bf16 mirror, 14 bytes per element) against clone() of the
    arena (8 bytes per element), alternating; the expectation to compare with is the byte ratio, 1.75;
  * one eager training step with ema and without, alternating;
  * entering plus leaving average_parameters() (four exchange launches: the arenas, 16 bytes per element, and the mirrors, 8);
  * with --parent TREE: the same eager step, without ema, by the package under TREE (a checkout of the parent commit, built), in a process
    of its own started from here.
DEVICE EVENTS around the calls, medians of 7 after 2 warm-ups, with min and max.  Usage: python scratch/ema_time.py --out DIR [--parent TREE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

WARMUP, RUNS = 2, 7


def stats(ms):
	return dict(median_ms = statistics.median(ms), min_ms = min(ms), max_ms = max(ms), runs = len(ms))


def events(fns):
	"""Device-event times (ms) of every callable in fns, alternating, WARMUP + RUNS rounds."""
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


def workload(ca, d):
	torch.manual_seed(0)
	fe = ca.models.LogFilterBankFrontend(64, 16000, 0.02, 0.01, 'hann_window')
	model = ca.models.Wav2Letter(64, [38], frontend = fe, dropout = 0.2, check_time_dim_padded = False, compute_dtype = torch.bfloat16).to(d).train()
	flat = ca.train.FlatParameters(model)
	opt = ca.train.SGD(flat, lr = 1e-4, momentum = 0.9, weight_decay = 1e-3)
	g = torch.Generator().manual_seed(1)
	x = (torch.rand(64, 16000 * 15, generator = g) * 2 - 1).to(d)
	y = torch.randint(0, 37, (64, 1, 150), generator = g).to(d)
	return model, flat, opt, (x, torch.ones(64, device = d), y, torch.full((64, 1), 150, dtype = torch.long, device = d))


def parent_step(tree):
	"""This process runs the package under `tree`: the eager step alone."""
	sys.path.insert(0, os.path.abspath(tree))
	import convasr_amd as ca
	assert os.path.abspath(ca.__file__).startswith(os.path.abspath(tree)), ca.__file__
	d = torch.device('cuda:0')
	model, flat, opt, batch = workload(ca, d)
	it = [0]

	def run():
		ca.train.train_step(model, opt, *batch, iteration = it[0])
		it[0] += 1
	print(json.dumps(stats(events(dict(step = run))['step'])))


def measure(args):
	sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
	import convasr_amd as ca
	d = torch.device('cuda:0')
	model, flat, opt, batch = workload(ca, d)
	ema = ca.train.WeightEMA(flat, decay = 0.999)
	it = [0]

	def run(e):
		ca.train.train_step(model, opt, *batch, iteration = it[0], ema = e)
		it[0] += 1
	run(ema)  # (the first step allocates the mirrors)
	step = events({'without ema': lambda: run(None), 'with ema': lambda: run(ema)})
	keep = {}

	def clone():
		keep['c'] = flat.data.clone()

	def context():
		with ema.average_parameters():
			pass
	arena = events({'clone': clone, 'update': ema.update, 'enter + leave average_parameters': context})
	med = {k: statistics.median(v) for k, v in {**step, **arena}.items()}
	n = flat.numel
	res = dict(device = torch.cuda.get_device_name(0),
	           note = "the runtime names the MI355X 'AMD Radeon Graphics'; device_events: torch.cuda.Event pairs around the calls, alternating in one process; medians of 7 after 2 warm-ups",
	           warmup = WARMUP, model = 'Wav2Letter', dtype = 'bfloat16', batch = 64, seconds = 15, arena_elements = n,
	           arena = dict(device_events = {k: stats(v) for k, v in arena.items()}, update_over_clone = med['update'] / med['clone'], expected_from_bytes = 14 / 8,
	                        update_GBps = 14 * n / med['update'] / 1e6, clone_GBps = 8 * n / med['clone'] / 1e6, context_GBps = 2 * 24 * n / med['enter + leave average_parameters'] / 1e6),
	           step = dict(device_events = {k: stats(v) for k, v in step.items()}, added_ms = med['with ema'] - med['without ema'], with_over_without = med['with ema'] / med['without ema']))
	if args.parent:
		out = subprocess.run([sys.executable, os.path.abspath(__file__), '--parent-step', args.parent], capture_output = True, text = True, timeout = 300)
		if out.returncode != 0:
			raise RuntimeError('the parent leg failed:\n' + out.stdout + out.stderr)
		res['step']['parent_commit_without_ema'] = json.loads(out.stdout.strip().splitlines()[-1])
		res['step']['without_ema_over_parent'] = med['without ema'] / res['step']['parent_commit_without_ema']['median_ms']
	os.makedirs(args.out, exist_ok = True)
	with open(os.path.join(args.out, 'r23_ema.json'), 'w') as f:
		json.dump(res, f, indent = 1)
	print(json.dumps(res))


if __name__ == '__main__':
	ap = argparse.ArgumentParser()
	ap.add_argument('--out')
	ap.add_argument('--parent', default = None)
	ap.add_argument('--parent-step', default = None)
	args = ap.parse_args()
	if args.parent_step:
		parent_step(args.parent_step)
	else:
		measure(args)
