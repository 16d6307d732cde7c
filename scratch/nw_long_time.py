"""Timing of ops.nw_align_long / ops.edit_distance_long on the GPU (README row, profiles/r12_nw_align_long.json): the crossover table a later
change of metrics.split_route's threshold is to be made from.

    python scratch/nw_long_time.py --out DIR

(a) one pair of n x n units, n = 8,000, 16,383, 55,000 (an hour of characters) and 131,071; alphabet 38, b a 5 %-edited copy of a, the
    character scores: the alignment whole (ops.nw_align_long, its workspace allocation included) and in its two parts
    (convasr_nw_align_long_parts over one workspace: the fill, then the end cell and the walk), and the distance (ops.edit_distance_long).
    At 8,000 and 16,383 the one-wave kernels (ops.nw_align, ops.edit_distance) run beside them in this process, alternating run by run;
(b) 64 pairs of 2,000 x 2,000 units on both routes.
Medians of 7 after 2 warm-up runs, device events around the calls, one process."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCORES = (5, -3, -4, -3)


def gpu_ms(*fns, warmup = 2, runs = 7):
	"""Medians of the given calls, alternating run by run."""
	for _ in range(warmup):
		for fn in fns:
			fn()
	torch.cuda.synchronize()
	times = [[] for _ in fns]
	for _ in range(runs):
		for fn, ts in zip(fns, times):
			a, b = torch.cuda.Event(enable_timing = True), torch.cuda.Event(enable_timing = True)
			a.record()
			fn()
			b.record()
			torch.cuda.synchronize()
			ts.append(a.elapsed_time(b))
	out = [dict(median_ms = statistics.median(ts), min_ms = min(ts), max_ms = max(ts), runs = runs) for ts in times]
	return out[0] if len(fns) == 1 else out


def pairs(rng, N, n, alpha = 38, p = 0.05):
	"""(N, n) int32 a and b, b a copy of a with a fraction p of its units deleted, substituted or inserted, cut or filled to n."""
	a = rng.integers(0, alpha, (N, n), dtype = np.int32)
	b = np.empty_like(a)
	for k in range(N):
		r = rng.random(n)
		row = np.where(r < 2 * p / 3, rng.integers(0, alpha, n, dtype = np.int32), a[k])
		row = np.repeat(row, np.where(r < p / 3, 0, np.where(r > 1 - p / 3, 2, 1)))
		b[k] = np.concatenate([row, rng.integers(0, alpha, n, dtype = np.int32)])[:n]
	return a, b


def measure(a, b, with_short, d):
	from convasr_amd import _lib, ops
	N, n = a.shape
	a, b = torch.from_numpy(a).to(d), torch.from_numpy(b).to(d)
	ln = torch.full((N,), n, dtype = torch.int32, device = d)
	T = ops.nw_align_long_tile()
	tiles = -(-n // T)
	res = dict(pairs = N, units = n, tile = T, fill_launches = 2 * tiles - 1, align_workspace_bytes = ops.nw_align_long_workspace_bytes(N, n, n),
	           distance_workspace_bytes = ops.edit_distance_long_workspace_bytes(N, n, n))
	ws = torch.empty(res['align_workspace_bytes'], dtype = torch.uint8, device = d)
	parts = lambda which: ops._nw_launch('convasr_nw_align_long_parts', ops.nw_align_long_workspace_bytes, a, ln, b, ln, SCORES, which, ws)
	res['fill'] = gpu_ms(lambda: parts(1))
	res['walk'] = gpu_ms(lambda: parts(2))
	del ws
	a64, l64 = a.long(), ln.long()
	b64 = b.long()
	long_align, long_dist = (lambda: ops.nw_align_long(a, ln, b, ln, SCORES)), (lambda: ops.edit_distance_long(a, ln, b, ln))
	if with_short:
		res['align'], res['align_one_wave'] = gpu_ms(long_align, lambda: ops.nw_align(a, ln, b, ln, SCORES))
		res['distance'], res['distance_one_wave'] = gpu_ms(long_dist, lambda: ops.edit_distance(a64, l64, b64, l64, _lib.METRIC_CHARS, -1))
		res['align_one_wave_over_tiled'] = res['align_one_wave']['median_ms'] / res['align']['median_ms']
		res['distance_one_wave_over_tiled'] = res['distance_one_wave']['median_ms'] / res['distance']['median_ms']
		res['equal'] = bool(all(torch.equal(x, y) for x, y in zip(long_align(), ops.nw_align(a, ln, b, ln, SCORES)))
		                    and torch.equal(long_dist(), ops.edit_distance(a64, l64, b64, l64, _lib.METRIC_CHARS, -1)[0]))
	else:
		res['align'], res['distance'] = gpu_ms(long_align), gpu_ms(long_dist)
	res['walk_share_of_align'] = res['walk']['median_ms'] / res['align']['median_ms']
	return res


def main(out_dir):
	d = torch.device('cuda:0')
	rng = np.random.default_rng(12)
	res = dict(device = torch.cuda.get_device_name(0), scores = SCORES, single_pair = {}, batch = {})
	for n in (8000, 16383, 55000, 131071):
		r = measure(*pairs(rng, 1, n), n <= 16383, d)
		print(json.dumps(r), flush = True)
		res['single_pair'][str(n)] = r
	r = measure(*pairs(rng, 64, 2000), True, d)
	print(json.dumps(r), flush = True)
	res['batch']['64x2000'] = r
	os.makedirs(out_dir, exist_ok = True)
	json.dump(res, open(os.path.join(out_dir, 'r12_nw_align_long.json'), 'w'), indent = 1)


if __name__ == '__main__':
	ap = argparse.ArgumentParser()
	ap.add_argument('--out', default = os.path.join(ROOT, 'profiles'))
	args = ap.parse_args()
	assert torch.cuda.is_available(), 'this script measures on the GPU'
	main(args.out)
