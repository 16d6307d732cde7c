"""Timing of ctc.star_alignment on the GPU next to ctc.alignment_long (README row, DESIGN 7o, profiles/r24_star_alignment.json).

    python scratch/star_align_time.py --out DIR

Shapes: 8,000 labels x 60,000 frames (random log-probs); one hour, 48,000 labels x 180,000 frames (planted, with four inserts of
1,500 frames in word gaps); 64 x 753 frames x 150 labels (random).  The labels have a space before every sixth one.  Masks: all-false
and 'words'.  Device events around convasr_star_alignment_parts over one workspace -- the sweep, the walk, both -- around the whole
ops.star_ctc_alignment call (unit table, read-back and workspace allocation included) and around ops.ctc_alignment_long on the same
log-probs and targets, the five taken in turn inside every repetition; medians of 7 repetitions after 2 warm-ups, with min and max."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _star_align_ref as A  # noqa: E402

C, BLANK, SPACE = 38, 37, 36
PENALTY, ENTER = -1.0, -2.0


def in_turn(fns, warmup = 2, runs = 7):
	times = {k: [] for k in fns}
	for rep in range(warmup + runs):
		for k, fn in fns.items():
			a, b = torch.cuda.Event(enable_timing = True), torch.cuda.Event(enable_timing = True)
			a.record()
			fn()
			b.record()
			torch.cuda.synchronize()
			if rep >= warmup:
				times[k].append(a.elapsed_time(b))
	return {k: dict(median_ms = statistics.median(v), min_ms = min(v), max_ms = max(v), runs = runs) for k, v in times.items()}


def worded_labels(seed, B, S, every = 6):
	labels = np.random.RandomState(seed).randint(0, 33, size = (B, S)).astype(np.int64)
	labels[:, every - 1::every] = SPACE
	return labels


def measure(lp_btc, tg, il, tl, mode):
	import convasr_amd as ca
	d = lp_btc.device
	tg, il, tl = tg.to(d), il.to(d), tl.to(d)
	mask = ca.ctc.star_gaps(tg, tl, 'words', SPACE) if mode == 'words' else torch.zeros(tg.shape[0], tg.shape[1] + 1, dtype = torch.bool, device = d)
	star = lambda **kw: ca.ops.star_ctc_alignment(lp_btc, tg, il, tl, BLANK, mask, PENALTY, ENTER, **kw)
	swept = star(parts = 1)
	units, n_units, N_max, nbytes, ws = swept._reuse
	sb, chunk = ca.ops.star_alignment_tiles()
	B, T, _ = lp_btc.shape
	res = dict(mask = mode, units_max = N_max, stars = int(mask.sum()), workspace_bytes = nbytes, launches_at_most = -(-T // chunk) + -(-(2 * N_max + 1) // sb) - 1 + 1,
	           alignment_long_workspace_bytes = ca.ops._query('convasr_ctc_alignment_long_workspace_bytes', B, T, tg.shape[1]))
	res.update(in_turn(dict(sweep = lambda: star(parts = 1, _reuse = swept._reuse), walk = lambda: star(parts = 2, _reuse = swept._reuse), both = lambda: star(parts = 3, _reuse = swept._reuse),
	                        call = lambda: star(), alignment_long_call = lambda: ca.ops.ctc_alignment_long(lp_btc, tg, il, tl, BLANK))))
	res['star_call_over_alignment_long_call'] = res['call']['median_ms'] / res['alignment_long_call']['median_ms']
	parts, whole = star(parts = 2, _reuse = swept._reuse), star()
	assert all(torch.equal(getattr(parts, k), getattr(whole, k)) for k in ('alignment', 'star_begin', 'star_frames', 'score'))
	del swept, units, ws
	return res, whole


def main(out_dir):
	import convasr_amd as ca
	d = torch.device('cuda:0')
	res = dict(device = torch.cuda.get_device_name(0), states_per_block = ca.ops.star_alignment_tiles()[0], default_chunk_frames = ca.ops.star_alignment_tiles()[1], penalty = PENALTY, enter = ENTER, cases = [])
	gen = torch.Generator().manual_seed(8)
	for name, B, T, S in (('8000_labels_60000_frames', 1, 60000, 8000), ('64_x_753_frames_150_labels', 64, 753, 150)):
		lp = torch.randn(B, T, C, generator = gen).log_softmax(-1).to(d)
		tg = torch.from_numpy(worded_labels(3, B, S))
		il = torch.full((B, ), T) if B == 1 else torch.randint(2 * S + 1, T + 1, (B, ), generator = gen)
		tl = torch.full((B, ), S) if B == 1 else torch.randint(1, S + 1, (B, ), generator = gen)
		for mode in ('none', 'words'):
			r, _ = measure(lp, tg, il, tl, mode)
			r.update(case = name, B = B, frames = T, labels = S)
			print(json.dumps(r), flush = True)
			res['cases'].append(r)
		del lp
	T, S, Tb = 180000, 48000, 179500
	labels = worded_labels(7, 1, S)
	inserts = {5: 1500, 12005: 1500, 30005: 1500, 47999: 1500}
	assert all(labels[0, g] == SPACE for g in inserts)
	lp_np, pos, runs = A.planted(7, T, labels[0], C, BLANK, inserts, input_length = Tb)
	lp, tg, il, tl = torch.from_numpy(lp_np).unsqueeze(0).to(d), torch.from_numpy(labels), torch.tensor([Tb]), torch.tensor([S])
	for mode in ('none', 'words'):
		r, whole = measure(lp, tg, il, tl, mode)
		r.update(case = 'one_hour', B = 1, frames = T, input_length = Tb, labels = S)
		if mode == 'words':
			begin, frames = whole.star_begin[0].cpu().numpy(), whole.star_frames[0].cpu().numpy()
			r['equals_planted'] = bool(np.array_equal(whole.alignment[0].cpu().numpy(), pos)) and all((begin[g], frames[g]) == (runs[g] if g in runs else (-1, 0)) for g in range(S + 1))
		print(json.dumps(r), flush = True)
		res['cases'].append(r)
	os.makedirs(out_dir, exist_ok = True)
	json.dump(res, open(os.path.join(out_dir, 'r24_star_alignment.json'), 'w'), indent = 1)


if __name__ == '__main__':
	ap = argparse.ArgumentParser()
	ap.add_argument('--out', default = os.path.join(ROOT, 'profiles'))
	args = ap.parse_args()
	assert torch.cuda.is_available(), 'this script measures on the GPU'
	main(args.out)
