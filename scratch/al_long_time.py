"""Timing of ctc.alignment_long on the GPU (README row, profiles/r08_alignment_long.json).

    python scratch/al_long_time.py --out DIR

(a) 8,000 labels x 60,000 frames (random log-probs, the case of scratch/al_time.py): ctc.alignment and ctc.alignment_long in this process
    on the same device;
(b) the one-hour case of tests/test_ctc_alignment_long_gpu.py: 48,000 planted labels over 180,000 frames, default chunk length;
(c) (b) at other chunk lengths.
Medians over repeated runs after a warm-up, device events around the calls.  The long form is timed whole (ctc.alignment_long, its
workspace allocation included) and in its two parts (convasr_ctc_alignment_long_parts over one workspace: the sweep, then the walk)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _ctc_align_ref as R  # noqa: E402

C = 38


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


def long_form(lp_tbc, tg, il, tl, chunk_frames):
	"""Whole call, sweep and walk of ctc.alignment_long at one chunk length."""
	import convasr_amd as ca
	from convasr_amd import _lib
	from convasr_amd._lib import call, ptr, stream_ptr
	lib = _lib.load()
	d = lp_tbc.device
	lp = lp_tbc.permute(1, 0, 2).contiguous()
	B, T, _ = lp.shape
	tg, il, tl = tg.to(d), il.to(d), tl.to(d)
	S_max = tg.shape[1]
	nbytes = lib.convasr_ctc_alignment_long_workspace_bytes(B, T, S_max)
	ws = torch.empty(nbytes, dtype = torch.uint8, device = d)
	out = torch.empty(B, S_max, dtype = torch.int64, device = d)
	part = lambda parts: call('convasr_ctc_alignment_long_parts', ptr(lp), ptr(tg), ptr(il), ptr(tl), ptr(out), ptr(ws), nbytes, B, T, C, S_max, C - 1, chunk_frames, parts, stream_ptr())
	sb, default = ca.ops.ctc_alignment_long_tiles()
	chunk = chunk_frames or default
	res = dict(chunk_frames = chunk, workspace_bytes = nbytes, launches_at_most = -(-T // chunk) + -(-(2 * S_max + 1) // sb) - 1)
	res['sweep'] = gpu_ms(lambda: part(1))
	res['walk'] = gpu_ms(lambda: part(2))
	res['both'] = gpu_ms(lambda: part(3))
	parts_result = out.clone()
	del ws
	res['call'] = gpu_ms(lambda: ca.ops.ctc_alignment_long(lp, tg, il, tl, C - 1, chunk_frames = chunk_frames))
	res['walk_share_of_both'] = res['walk']['median_ms'] / res['both']['median_ms']
	whole = ca.ops.ctc_alignment_long(lp, tg, il, tl, C - 1, chunk_frames = chunk_frames)
	assert torch.equal(whole, parts_result)
	return res, whole


def main(out_dir):
	import convasr_amd as ca
	d = torch.device('cuda:0')
	res = dict(device = torch.cuda.get_device_name(0), states_per_block = ca.ops.ctc_alignment_long_tiles()[0], default_chunk_frames = ca.ops.ctc_alignment_long_tiles()[1])
	# (a)
	gen = torch.Generator().manual_seed(8)
	B, T, S = 1, 60000, 8000
	tg = torch.randint(0, C - 1, (B, S), generator = gen)
	tl, il = torch.full((B, ), S), torch.full((B, ), T)
	lp = torch.randn(T, B, C, generator = gen).log_softmax(-1).to(d)
	a = dict(labels = S, frames = T, alignment = gpu_ms(lambda: ca.ctc.alignment(lp, tg, il, tl, blank = C - 1), runs = 5))
	a['alignment_long'], whole = long_form(lp, tg, il, tl, 0)
	a['equal'] = bool(torch.equal(whole, ca.ctc.alignment(lp, tg, il, tl, blank = C - 1)))
	a['alignment_over_alignment_long'] = a['alignment']['median_ms'] / a['alignment_long']['call']['median_ms']
	print(json.dumps(a), flush = True)
	res['a_8000_labels_60000_frames'] = a
	del lp
	# (b), (c)
	T, S, Tb = 180000, 48000, 179500
	lp_np, tg_np, pos = R.planted(7, T, S, C, C - 1, 12.0, input_length = Tb)
	lp, tg, il, tl = torch.from_numpy(lp_np).unsqueeze(1).to(d), torch.from_numpy(tg_np).unsqueeze(0), torch.tensor([Tb]), torch.tensor([S])
	hour = dict(labels = S, frames = T, input_length = Tb, by_chunk_frames = {})
	for chunk_frames in (0, 64, 128, 512, 1024):
		r, whole = long_form(lp, tg, il, tl, chunk_frames)
		r['equals_planted'] = bool(torch.equal(whole.cpu()[0], torch.from_numpy(pos)))
		print(json.dumps(r), flush = True)
		hour['by_chunk_frames'][str(r['chunk_frames'])] = r
	res['b_c_one_hour'] = hour
	os.makedirs(out_dir, exist_ok = True)
	json.dump(res, open(os.path.join(out_dir, 'r08_alignment_long.json'), 'w'), indent = 1)


if __name__ == '__main__':
	ap = argparse.ArgumentParser()
	ap.add_argument('--out', default = os.path.join(ROOT, 'profiles'))
	args = ap.parse_args()
	assert torch.cuda.is_available(), 'this script measures on the GPU'
	main(args.out)
