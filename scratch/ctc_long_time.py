"""Timing of ops.ctc_loss_long on the GPU (README row, profiles/r11_ctc_loss_long.json).

    python scratch/ctc_long_time.py --out DIR

Loss and gradient of random log-probs (x 2 before the log-softmax) against random targets, every utterance at full length, C = 38:
(a) 1 x 30,000 frames x 9,000 labels (ten minutes), at the default chunk length and at 64, 128 and 512;
(b) 8 x 13,000 x 600;
(c) 2 x 2,100 x 1,024, and torch's fp32 F.ctc_loss (forward and backward, the oracle's call) on this host's CPU for the same batch;
(d) 64 x 753 x 150 on both routes: what the tiled kernel costs where the one-workgroup kernel applies.
Medians of 7 runs after 2 warm-up runs, device events around the calls (workspace allocation included).  Single-device measurements."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def case(B, T, S, chunks = (0, ), short_too = False, cpu_fp32 = False):
	from convasr_amd import ops, _lib
	from oracle import convasr_oracle as O
	d = torch.device('cuda:0')
	gen = torch.Generator().manual_seed(S)
	lp = (torch.randn(B, T, C, generator = gen) * 2).log_softmax(-1)
	y = torch.randint(0, C - 1, (B, S), generator = gen)
	olen, ylen = torch.full((B, ), T), torch.full((B, ), S)
	lpd, yd, od, yl = lp.to(d).permute(0, 2, 1), y.to(d), olen.to(d), ylen.to(d)
	assert ops.is_cl(lpd)
	sb, default = ops.ctc_loss_long_tiles()
	res = dict(B = B, frames = T, labels = S, workspace_bytes = _lib.load().convasr_ctc_loss_long_workspace_bytes(B, T, C, S), short_kernel_takes_it = bool(_lib.load().convasr_ctc_loss_supported(B, T, C, S)), by_chunk_frames = {})
	for chunk_frames in chunks:
		chunk = chunk_frames or default
		r = gpu_ms(lambda: ops.ctc_loss_long(lpd, yd, od, yl, C - 1, chunk_frames = chunk_frames))
		r['forward_only'] = gpu_ms(lambda: ops.ctc_loss_long(lpd, yd, od, yl, C - 1, need_grad = False, chunk_frames = chunk_frames))
		r['launches_per_sweep'] = -(-T // chunk) + -(-(2 * S + 1) // sb) - 1  # one launch runs an anti-diagonal of the alpha sweep and one of the beta sweep
		nll, _ = ops.ctc_loss_long(lpd, yd, od, yl, C - 1, chunk_frames = chunk_frames)
		r['all_finite'] = bool(torch.isfinite(nll).all())
		res['by_chunk_frames'][str(chunk)] = r
	if short_too:
		res['short_kernel'] = gpu_ms(lambda: ops.ctc_loss(lpd, yd, od, yl, C - 1))
		res['long_over_short'] = res['by_chunk_frames'][str(default)]['median_ms'] / res['short_kernel']['median_ms']
	if cpu_fp32:
		times = []
		for _ in range(3):
			x = lp.permute(0, 2, 1).clone().requires_grad_(True)
			t0 = time.perf_counter()
			O.ctc_loss(x, y, olen, ylen).sum().backward()
			times.append((time.perf_counter() - t0) * 1e3)
		res['torch_fp32_cpu_forward_backward_ms'] = dict(median_ms = statistics.median(times), runs = 3, threads = torch.get_num_threads())
	print(json.dumps(res), flush = True)
	return res


def main(out_dir):
	from convasr_amd import ops
	res = dict(device = torch.cuda.get_device_name(0), note = 'single-device measurements', states_per_block = ops.ctc_loss_long_tiles()[0], default_chunk_frames = ops.ctc_loss_long_tiles()[1])
	res['a_ten_minutes'] = case(1, 30000, 9000, chunks = (0, 64, 128, 512))
	res['b_8x13000x600'] = case(8, 13000, 600)
	res['c_2x2100x1024'] = case(2, 2100, 1024, cpu_fp32 = True)
	res['d_64x753x150'] = case(64, 753, 150, short_too = True)
	os.makedirs(out_dir, exist_ok = True)
	json.dump(res, open(os.path.join(out_dir, 'r11_ctc_loss_long.json'), 'w'), indent = 1)


if __name__ == '__main__':
	ap = argparse.ArgumentParser()
	ap.add_argument('--out', default = os.path.join(ROOT, 'profiles'))
	args = ap.parse_args()
	assert torch.cuda.is_available(), 'this script measures on the GPU'
	main(args.out)
