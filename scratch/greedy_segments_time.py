"""Timing of GreedyCTCGenerator.generate with time stamps on the GPU (README row, profiles/r10_greedy_segments.json): the device route
(ops.argmax -> ops.ctc_greedy_segments -> gathered stamps) against the host loop generate_host on the same CUDA tensors, in one process,
alternating.  Shapes: 64 x 753 frames (the 64 x 15 s batch) and 1 x 180,000 frames (an hour), 38 classes; speech-like paths of runs of
3 frames, 60 % blanks, 3 % spaces, seeded.  End to end = wall clock between two device synchronisations (host work included); the five
launches of convasr_ctc_greedy_segments alone by device events.  Medians of 7 after 2 warm-ups, with min and max.
Usage: python scratch/greedy_segments_time.py --out DIR"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convasr_amd import ops  # noqa: E402
from convasr_amd.transcribe import RU_ALPHABET  # noqa: E402
from convasr_amd.transcript_generators import CharTokenizerLegacy, GreedyCTCGenerator  # noqa: E402

WARMUP, RUNS = 2, 7


def speech_like(B, T, tok, seed):
	rng = random.Random(seed)
	rows = []
	for _ in range(B):
		row = []
		while len(row) < T:
			r = rng.random()
			row += [tok.eps_id if r < 0.6 else tok.space_id if r < 0.63 else rng.randrange(len(tok.alphabet))] * 3
		rows.append(row[:T])
	return torch.tensor(rows)


def stats(ms):
	return dict(median_ms = statistics.median(ms), min_ms = min(ms), max_ms = max(ms), runs = len(ms))


def wall(fn):
	torch.cuda.synchronize()
	t0 = time.perf_counter()
	out = fn()
	torch.cuda.synchronize()
	return (time.perf_counter() - t0) * 1e3, out


def measure(B, T, tok, d):
	path = speech_like(B, T, tok, B + T)
	lp = torch.nn.functional.one_hot(path, tok.vocab_size).permute(0, 2, 1).float().to(d)
	olen = torch.full((B, ), T, dtype = torch.int64, device = d)
	begin, end = torch.zeros(B, device = d), torch.full((B, ), T * 0.02, device = d)
	ts = (T * 0.02) * torch.linspace(0, 1, steps = T, device = d).unsqueeze(0).expand(B, -1)
	gen = GreedyCTCGenerator()
	routes = dict(device = lambda: gen.generate(tok, lp, begin, end, olen, ts), host = lambda: gen.generate_host(tok, lp, begin, end, olen, ts),
	              device_ops_only = lambda: ops.ctc_greedy_segments(ops.argmax(lp), olen, tok.eps_id, tok.space_id, gen.blank_amount_to_space))
	times = {k: [] for k in routes}
	results = {}
	for rep in range(WARMUP + RUNS):
		for k, fn in routes.items():  # alternating, so that drift of the machine hits all alike
			ms, results[k] = wall(fn)
			if rep >= WARMUP:
				times[k].append(ms)
	assert results['device'] == results['host']
	tokens, frames, counts, seg_first, seg_begin, seg_end = results['device_ops_only']
	n_tok, n_seg = int(tokens.numel()), int(seg_first.numel())

	# the five launches alone: device events around the C entry, buffers allocated outside
	idx = ops.argmax(lp)
	lib_bytes = ops._lib.load().convasr_ctc_greedy_segments_workspace_bytes(B, T)
	bufs = [torch.empty(2 * B * T, dtype = torch.int64, device = d), torch.empty(2 * B * T, dtype = torch.int32, device = d), torch.empty(2, B, dtype = torch.int64, device = d),
	        torch.empty(B * T, dtype = torch.int64, device = d), torch.empty(B * T, dtype = torch.int32, device = d), torch.empty(B * T, dtype = torch.int32, device = d),
	        torch.empty(lib_bytes, dtype = torch.uint8, device = d)]
	kernel_ms, argmax_ms = [], []
	for rep in range(WARMUP + RUNS):
		e = [torch.cuda.Event(enable_timing = True) for _ in range(4)]
		e[0].record()
		ops.call('convasr_ctc_greedy_segments', ops.ptr(idx), ops.ptr(olen), *[ops.ptr(b) for b in bufs], lib_bytes, B, T, tok.eps_id, tok.space_id, 10, 1, ops.stream_ptr())
		e[1].record()
		e[2].record()
		ops.argmax(lp)
		e[3].record()
		torch.cuda.synchronize()
		if rep >= WARMUP:
			kernel_ms.append(e[0].elapsed_time(e[1]))
			argmax_ms.append(e[2].elapsed_time(e[3]))
	d2h_device = 16 + 8 * B + 8 * n_tok + 8 * n_seg + 2 * 4 * n_seg + 2 * 4 * B  # count sums, segment counts, tokens, first-token offsets, begin / end stamps, begin / end
	d2h_host = 8 * B * T + 4 * B * T + 8 * B + 2 * 4 * B  # the path, the time stamps, the lengths, begin / end
	return dict(B = B, T = T, classes = tok.vocab_size, tokens = n_tok, segments = n_seg, chunk_frames = ops.ctc_greedy_segments_chunk(),
	            workspace_bytes = lib_bytes, generate_device_route = stats(times['device']), generate_host_route = stats(times['host']),
	            argmax_and_segments_with_read_back = stats(times['device_ops_only']), segments_five_launches_device_events = stats(kernel_ms),
	            argmax_device_events = stats(argmax_ms), device_to_host_bytes = dict(device_route = d2h_device, host_route = d2h_host),
	            speedup_of_medians = statistics.median(times['host']) / statistics.median(times['device']), results_equal = True)


if __name__ == '__main__':
	ap = argparse.ArgumentParser()
	ap.add_argument('--out', required = True)
	args = ap.parse_args()
	d = torch.device('cuda:0')
	tok = CharTokenizerLegacy(RU_ALPHABET)
	res = dict(device = torch.cuda.get_device_name(0), note = "the runtime names the MI355X 'AMD Radeon Graphics'; wall clock between two device synchronisations, alternating routes in one process",
	           warmup = WARMUP, shapes = [measure(64, 753, tok, d), measure(1, 180000, tok, d)])
	os.makedirs(args.out, exist_ok = True)
	with open(os.path.join(args.out, 'r10_greedy_segments.json'), 'w') as f:
		json.dump(res, f, indent = 1)
	print(json.dumps(res))
