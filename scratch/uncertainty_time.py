"""Timing of the uncertainty passes on the GPU (README row, profiles/r15_uncertainty.json).  Shapes: 64 x 753 frames (the 64 x 15 s batch)
and 1 x 180,000 frames (an hour), 38 classes; seeded log-probs that lean towards speech-like paths (runs of 3 frames, 60 % blanks, 3 % spaces).
  * ops.frame_uncertainty against ops.argmax alone (the pass it replaces on the decode route) and against ops.argmax + ops.entropy +
    ops.weighted_mean_entropy run one after the other (three reads of the same bytes): DEVICE EVENTS around the C entry points, output
    buffers allocated outside; bytes read plus written over the time as a share of the 8 TB/s HBM peak.
  * ops.span_uncertainty on the greedy segments of those inputs: DEVICE EVENTS likewise.
  * GreedyCTCGenerator.generate with time stamps, with and without uncertainty = True: WALL CLOCK between two device synchronisations, host
    work included, alternating in one process.
Medians of 7 after 2 warm-ups, with min and max.  Usage: python scratch/uncertainty_time.py --out DIR"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from convasr_amd import ops  # noqa: E402
from convasr_amd.transcribe import RU_ALPHABET  # noqa: E402
from convasr_amd.transcript_generators import UNCERTAINTY_KEYS, CharTokenizerLegacy, GreedyCTCGenerator  # noqa: E402
from greedy_segments_time import speech_like, stats, wall  # noqa: E402

WARMUP, RUNS = 2, 7
HBM_PEAK = 8e12  # bytes / s


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


def measure(B, T, tok, d):
	C = tok.vocab_size
	path = speech_like(B, T, tok, B + T)
	g = torch.Generator().manual_seed(B + T)
	logits = torch.randn(B, T, C, generator = g) * 2
	logits.scatter_add_(2, path.unsqueeze(-1), torch.full((B, T, 1), 5.0))
	lp = torch.log_softmax(logits, -1).to(d).permute(0, 2, 1)  # (B, C, T), channels-last
	olen = torch.full((B, ), T, dtype = torch.int64, device = d)
	begin, end = torch.zeros(B, device = d), torch.full((B, ), T * 0.02, device = d)
	ts = (T * 0.02) * torch.linspace(0, 1, steps = T, device = d).unsqueeze(0).expand(B, -1)
	gen = GreedyCTCGenerator()

	# the C entry points alone
	idx = torch.empty(B, T, dtype = torch.int64, device = d)
	f = torch.empty(5, B, T, dtype = torch.float32, device = d)
	per_utt = torch.empty(2, B, dtype = torch.float32, device = d)
	P, S = ops.ptr, ops.stream_ptr
	frame = lambda: ops.call('convasr_frame_uncertainty', P(lp), P(olen), P(idx), P(f[0]), P(f[1]), P(f[2]), P(f[3]), P(f[4]), B, T, C, tok.eps_id, S())
	frame_idx_only = lambda: ops.call('convasr_frame_uncertainty', P(lp), P(olen), P(idx), None, None, None, None, None, B, T, C, tok.eps_id, S())
	argmax = lambda: ops.call('convasr_argmax', P(lp), P(idx), B * T, C, S())
	entropy = lambda: ops.call('convasr_entropy', P(lp), P(olen), P(per_utt[0]), B, T, C, 1e-9, S())
	weighted = lambda: ops.call('convasr_weighted_mean_entropy', P(lp), P(olen), P(per_utt[1]), B, T, C, tok.eps_id, 1e-9, S())

	def three():
		argmax(); entropy(); weighted()
	kernel = events(dict(frame_uncertainty = frame, frame_uncertainty_idx_only = frame_idx_only, argmax = argmax, argmax_entropy_weighted_mean_entropy = three))
	assert torch.equal(ops.frame_uncertainty(lp, tok.eps_id, olen).idx, ops.argmax(lp))

	st = ops.frame_uncertainty(lp, tok.eps_id, olen)
	tokens, frames, counts, seg_first, seg_begin, seg_end = ops.ctc_greedy_segments(st.idx, olen, tok.eps_id, tok.space_id, gen.blank_amount_to_space)
	N, n_tok = int(seg_first.numel()), int(tokens.numel())
	utt = torch.repeat_interleave(counts[1], output_size = N)
	first = torch.cat([seg_first, torch.tensor([n_tok], device = d)])
	n_out = torch.empty(N, dtype = torch.int32, device = d)
	o = torch.empty(5, N, dtype = torch.float32, device = d)
	span = lambda: ops.call('convasr_span_uncertainty', P(lp), P(st.idx), P(st.p1), P(st.margin), P(st.entropy), P(st.p_eps), P(utt), P(seg_begin), P(seg_end), P(first), P(tokens),
	                        P(frames), n_tok, P(st.idx), None, T, P(n_out), P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), N, B, T, C, 1e-9, S())
	kernel.update(events(dict(span_uncertainty = span)))

	# the generator, end to end
	routes = dict(plain = lambda: gen.generate(tok, lp, begin, end, olen, ts), with_uncertainty = lambda: gen.generate(tok, lp, begin, end, olen, ts, uncertainty = True))
	times, results = {k: [] for k in routes}, {}
	for rep in range(WARMUP + RUNS):
		for k, fn in routes.items():
			ms, results[k] = wall(fn)
			if rep >= WARMUP:
				times[k].append(ms)
	assert [[{k: v for k, v in seg.items() if k not in UNCERTAINTY_KEYS} for seg in utt_[0]] for utt_ in results['with_uncertainty']] == [list(utt_[0]) for utt_ in results['plain']]

	rows = B * T
	moved = dict(frame_uncertainty = rows * (4 * C + 8 + 5 * 4), frame_uncertainty_idx_only = rows * (4 * C + 8), argmax = rows * (4 * C + 8),
	             argmax_entropy_weighted_mean_entropy = rows * (3 * 4 * C + 8) + 8 * B)
	out = dict(B = B, T = T, classes = C, segments = N, events = n_tok, device_events = {k: stats(v) for k, v in kernel.items()},
	           bytes_read_plus_written = moved,
	           share_of_hbm_peak = {k: moved[k] / (statistics.median(kernel[k]) * 1e-3) / HBM_PEAK for k in moved},
	           frame_uncertainty_over_argmax = statistics.median(kernel['frame_uncertainty']) / statistics.median(kernel['argmax']),
	           frame_uncertainty_over_three_passes = statistics.median(kernel['frame_uncertainty']) / statistics.median(kernel['argmax_entropy_weighted_mean_entropy']),
	           generate_wall_clock = {k: stats(v) for k, v in times.items()},
	           generate_with_over_without = statistics.median(times['with_uncertainty']) / statistics.median(times['plain']), text_and_stamps_equal = True)
	return out


if __name__ == '__main__':
	ap = argparse.ArgumentParser()
	ap.add_argument('--out', required = True)
	args = ap.parse_args()
	d = torch.device('cuda:0')
	tok = CharTokenizerLegacy(RU_ALPHABET)
	res = dict(device = torch.cuda.get_device_name(0),
	           note = "the runtime names the MI355X 'AMD Radeon Graphics'; device_events: torch.cuda.Event pairs around the C entry points, alternating; generate_wall_clock: between two device synchronisations, host work included, alternating in one process; medians of 7 after 2 warm-ups",
	           warmup = WARMUP, shapes = [measure(64, 753, tok, d), measure(1, 180000, tok, d)])
	os.makedirs(args.out, exist_ok = True)
	with open(os.path.join(args.out, 'r15_uncertainty.json'), 'w') as f:
		json.dump(res, f, indent = 1)
	print(json.dumps(res))
