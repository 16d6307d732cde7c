"""Timing of the distillation kernels on the GPU (README row, DESIGN 7k, profiles/r19_distill.json).
  * ops.topk_frames (k = 8, fp16 values, uint8 / int16 indices) against ops.argmax on the same tensor -- the floor of one read of it;
  * ops.distill_kl with the gradient against ops.log_softmax + ops.log_softmax_bwd -- one read and one write of the same array each, so
    twice what distill_kl moves;
  both at 64 x 753 frames x 38 classes (the 64 x 15 s batch) and at 512 classes: DEVICE EVENTS around the C entry points, output buffers
  allocated outside, alternating in one process.
  * one eager Wav2Letter bf16 training step (SGD, dropout 0.2) on the benchmark batch, with and without a stored teacher (k = 8, fp16 /
    uint8, made once by another Wav2Letter; weight 0.5, temperature 2): DEVICE EVENTS around train_step, alternating.
Medians of 7 after 2 warm-ups, with min and max.  Usage: python scratch/distill_time.py --out DIR"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import convasr_amd as ca  # noqa: E402
from convasr_amd import _lib, ops  # noqa: E402

WARMUP, RUNS = 2, 7
K = 8


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


def kernels(B, T, C, d):
	g = torch.Generator().manual_seed(C)
	z = (torch.randn(B, T, C, generator = g) * 3).to(d).permute(0, 2, 1)
	teacher = (torch.randn(B, T, C, generator = g) * 3).to(d).permute(0, 2, 1)
	idt = torch.uint8 if C <= 256 else torch.int16
	values, indices = (t.permute(0, 2, 1) for t in ops.topk_frames(teacher, K, torch.float16, idt))  # (B, T, k) memory
	olen = torch.full((B, ), T, dtype = torch.int64, device = d)
	idx = torch.empty(B, T, dtype = torch.int64, device = d)
	v_out, i_out = torch.empty_like(values), torch.empty_like(indices)
	kd, frames = torch.empty(B, dtype = torch.float32, device = d), torch.empty(B, T, dtype = torch.float32, device = d)
	grad, lp, dlp = (ops.empty_cl(B, C, T, torch.float32, d) for _ in range(3))
	P, S, icode = ops.ptr, ops.stream_ptr, ops.INDEX_CODES[idt]
	fns = dict(
		topk_frames = lambda: ops.call('convasr_topk_frames', P(z), P(v_out), _lib.F16, P(i_out), icode, B, T, C, K, S()),
		argmax = lambda: ops.call('convasr_argmax', P(z), P(idx), B * T, C, S()),
		distill_kl = lambda: ops.call('convasr_distill_kl', P(z), P(values), _lib.F16, P(indices), icode, P(olen), P(kd), P(frames), P(grad), B, T, C, K, 2.0, S()),
		distill_kl_no_grad = lambda: ops.call('convasr_distill_kl', P(z), P(values), _lib.F16, P(indices), icode, P(olen), P(kd), P(frames), None, B, T, C, K, 2.0, S()),
	)

	def softmax_pair():
		ops.call('convasr_log_softmax_fwd', P(z), P(lp), B * T, C, S())
		ops.call('convasr_log_softmax_bwd', P(grad), P(lp), P(dlp), B * T, C, S())
	fns['log_softmax_fwd_bwd'] = softmax_pair
	t = events(fns)
	med = {k: statistics.median(v) for k, v in t.items()}
	rows = B * T
	moved = dict(topk_frames = rows * (4 * C + K * (2 + indices.element_size())), argmax = rows * (4 * C + 8), distill_kl = rows * (8 * C + K * (2 + indices.element_size()) + 4),
	             log_softmax_fwd_bwd = rows * 4 * C * 5)
	return dict(B = B, T = T, classes = C, k = K, values = 'float16', indices = str(idt).replace('torch.', ''), device_events = {k: stats(v) for k, v in t.items()}, bytes_read_plus_written = moved,
	            topk_frames_over_argmax = med['topk_frames'] / med['argmax'], distill_kl_over_log_softmax_fwd_bwd = med['distill_kl'] / med['log_softmax_fwd_bwd'])


def step(d):
	torch.manual_seed(0)
	fe = lambda: ca.models.LogFilterBankFrontend(64, 16000, 0.02, 0.01, 'hann_window')
	model = ca.models.Wav2Letter(64, [38], frontend = fe(), dropout = 0.2, check_time_dim_padded = False, compute_dtype = torch.bfloat16).to(d).train()
	big = ca.models.Wav2Letter(64, [38], frontend = fe(), dropout = 0.2, check_time_dim_padded = False, compute_dtype = torch.bfloat16).to(d)
	flat = ca.train.FlatParameters(model)
	opt = ca.train.SGD(flat, lr = 1e-4, momentum = 0.9, weight_decay = 1e-3)
	g = torch.Generator().manual_seed(1)
	x = (torch.rand(64, 16000 * 15, generator = g) * 2 - 1).to(d)
	xlen = torch.ones(64, device = d)
	y = torch.randint(0, 37, (64, 1, 150), generator = g).to(d)
	ylen = torch.full((64, 1), 150, dtype = torch.long, device = d)
	teacher, _ = ca.distill.teacher_from_model(big, x, xlen, K)  # made once: a stored teacher, nothing of it inside the timed step
	it = [0]

	def run(**kw):
		ca.train.train_step(model, opt, x, xlen, y, ylen, iteration = it[0], **kw)
		it[0] += 1
	t = events(dict(plain = run, with_teacher = lambda: run(teacher = teacher, distill_weight = 0.5, distill_temperature = 2.0)))
	med = {k: statistics.median(v) for k, v in t.items()}
	return dict(model = 'Wav2Letter', dtype = 'bfloat16', batch = 64, seconds = 15, k = K, device_events = {k: stats(v) for k, v in t.items()}, with_teacher_over_plain = med['with_teacher'] / med['plain'],
	            added_ms = med['with_teacher'] - med['plain'])


if __name__ == '__main__':
	ap = argparse.ArgumentParser()
	ap.add_argument('--out', required = True)
	args = ap.parse_args()
	d = torch.device('cuda:0')
	res = dict(device = torch.cuda.get_device_name(0),
	           note = "the runtime names the MI355X 'AMD Radeon Graphics'; device_events: torch.cuda.Event pairs around the C entry points (kernels) or around train_step (step), alternating in one process; medians of 7 after 2 warm-ups",
	           warmup = WARMUP, kernels = [kernels(64, 753, 38, d), kernels(64, 753, 512, d)], step = step(d))
	os.makedirs(args.out, exist_ok = True)
	with open(os.path.join(args.out, 'r19_distill.json'), 'w') as f:
		json.dump(res, f, indent = 1)
	print(json.dumps(res))
