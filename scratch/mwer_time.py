"""Timing of the N-best MWER loss on the GPU (README row, DESIGN, profiles/r22_mwer.json).
  * convasr_mwer_loss (three launches, with the gradient) at 64 x 753 frames, 38 classes, 150-label hypotheses, N = 4 and 8, against the
    COMPOSED form on the same tensors: the log-probs repeated N times, convasr_ctc_loss with gradient on B N rows, the weights and the
    weighted sum of the N gradients as torch ops.  DEVICE EVENTS around the calls, output buffers and workspaces allocated outside (the
    composed form's repeat and its ATen temporaries are part of what it costs), alternating in one process; the bytes both take;
  * ctc.MWER.hypotheses (beam search + edit distance) on its own on the same log-probs, at several beam widths;
  * one eager Wav2Letter bf16 training step (SGD, dropout 0.2) on the benchmark batch with and without model.ctc_mwer: DEVICE EVENTS
    around train_step, alternating.  The model is untrained, so its hypotheses are short: the step shows the decode's cost, not that of
    150-label lattices (the first table has those).
Medians of 7 after 2 warm-ups, with min and max.  Usage: python scratch/mwer_time.py --out DIR"""
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
SPACE, SCALE = 36, 0.1


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


def inputs(B, T, C, L, N, d):
	"""log-probs that lean towards a base labelling; hypothesis n = the base with n substitutions, risk n"""
	g = torch.Generator().manual_seed(0)
	base = torch.randint(0, C - 2, (B, L), generator = g)
	logits = torch.randn(B, C, T, generator = g)
	frame = (torch.arange(T) * L // T).clamp(max = L - 1)
	logits.scatter_add_(1, base[:, frame].unsqueeze(1), torch.full((B, 1, T), 2.0))
	hyps = base.unsqueeze(1).repeat(1, N, 1)
	for n in range(1, N):
		pos = torch.randint(0, L, (B, n), generator = g)
		hyps[:, n].scatter_(1, pos, (hyps[:, n].gather(1, pos) + 1) % (C - 2))
	risk = torch.arange(N, dtype = torch.float32).repeat(B, 1)
	return ops.as_cl(logits.log_softmax(dim = 1).to(d)), hyps.to(d), torch.full((B, N), L, dtype = torch.int64, device = d), torch.full((B, ), T, dtype = torch.int64, device = d), risk.to(d)


def kernels(B, T, C, L, N, d):
	lp, hyps, lens, olen, risk = inputs(B, T, C, L, N, d)
	P, St = ops.ptr, ops.stream_ptr
	loss, nll, post, grad = torch.empty(B, device = d), torch.empty(B, N, device = d), torch.empty(B, N, device = d), ops.empty_cl(B, C, T, torch.float32, d)
	ws = torch.empty(ops._query('convasr_mwer_workspace_bytes', B, N, T, C, L), dtype = torch.uint8, device = d)
	ws_ctc = torch.empty(ops._cached_query('convasr_ctc_workspace_bytes', B * N, T, L), dtype = torch.uint8, device = d)
	nll_rows, grad_rows = torch.empty(B * N, device = d), torch.empty(B * N, T, C, device = d)
	hyps_rows, lens_rows, olen_rows = hyps.reshape(B * N, L).contiguous(), lens.reshape(B * N).contiguous(), olen.repeat_interleave(N).contiguous()
	lp_btc = lp.permute(0, 2, 1)  # the memory layout, (B, T, C)
	assert lp_btc.is_contiguous()
	composed_out = {}

	def fused():
		ops.call('convasr_mwer_loss', P(lp), P(hyps), P(lens), P(olen), P(risk), SCALE, P(loss), P(grad), P(nll), P(post), P(ws), B, N, T, C, L, C - 1, St())

	def composed():
		rows = lp_btc.repeat_interleave(N, dim = 0)  # N copies of the log-probs
		ops.call('convasr_ctc_loss', P(rows), P(hyps_rows), P(olen_rows), P(lens_rows), P(nll_rows), P(grad_rows), P(ws_ctc), B * N, T, C, L, C - 1, St())
		p = torch.softmax(-SCALE * nll_rows.view(B, N), dim = 1)
		E = (p * risk).sum(dim = 1)
		w = SCALE * p * (risk - E.unsqueeze(1))
		composed_out['loss'] = E - risk.mean(dim = 1)
		composed_out['grad'] = -(w.view(B, N, 1, 1) * grad_rows.view(B, N, T, C)).sum(dim = 1)  # (convasr_ctc_loss's gradient is exp(lp) - posterior; the weights sum to 0)

	t = events(dict(fused = fused, composed = composed))
	med = {k: statistics.median(v) for k, v in t.items()}
	diff = dict(loss = float((composed_out['loss'] - loss).abs().max()), grad = float((composed_out['grad'] - grad.permute(0, 2, 1)).abs().max()), grad_max = float(grad.abs().max()))
	composed_bytes = dict(workspace = ws_ctc.numel(), log_prob_copies = B * N * T * C * 4, gradients = B * N * T * C * 4)
	return dict(B = B, T = T, classes = C, labels = L, N = N, scale = SCALE, device_events = {k: stats(v) for k, v in t.items()}, fused_over_composed = med['fused'] / med['composed'],
	            bytes = dict(fused_workspace = ws.numel(), composed = composed_bytes, composed_total = sum(composed_bytes.values())), fused_minus_composed = diff)


def decode(B, T, C, L, d):
	lp, hyps, _, olen, _ = inputs(B, T, C, L, 2, d)
	y, ylen = hyps[:, 0].contiguous(), torch.full((B, ), L, dtype = torch.int64, device = d)
	y[:, 5::6] = SPACE
	fns = {}
	for n_best, width in ((4, 8), (4, 32), (8, 32), (8, 128), (8, 512)):
		m = ctc.MWER(n_best, width, weight = 1.0, ctc_weight = 1.0, unit = 'words', space = SPACE)
		fns[f'n_best {n_best}, beam_width {width}'] = lambda m = m: m.hypotheses(lp, olen, y, ylen)
	return dict(B = B, T = T, classes = C, labels = L, unit = 'words', device_events = {k: stats(v) for k, v in events(fns).items()})


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
	options = {'plain': None, 'mwer n_best 4, beam_width 16': ctc.MWER(4, 16, weight = 0.1, ctc_weight = 1.0, unit = 'words', space = SPACE, include_reference = True),
	           'mwer n_best 8, beam_width 128': ctc.MWER(8, 128, weight = 0.1, ctc_weight = 1.0, unit = 'words', space = SPACE, include_reference = True)}
	it = [0]
	seen = {}

	def run(name):
		model.ctc_mwer = options[name]
		res = ca.train.train_step(model, opt, x, xlen, y, ylen, iteration = it[0])
		seen[name] = res
		it[0] += 1
	t = events({k: (lambda k = k: run(k)) for k in options})
	med = {k: statistics.median(v) for k, v in t.items()}
	risk = {k: float(v['mwer_expected_risk'].mean()) for k, v in seen.items() if 'mwer_expected_risk' in v}
	return dict(model = 'Wav2Letter', dtype = 'bfloat16', batch = 64, seconds = 15, note = 'untrained model: its hypotheses are short; with include_reference the reference (150 labels) is one of the lattices',
	            device_events = {k: stats(v) for k, v in t.items()}, over_plain = {k: med[k] / med['plain'] for k in med if k != 'plain'}, added_ms = {k: med[k] - med['plain'] for k in med if k != 'plain'},
	            last_expected_risk = risk)


if __name__ == '__main__':
	ap = argparse.ArgumentParser()
	ap.add_argument('--out', required = True)
	args = ap.parse_args()
	d = torch.device('cuda:0')
	res = dict(device = torch.cuda.get_device_name(0),
	           note = "the runtime names the MI355X 'AMD Radeon Graphics'; device_events: torch.cuda.Event pairs around the calls, alternating in one process; medians of 7 after 2 warm-ups",
	           warmup = WARMUP, kernels = [kernels(64, 753, 38, 150, N, d) for N in (4, 8)], hypotheses = decode(64, 753, 38, 150, d), step = step(d))
	os.makedirs(args.out, exist_ok = True)
	with open(os.path.join(args.out, 'r22_mwer.json'), 'w') as f:
		json.dump(res, f, indent = 1)
	print(json.dumps(res))
