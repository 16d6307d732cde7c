"""A float64 numpy restatement of convasr_frame_uncertainty and convasr_span_uncertainty, written from the rule in include/convasr_hip.h.
tests/test_uncertainty_ref.py holds it against the reference's own numbers (tests/golden/uncertainty.npz), a per-span Python loop and the
greedy rule's restatement; tests/test_uncertainty_gpu.py holds the kernels against it."""
import types

import numpy as np

EINVAL = -1
MAX_CLASSES = 8192


def _order_key(row):
	"""Sort key of the argmax's total order: NaN above every number, ties to the lower index -> the indices from best to worst."""
	nan = np.isnan(row)
	return sorted(range(len(row)), key = lambda c: (0 if nan[c] else 1, 0.0 if nan[c] else -row[c], c))


def frame_envelope(B, T, C, eps_id):
	"""The library's answer to a call of these sizes: 0 inside the envelope, EINVAL outside."""
	return 0 if B >= 1 and T >= 1 and B * T < 2 ** 31 and 2 <= C <= MAX_CLASSES and 0 <= eps_id < C else EINVAL


def frame_uncertainty(lp, eps_id = -1, lengths = None):
	"""lp: (B, T, C) float32 log-probs.  Returns a namespace of (B, T) arrays: idx int64, and float64 p1, p2, margin, entropy, entropy_nb, p_eps."""
	lp = np.asarray(lp)
	B, T, C = lp.shape
	eps_id = eps_id % C
	assert frame_envelope(B, T, C, eps_id) == 0
	x = lp.astype(np.float64)
	nan = np.isnan(x)
	has_nan = nan.any(-1)
	with np.errstate(all = 'ignore'):
		# the total order: NaN above every number (the first NaN of a frame wins), ties to the lower index (argmax returns the first maximum)
		idx = np.where(has_nan, nan.argmax(-1), np.where(nan, -np.inf, x).argmax(-1)).astype(np.int64)
		best = np.take_along_axis(x, idx[..., None], -1)[..., 0]
		rest = x.copy()
		np.put_along_axis(rest, idx[..., None], -np.inf, -1)
		p1, p2 = np.exp(best), np.exp(rest.max(-1))  # (a frame with a NaN is overwritten below)
		others = np.delete(x, eps_id, axis = -1)
		d = others - others.max(-1, keepdims = True)
		lq = d - np.log(np.exp(d).sum(-1, keepdims = True))  # log_softmax over the classes other than eps_id; one class: exactly 0
		vals = dict(p1 = p1, p2 = p2, margin = p1 - p2, entropy = -(np.exp(x) * x).sum(-1), entropy_nb = -(np.exp(lq) * lq).sum(-1) + 0.0, p_eps = np.exp(x[..., eps_id]))
	n = np.full(B, T) if lengths is None else np.clip(np.asarray(lengths, dtype = np.int64), 0, T)
	live = np.arange(T)[None, :] < n[:, None]
	for k, v in vals.items():
		vals[k] = np.where(live, np.where(has_nan, np.nan, v), 0.0)
	return types.SimpleNamespace(idx = idx, **vals)


def frame_uncertainty_loop(lp, eps_id = -1, lengths = None):
	"""frame_uncertainty frame by frame and class by class, as the header words it (small inputs): what the vectorised form is checked against."""
	lp = np.asarray(lp)
	B, T, C = lp.shape
	eps_id = eps_id % C
	x = lp.astype(np.float64)
	out = types.SimpleNamespace(idx = np.zeros((B, T), np.int64), **{k: np.zeros((B, T)) for k in ('p1', 'p2', 'margin', 'entropy', 'entropy_nb', 'p_eps')})
	others = [c for c in range(C) if c != eps_id]
	with np.errstate(all = 'ignore'):
		for b in range(B):
			n = T if lengths is None else min(max(int(lengths[b]), 0), T)
			for t in range(T):
				row = x[b, t]
				order = _order_key(row)
				out.idx[b, t] = order[0]
				if t >= n:
					continue
				if np.isnan(row).any():
					for k in ('p1', 'p2', 'margin', 'entropy', 'entropy_nb', 'p_eps'):
						getattr(out, k)[b, t] = np.nan
					continue
				out.p1[b, t], out.p2[b, t] = np.exp(row[order[0]]), np.exp(row[order[1]])
				out.margin[b, t] = out.p1[b, t] - out.p2[b, t]
				out.entropy[b, t] = -sum(np.exp(v) * v for v in row)
				out.p_eps[b, t] = np.exp(row[eps_id])
				m = max(row[c] for c in others)
				S = sum(np.exp(row[c] - m) for c in others)
				out.entropy_nb[b, t] = -sum(np.exp(row[c] - m - np.log(S)) * (row[c] - m - np.log(S)) for c in others) + 0.0
	return out


def span_envelope(N, B, T, C, eps = 1e-9, Tp = None, frame_map = False, events = True, path = False):
	Tp = T if Tp is None else Tp
	ok = 1 <= N < 2 ** 31 and B >= 1 and T >= 1 and Tp >= 1 and B * T < 2 ** 31 and B * Tp < 2 ** 31 and (frame_map or Tp == T) and 2 <= C <= MAX_CLASSES and eps >= 0 and (events or not path)
	return 0 if ok else EINVAL


def span_uncertainty(lp, stats, utt, begin, end, first = None, tokens = None, frames = None, path = None, eps = 1e-9, frame_map = None):
	"""lp: (B, T, C) float32; stats: arrays idx, p1, margin, entropy, p_eps of shape (B, T) (the device's fp32 ones, or frame_uncertainty's).
	Returns a namespace of (N,) arrays: n_events, confidence, confidence_min, margin, entropy, uncertainty (float64)."""
	lp = np.asarray(lp)
	B, T, C = lp.shape
	N = len(utt)
	Tp = T if frame_map is None else np.asarray(frame_map).shape[1]
	assert span_envelope(N, B, T, C, eps, Tp, frame_map is not None, tokens is not None, path is not None) == 0
	H, PE, M, P1 = (np.asarray(getattr(stats, k), dtype = np.float64) for k in ('entropy', 'p_eps', 'margin', 'p1'))
	idx = np.asarray(stats.idx)
	eps = float(np.float32(eps))
	clamp = lambda v, lo, hi: min(max(int(v), lo), hi)
	out = types.SimpleNamespace(n_events = np.zeros(N, np.int32), **{k: np.zeros(N) for k in ('confidence', 'confidence_min', 'margin', 'entropy', 'uncertainty')})
	n_total = 0 if tokens is None else len(tokens)
	with np.errstate(all = 'ignore'):
		for k in range(N):
			u = clamp(utt[k], 0, B - 1)
			b0 = clamp(begin[k], 0, Tp - 1)
			e0 = clamp(end[k], b0, Tp - 1)
			fb, fe = b0, e0
			if frame_map is not None:
				fb = clamp(frame_map[u][b0], 0, T - 1)
				fe = clamp(frame_map[u][e0], fb, T - 1)
			h, w = H[u, fb:fe + 1], 1.0 - PE[u, fb:fe + 1]
			out.entropy[k] = h.sum() / (fe - fb + 1)
			out.uncertainty[k] = (h * w).sum() / (eps + w.sum())
			if tokens is None:
				continue
			lo = clamp(first[k], 0, n_total)
			hi = clamp(first[k + 1], lo, n_total)
			ls, ms = [], []
			for j in range(lo, hi):
				tk, fr = int(tokens[j]), int(frames[j])
				if j > lo and int(tokens[j - 1]) == tk and int(frames[j - 1]) == fr:
					continue
				c, p = clamp(tk, 0, C - 1), clamp(fr, 0, Tp - 1)
				if path is not None and int(path[u][p]) != tk:
					continue
				f = p if frame_map is None else clamp(frame_map[u][p], 0, T - 1)
				l = float(lp[u, f, c])
				ls.append(l)
				ms.append(M[u, f] if int(idx[u, f]) == c else np.exp(l) - P1[u, f])
			out.n_events[k] = len(ls)
			if ls:
				out.confidence[k] = np.exp(np.sum(ls) / len(ls))
				out.confidence_min[k] = np.exp(np.min(ls))
				out.margin[k] = np.min(ms)
	return out


def greedy_spans(paths, lengths, eps, space, bats, split_words = True):
	"""The spans and events GreedyCTCGenerator.generate hands to ops.span_uncertainty, from the greedy rule's restatement
	(tests/_greedy_ref.py): a namespace of lists utt, begin, end, first (N + 1 entries), tokens, frames."""
	import _greedy_ref
	tokens, frames, counts, first, begin, end = _greedy_ref.greedy_segments_batch(paths, lengths, eps, space, bats, split_words)
	utt = [b for b, n in enumerate(counts[1]) for _ in range(n)]
	return types.SimpleNamespace(utt = utt, begin = begin, end = end, first = first + [len(tokens)], tokens = tokens, frames = frames)


def span_mean_abs_l(lp, utt, first, tokens, frames, path = None, frame_map = None):
	"""mean |l_j| over the events of every span that count (the confidence bar scales with it); 0 where none counts."""
	lp = np.asarray(lp)
	out = np.zeros(len(utt))
	for k in range(len(utt)):
		ls = []
		for j in range(int(first[k]), int(first[k + 1])):
			tk, fr = int(tokens[j]), int(frames[j])
			if (j > first[k] and int(tokens[j - 1]) == tk and int(frames[j - 1]) == fr) or (path is not None and int(path[utt[k]][fr]) != tk):
				continue
			ls.append(abs(float(lp[utt[k], fr if frame_map is None else int(frame_map[utt[k]][fr]), tk])))
		out[k] = np.mean(ls) if ls else 0.0
	return out


def log_softmax32(logits):
	"""float32 log-probs of float64 logits along the last axis."""
	logits = np.asarray(logits, dtype = np.float64)
	d = logits - logits.max(-1, keepdims = True)
	return (d - np.log(np.exp(d).sum(-1, keepdims = True))).astype(np.float32)


def special_frames(rng, C):
	"""(3, 12, C) log-probs with exact ties (first, last, three-way), one NaN frame, two NaNs, a class at -inf, the blank at -inf."""
	x = log_softmax32(rng.standard_normal((3, 12, C)) * 3)
	x[0, 1, 0] = x[0, 1, C - 1] = x[0, 1].max() + 0.5
	x[0, 2, :] = np.float32(-np.log(C))
	x[0, 3, C - 1] = np.nan
	x[0, 4, 0] = x[0, 4, C - 1] = np.nan
	x[1, 0, C // 2] = -np.inf
	x[1, 1, C - 1] = -np.inf
	x[1, 2, 0] = np.nan
	x[1, 2, 1] = np.inf
	return x
