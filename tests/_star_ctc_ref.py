"""Float64 numpy restatement of the star-token CTC lattice (include/convasr_hip.h: convasr_star_ctc_loss has the rule), vectorised over
the states of an utterance.  Shared by tests/test_star_ctc_ref.py (which pins it against a subset sum through F.ctc_loss) and
tests/test_star_ctc_gpu.py (which pins the kernel against it)."""
import numpy as np

STAR = -1


def units_of(labels, mask):
	"""labels (S,), mask (S + 1,) bool -> (classes of the units with STAR for a star, gap of every unit or -1 for a label)."""
	cls, gap = [], []
	for g in range(len(labels) + 1):
		if mask[g]:
			cls.append(STAR)
			gap.append(g)
		if g < len(labels):
			cls.append(int(labels[g]))
			gap.append(-1)
	return np.array(cls, dtype = np.int64), np.array(gap, dtype = np.int64)


def _lse(stack):
	m = stack.max(axis = 0)
	ms = np.where(np.isfinite(m), m, 0.0)
	with np.errstate(divide = 'ignore'):
		return ms + np.log(np.exp(stack - ms).sum(axis = 0))


def _shift(v, d):
	"""out[s] = v[s - d] (d > 0) or v[s + |d|] (d < 0), -inf where that state does not exist"""
	if d == 0:
		return v
	out = np.full_like(v, -np.inf)
	if d > 0:
		out[d:] = v[:-d] if d < len(v) else []
	elif d < 0:
		out[:d] = v[-d:] if -d < len(v) else []
	return out


def lattice(lp_tc, labels, mask, blank, penalty, enter):
	"""One utterance: lp_tc (T, C) float64 with T >= 1.  Returns (nll, post (T, C), star (S + 1,)): the posterior mass of the label and
	blank states of every class at every frame, and the expected frames every gap's star absorbs."""
	T, C = lp_tc.shape
	S = len(labels)
	ucls, ugap = units_of(labels, mask)
	n = len(ucls)
	L = 2 * n + 1
	cls = np.full(L, blank, dtype = np.int64)
	cls[1::2] = ucls
	is_star = cls == STAR
	unit = np.arange(L) % 2 == 1
	NEG = -np.inf
	# cost of the arc from s - d into s (-inf: no such arc)
	c = np.full((5, L), NEG)
	c[0] = 0.0
	c[1, 1:] = np.where(is_star[1:], enter, 0.0)
	for s in range(1, L, 2):
		if s >= 2 and cls[s] != cls[s - 2]:
			c[2, s] = enter if is_star[s] else 0.0
		if s >= 3 and is_star[s - 2]:
			c[3, s] = 0.0
			if s >= 4 and cls[s - 4] != cls[s]:
				c[4, s] = 0.0
	em = np.where(is_star[None, :], penalty, lp_tc[:, np.where(is_star, 0, cls)])  # (T, L)
	start = np.full(L, NEG)
	start[0] = 0.0
	if L > 1:
		start[1] = enter if is_star[1] else 0.0
	if L > 3 and is_star[1]:
		start[3] = 0.0
	end = np.full(L, NEG)
	end[L - 1] = 0.0
	if L >= 2:
		end[L - 2] = 0.0
	if n >= 1 and is_star[L - 2]:
		end[L - 3] = 0.0
		if L >= 4:
			end[L - 4] = 0.0
	alpha = np.empty((T, L))
	beta = np.empty((T, L))
	with np.errstate(invalid = 'ignore'):
		alpha[0] = start + em[0]
		for t in range(1, T):
			a = alpha[t - 1]
			alpha[t] = _lse(np.stack([_shift(a, d) + c[d] for d in range(5)])) + em[t]
		beta[T - 1] = end + em[T - 1]
		for t in range(T - 2, -1, -1):
			b = beta[t + 1]
			beta[t] = _lse(np.stack([_shift(b + c[d], -d) for d in range(5)])) + em[t]
		total = _lse((alpha[T - 1] + end)[:, None])[0]
		post_s = np.where(np.isfinite(alpha) & np.isfinite(beta) & np.isfinite(total), np.exp(alpha + beta - em - total), 0.0)  # (T, L)
	post = np.zeros((T, C))
	star = np.zeros(S + 1)
	if np.isfinite(total):
		for s in range(L):
			if is_star[s]:
				star[ugap[s >> 1]] += post_s[:, s].sum()
			else:
				post[:, cls[s]] += post_s[:, s]
	return -total, post, star


def star_ctc_ref(log_probs, targets, olen, ylen, blank, star_mask, penalty, enter):
	"""log_probs (B, C, T), targets (B, S_max), star_mask (B, S_max + 1): array-likes.  Returns float64 (nll (B,), grad (B, C, T) with
	grad = occ * exp(lp) - post for t < olen and 0 beyond (all 0 for an infeasible utterance), star_frames (B, S_max + 1))."""
	lp = np.asarray(log_probs, dtype = np.float64)
	targets, olen, ylen, star_mask = np.asarray(targets), np.asarray(olen), np.asarray(ylen), np.asarray(star_mask).astype(bool)
	B, C, T = lp.shape
	targets = targets.reshape(B, -1)
	S_max = targets.shape[1]
	nll = np.empty(B)
	grad = np.zeros((B, C, T))
	frames = np.zeros((B, S_max + 1))
	for b in range(B):
		Tb, S = int(olen[b]), int(ylen[b])
		if Tb == 0:
			nll[b] = 0.0 if S == 0 else np.inf
			continue
		rows = lp[b, :, :Tb].T
		nll[b], post, star = lattice(rows, targets[b, :S], star_mask[b, :S + 1], blank, penalty, enter)
		if np.isfinite(nll[b]):
			with np.errstate(invalid = 'ignore'):
				grad[b, :, :Tb] = (post.sum(axis = 1, keepdims = True) * np.exp(rows) - post).T
			frames[b, :S + 1] = star
	return nll, grad, frames
