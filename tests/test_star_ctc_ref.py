"""The star-token CTC rule without a GPU: the float64 restatement of the lattice (tests/_star_ctc_ref.py, what the kernel is held to in
tests/test_star_ctc_gpu.py) against an independent statement of the same likelihood,

  exp(-nll) = sum over the subsets A of the allowed gaps of exp(|A| star_enter) * P_ctc(labels with a star class at the gaps in A),

taken through float64 F.ctc_loss over log-probs that carry one more column per gap holding star_penalty; then ctc.star_gaps, StarCTC's
refusals, the wiring of the new entry points and their envelope, which is checked before any launch."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _star_ctc_ref import star_ctc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('convasr_star_ctc_states_per_wave', 'convasr_star_ctc_renorm_frames', 'convasr_star_ctc_max_states', 'convasr_star_ctc_supported', 'convasr_star_ctc_workspace_bytes', 'convasr_star_ctc_loss')
_DUMMY = (ctypes.c_char * 64)()
C, BLANK = 4, 3  # a 3-letter alphabet, so labels repeat
PENALTIES = [(0.0, 0.0), (-0.3, -0.7), (-1.1, 0.0), (0.0, -0.5)]


def cases(n = 72, seed = 11):
	"""(logits (C, T), labels (S,), mask (S + 1,), penalty, enter): T 1-12, S 0-5, at most 6 allowed gaps, every pair of PENALTIES in turn"""
	rng = np.random.default_rng(seed)
	out = []
	for i in range(n):
		T, S = int(rng.integers(1, 13)), int(rng.integers(0, 6))
		labels = rng.integers(0, C - 1, S)
		mask = rng.random(S + 1) < (0.0, 0.35, 0.7, 1.0)[i % 4]
		out.append((rng.standard_normal((C, T)) * 2, labels, mask, *PENALTIES[(i // 4) % len(PENALTIES)]))
	return out


def subset_sum(logits, labels, mask, penalty, enter):
	"""(nll, d nll / d logits (C, T), star frames per gap (S + 1,)) of the subset sum, all subsets in one batched float64 F.ctc_loss; the
	star of gap g is class C + g, whose column is a leaf: d (-nll) / d column, summed over the frames, is that star's expected frame count"""
	S, T = len(labels), logits.shape[1]
	lg = torch.tensor(logits, dtype = torch.float64, requires_grad = True)
	cols = torch.full((S + 1, T), float(penalty), dtype = torch.float64, requires_grad = True)
	raw = torch.cat([lg.log_softmax(dim = 0), cols], dim = 0)  # (C + S + 1, T)
	# ATen's backward is exp(lp) - posterior: the derivative with respect to LOGITS behind a log_softmax, not with respect to log-probs that
	# do not sum to one.  So the extended rows are normalised for F.ctc_loss and the normaliser, which every path pays once per frame, is
	# given back: P(raw) = P(raw - Z) exp(sum_t Z_t).  Autograd through both terms is then the true derivative with respect to the columns.
	Z = torch.logsumexp(raw, dim = 0)
	ext = raw - Z
	gaps = [g for g in range(S + 1) if mask[g]]
	subsets = [A for k in range(len(gaps) + 1) for A in itertools.combinations(gaps, k)]
	tg = torch.zeros(len(subsets), 2 * S + 1, dtype = torch.int64)
	tl = torch.zeros(len(subsets), dtype = torch.int64)
	for i, A in enumerate(subsets):
		seq = [u for g in range(S + 1) for u in ([C + g] if g in A else []) + ([int(labels[g])] if g < S else [])]
		tg[i, :len(seq)] = torch.tensor(seq, dtype = torch.int64)
		tl[i] = len(seq)
	lp = ext.t().unsqueeze(1).expand(T, len(subsets), C + S + 1)
	olen = torch.full((len(subsets), ), T, dtype = torch.int64)
	fin = torch.isfinite(F.ctc_loss(lp.detach(), tg, olen, tl, blank = BLANK, reduction = 'none', zero_infinity = False))
	loss = F.ctc_loss(lp, tg, olen, tl, blank = BLANK, reduction = 'none', zero_infinity = True)  # (an infinite loss left out below would still put NaN into the gradient)
	if not bool(fin.any()):
		return float('inf'), np.zeros_like(logits), np.zeros(S + 1)
	sizes = torch.tensor([float(len(A)) for A in subsets], dtype = torch.float64)
	nll = -torch.logsumexp((sizes * enter - loss)[fin], dim = 0) - Z.sum()
	nll.backward()
	return float(nll.detach()), lg.grad.numpy(), -cols.grad.sum(dim = 1).numpy()


def restated(logits, labels, mask, penalty, enter):
	"""the restatement on one utterance: (nll, d nll / d logits through log_softmax's backward, star_frames)"""
	lp = torch.tensor(logits, dtype = torch.float64).log_softmax(dim = 0).numpy()
	S = len(labels)
	nll, grad, frames = star_ctc_ref(lp[None], np.asarray(labels, dtype = np.int64).reshape(1, S), [logits.shape[1]], [S], BLANK, np.asarray(mask)[None], penalty, enter)
	g = grad[0]
	return float(nll[0]), g - np.exp(lp) * g.sum(axis = 0, keepdims = True), frames[0]


def test_restatement_is_the_subset_sum_through_ctc_loss():
	infeasible, worst = 0, [0.0, 0.0, 0.0]
	all_cases = cases()
	for logits, labels, mask, penalty, enter in all_cases:
		assert int(mask.sum()) <= 6
		want = subset_sum(logits, labels, mask, penalty, enter)
		got = restated(logits, labels, mask, penalty, enter)
		if not np.isfinite(want[0]):
			infeasible += 1
			assert got[0] == float('inf') and not got[1].any() and not got[2].any()
			continue
		errs = [abs(got[0] - want[0]), float(np.abs(got[1] - want[1]).max()), float(np.abs(got[2] - want[2]).max())]
		worst = [max(a, b) for a, b in zip(worst, errs)]
		assert errs[0] <= 1e-10 and errs[1] <= 1e-10 and errs[2] <= 1e-10, (labels, mask, penalty, enter, errs)
	print(f'star ctc restatement vs subset sum: {len(all_cases)} cases, {infeasible} infeasible, worst |d nll| {worst[0]:.2e}, |d grad| {worst[1]:.2e}, |d star_frames| {worst[2]:.2e}')
	assert infeasible == N_INFEASIBLE and infeasible < len(all_cases) / 4


N_INFEASIBLE = 8  # of cases(): what the generator above draws (T < the frames the labels need)


def test_restatement_with_an_all_false_mask_is_ctc_loss():
	rng = np.random.default_rng(5)
	B, T, S = 6, 14, 5
	logits = torch.tensor(rng.standard_normal((B, C, T)), dtype = torch.float64, requires_grad = True)
	y = torch.tensor(rng.integers(0, C - 1, (B, S)))
	olen, ylen = torch.tensor([14, 9, 3, 14, 1, 7]), torch.tensor([5, 4, 5, 0, 1, 3])  # row 2: infeasible
	lp = logits.log_softmax(dim = 1)
	loss = F.ctc_loss(lp.permute(2, 0, 1), y, olen, ylen, blank = BLANK, reduction = 'none')
	fin = torch.isfinite(loss.detach())
	assert fin.tolist() == [True, True, False, True, True, True]
	loss[fin].sum().backward()
	nll, grad, frames = star_ctc_ref(lp.detach().numpy(), y.numpy(), olen.numpy(), ylen.numpy(), BLANK, np.zeros((B, S + 1), dtype = bool), -0.3, -0.7)
	assert np.array_equal(np.isfinite(nll), fin.numpy()) and not frames.any() and not grad[2].any()
	assert np.abs(nll[fin.numpy()] - loss.detach().numpy()[fin.numpy()]).max() <= 1e-10
	p = np.exp(lp.detach().numpy())
	assert np.abs((grad - p * grad.sum(axis = 1, keepdims = True)) - logits.grad.numpy())[fin.numpy()].max() <= 1e-10  # (the infeasible row: zeros here, above)
	# the convention itself: occ = 1 without a star, so grad = exp(lp) - posterior and its class sum is 0 inside olen
	assert np.abs(grad.sum(axis = 1)).max() <= 1e-12


def test_star_frames_of_one_star_column_is_the_derivative_with_respect_to_it():
	"""one column shared by every star: d (-nll) / d column summed over the frames = the frames all stars absorb = star_frames.sum()"""
	for logits, labels, mask, penalty, enter in cases(24, seed = 3):
		S, T = len(labels), logits.shape[1]
		lg = torch.tensor(logits, dtype = torch.float64)
		col = torch.full((1, T), float(penalty), dtype = torch.float64, requires_grad = True)
		raw = torch.cat([lg.log_softmax(dim = 0), col], dim = 0)
		Z = torch.logsumexp(raw, dim = 0)  # (see subset_sum: normalised rows for F.ctc_loss, the normaliser given back)
		ext = raw - Z
		gaps = [g for g in range(S + 1) if mask[g]]
		terms = []
		for k in range(len(gaps) + 1):
			for A in itertools.combinations(gaps, k):
				seq = [u for g in range(S + 1) for u in ([C] if g in A else []) + ([int(labels[g])] if g < S else [])]
				loss = F.ctc_loss(ext.t().unsqueeze(1), torch.tensor([seq], dtype = torch.int64).reshape(1, len(seq)), torch.tensor([T]), torch.tensor([len(seq)]), blank = BLANK, reduction = 'none')
				if bool(torch.isfinite(loss.detach()).all()):
					terms.append(k * enter - loss[0])
		got = restated(logits, labels, mask, penalty, enter)
		if not terms:
			assert got[0] == float('inf')
			continue
		ll = torch.logsumexp(torch.stack(terms), dim = 0) + Z.sum()
		ll.backward()
		assert abs(got[0] + float(ll.detach())) <= 1e-10 and abs(got[2].sum() - float(col.grad.sum())) <= 1e-10, (labels, mask)
		assert not got[2][~np.asarray(mask)].any()


def test_star_gaps_modes_on_cpu_tensors():
	from convasr_amd import ctc
	sp = 2
	y = torch.tensor([[0, sp, 1, sp, sp, 0], [sp, 1, 0, sp, 7, 7], [5, 5, 5, 5, 5, 5], [1, sp, 1, 1, 1, sp]])
	ylen = torch.tensor([6, 4, 0, 1])  # ragged: the labels past ylen (a space among them in rows 1 and 3) must not count
	def rows(m):
		return [[int(v) for v in r] for r in m]
	ends = ctc.star_gaps(y, ylen, 'ends')
	assert ends.dtype == torch.bool and ends.shape == (4, 7)
	assert rows(ends) == [[1, 0, 0, 0, 0, 0, 1], [1, 0, 0, 0, 1, 0, 0], [1, 0, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0]]
	assert rows(ctc.star_gaps(y, ylen, 'words', space = sp)) == [[1, 1, 0, 1, 1, 0, 1], [1, 0, 0, 1, 1, 0, 0], [1, 0, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0]]
	assert rows(ctc.star_gaps(y, ylen, 'all')) == [[1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 0, 0], [1, 0, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0]]
	empty = ctc.star_gaps(torch.zeros(2, 0, dtype = torch.int64), torch.tensor([0, 0]), 'words', space = sp)
	assert rows(empty) == [[1], [1]]
	assert rows(ctc.star_gaps(torch.tensor([[sp], [1], [sp]]), torch.tensor([1, 1, 0]), 'words', space = sp)) == [[1, 1], [1, 1], [1, 0]]  # a space as the first label: gap 0 once
	for bad in (dict(mode = 'some'), dict(mode = 'words')):
		with pytest.raises(ValueError):
			ctc.star_gaps(y, ylen, bad['mode'])
	with pytest.raises(ValueError):
		ctc.star_gaps(y, ylen[:3], 'all')


def test_star_ctc_option_refusals():
	from convasr_amd import ctc
	ok = ctc.StarCTC('words', penalty = -0.5, enter = -1, space = 2)
	assert (ok.gaps, ok.penalty, ok.enter, ok.space) == ('words', -0.5, -1.0, 2)
	assert torch.equal(ok.mask(torch.tensor([[0, 2, 1]]), torch.tensor([3])), torch.tensor([[True, True, False, True]]))
	assert ctc.StarCTC('all', penalty = 0.0, enter = 0.0).space is None
	with pytest.raises(TypeError):
		ctc.StarCTC('all')  # no defaults: nothing has been tuned
	with pytest.raises(TypeError):
		ctc.StarCTC('all', penalty = -1.0)
	for kw in (dict(gaps = 'words', penalty = -1.0, enter = -1.0), dict(gaps = 'every', penalty = -1.0, enter = -1.0), dict(gaps = 'all', penalty = 0.1, enter = -1.0), dict(gaps = 'all', penalty = -1.0, enter = 1e-9),
	           dict(gaps = 'all', penalty = float('nan'), enter = -1.0), dict(gaps = 'all', penalty = float('-inf'), enter = -1.0), dict(gaps = 'all', penalty = None, enter = -1.0), dict(gaps = 'all', penalty = -1.0, enter = '0')):
		with pytest.raises(ValueError):
			ctc.StarCTC(**kw)
	from convasr_amd import models
	assert 'self.ctc_star = None' in open(os.path.join(ROOT, 'convasr_amd', 'models.py')).read() and hasattr(models.JasperNet, 'forward')


def test_wiring_and_the_envelope_checked_before_any_launch():
	from convasr_amd import _lib, functional, ops
	header = open(os.path.join(ROOT, 'include', 'convasr_hip.h')).read()
	lib = _lib.load()
	for name in NEW:
		assert re.search(r'\b' + name + r'\s*\(', header), name
		assert name in _lib._SIGNATURES and hasattr(lib, name), name
	assert callable(ops.star_ctc_loss) and callable(functional.star_ctc_loss) and issubclass(functional.StarCtcLossFunction, torch.autograd.Function)
	per_wave, renorm, max_states = lib.convasr_star_ctc_states_per_wave(), lib.convasr_star_ctc_renorm_frames(), lib.convasr_star_ctc_max_states()
	assert per_wave >= 2 and per_wave % 2 == 0 and renorm >= 1 and max_states >= 1023
	assert ops.star_ctc_tiles() == (per_wave, renorm, max_states)
	s_top = (max_states - 3) // 4  # every gap starred: 4 S + 3 states
	assert s_top >= 255
	einval, eunsupported = -1, -3
	# the envelope the issue names is inside: 1,023 states, T = 4,096 at C = 512
	for shape in ((1, 1, 2, 0), (64, 753, 38, 150), (2, 4096, 512, 255), (1, 4096, 512, s_top)):
		assert lib.convasr_star_ctc_supported(*shape) == 1, shape
		assert lib.convasr_star_ctc_workspace_bytes(*shape) > 0, shape
	# no GPU is touched: every refusal precedes the first HIP call
	one = ctypes.cast(_DUMMY, ctypes.c_void_p)
	def call(B = 1, T = 8, C = 38, S = 3, blank = 37, penalty = -0.5, enter = -1.0, lp = one, mask = one, frames = one, ws = one):
		return lib.convasr_star_ctc_loss(lp, one, one, one, mask, penalty, enter, one, one, frames, ws, B, T, C, S, blank, None)
	for kw in (dict(S = s_top + 1), dict(S = 1023), dict(T = 1 << 20), dict(C = 8193), dict(B = 1 << 16)):
		shape = dict(dict(B = 1, T = 8, C = 38, S = 3), **kw)
		assert lib.convasr_star_ctc_supported(shape['B'], shape['T'], shape['C'], shape['S']) == 0, kw
		assert lib.convasr_star_ctc_workspace_bytes(shape['B'], shape['T'], shape['C'], shape['S']) == eunsupported, kw
		assert call(**{k: v for k, v in kw.items()}, **({'blank': 0} if 'C' in kw else {})) == eunsupported, kw
		assert b'star_ctc' in lib.convasr_last_error() and b'envelope' in lib.convasr_last_error()
	for kw in (dict(B = 0), dict(T = 0), dict(C = 1, blank = 0), dict(S = -1), dict(blank = 38), dict(blank = -1), dict(penalty = 0.1), dict(enter = 0.1), dict(penalty = float('nan')), dict(enter = float('nan')),
	           dict(lp = None), dict(mask = None), dict(frames = None), dict(ws = None)):
		assert call(**kw) == einval, kw
		assert b'star_ctc_loss' in lib.convasr_last_error()
	for bad in ((0, 8, 38, 3), (1, 0, 38, 3), (1, 8, 1, 3), (1, 8, 38, -1)):
		assert lib.convasr_star_ctc_supported(*bad) == 0, bad
