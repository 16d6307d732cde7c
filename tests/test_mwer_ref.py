"""The N-best MWER rule without a GPU: the float64 restatement (tests/_mwer_ref.py, what the kernels are held to in
tests/test_mwer_gpu.py) against three independent statements -- float64 F.ctc_loss for the hypotheses' likelihoods, a brute force over
every frame labelling for loss and posteriors, float64 autograd through a torch restatement of the formula for the gradient -- then the
parity inputs' condition (the hypothesis weights are not one-hot), MWER's refusals, and the wiring of the new entry points with their
envelope, which is checked before any launch."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _mwer_ref import mwer_ref, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('convasr_mwer_states_per_wave', 'convasr_mwer_renorm_frames', 'convasr_mwer_max_labels', 'convasr_mwer_max_hyps', 'convasr_mwer_supported', 'convasr_mwer_workspace_bytes', 'convasr_mwer_loss')
_DUMMY = (ctypes.c_char * 64)()


def near_base_batch(B, C, T, L, N, seed, lean = 3.0, olen = None, lengths = None):
	"""The parity inputs of tests/test_mwer_gpu.py: log-probs that lean mildly towards a base labelling (each label held for T // (L + 1)
	frames or so, `lean` added to its logit), hypotheses that are one- to three-edit variants of the base (substitute, delete, insert),
	risk = the number of edits plus a fraction, so non-integer.  -> (lp (B, C, T) fp32 tensor, hyps (B, N, L + 3), hyp_lengths, olen, risk)."""
	rng = np.random.default_rng(seed)
	blank = C - 1
	logits = rng.standard_normal((B, C, T))
	hyps = np.full((B, N, L + 3), C - 2, dtype = np.int64)
	lens = np.zeros((B, N), dtype = np.int64)
	risk = np.zeros((B, N), dtype = np.float32)
	olen = np.full(B, T, dtype = np.int64) if olen is None else np.asarray(olen, dtype = np.int64)
	for b in range(B):
		Lb = L if lengths is None else int(lengths[b])
		base = list(rng.integers(0, C - 1, Lb))
		for i in range(1, Lb):  # no repeats in the base: it fits in few frames
			while base[i] == base[i - 1]:
				base[i] = int(rng.integers(0, C - 1))
		Tb = int(olen[b])
		for i, c in enumerate(base):
			t0, t1 = Tb * (2 * i + 1) // (2 * Lb + 1), Tb * (2 * i + 2) // (2 * Lb + 1)
			logits[b, c, t0:max(t1, t0 + 1)] += lean
		for n in range(N):
			h, edits = list(base), 1 + n % 3
			for _ in range(edits if n else 0):
				kind, pos = int(rng.integers(0, 3)), int(rng.integers(0, max(len(h), 1)))
				if kind == 0 and h:
					h[pos] = int((h[pos] + 1 + rng.integers(0, C - 2)) % (C - 1))
				elif kind == 1 and len(h) > 1:
					del h[pos]
				else:
					h.insert(pos, int(rng.integers(0, C - 1)))
			lens[b, n] = len(h)
			hyps[b, n, :len(h)] = h
			risk[b, n] = (edits if n else 0) + 0.25 * (n % 2) - 0.5 * (n % 5 == 4)
	lp = torch.from_numpy(logits).float().log_softmax(dim = 1)
	return lp, torch.from_numpy(hyps), torch.from_numpy(lens), torch.from_numpy(olen), torch.from_numpy(risk)


def informative(ref, min_p = 0.05):
	"""the condition the parity cases must meet, on the restatement's own values: at least half of the utterances have two hypotheses with
	p >= 0.05, and max |grad| >= 1e-2"""
	loss, grad, nll, post, w = ref
	two = (post >= min_p).sum(axis = 1) >= 2
	return two.sum() * 2 >= len(two) and np.abs(grad).max() >= 1e-2


def small_cases(n = 24, seed = 5, C = 3, N = 3):
	rng = np.random.default_rng(seed)
	out = []
	for i in range(n):
		T = int(rng.integers(1, 7))
		lp = torch.from_numpy(rng.standard_normal((1, C, T)) * 1.5).log_softmax(dim = 1).numpy()
		lens = rng.integers(-1 if i % 5 == 0 else 0, 4, (1, N))
		hyps = rng.integers(0, C - 1, (1, N, 3))
		risk = rng.standard_normal((1, N)) * 2
		out.append((lp, hyps, lens, np.array([T]), risk, (0.1, 1.0, 3.0)[i % 3]))
	return out


def test_hyp_nll_against_float64_ctc_loss():
	worst = 0.0
	for lp, hyps, lens, olen, risk, scale in small_cases(40, seed = 6, C = 4, N = 4):
		_, _, nll, _, _ = mwer_ref(lp, hyps, lens, olen, risk, lp.shape[1] - 1, scale)
		for n in range(lens.shape[1]):
			L = int(lens[0, n])
			if L < 0:
				assert nll[0, n] == np.inf
				continue
			want = F.ctc_loss(torch.from_numpy(lp[0].T.copy()).unsqueeze(1), torch.from_numpy(hyps[0, n, :L].copy()).reshape(1, L), torch.tensor([int(olen[0])]), torch.tensor([L]), blank = lp.shape[1] - 1, reduction = 'none')
			want = float(want[0])
			assert np.isfinite(want) == np.isfinite(nll[0, n]), (want, nll[0, n])
			if np.isfinite(want):
				worst = max(worst, abs(want - nll[0, n]))
	assert worst <= 1e-12, worst


def collapse(path, blank):
	out, prev = [], None
	for c in path:
		if c != prev and c != blank:
			out.append(c)
		prev = c
	return tuple(out)


def test_loss_and_posteriors_against_a_brute_force_over_every_labelling():
	"""T <= 6, C = 3, N = 3: P(h) = the sum of prod_t exp(lp[c_t, t]) over the C^T labellings that collapse to h"""
	C, blank = 3, 2
	seen_two = 0
	for lp, hyps, lens, olen, risk, scale in small_cases(24, seed = 5):
		T, N = int(olen[0]), lens.shape[1]
		prob = {}
		for path in itertools.product(range(C), repeat = T):
			k = collapse(path, blank)
			prob[k] = prob.get(k, 0.0) + float(np.exp(sum(lp[0, c, t] for t, c in enumerate(path))))
		P = np.array([prob.get(tuple(int(v) for v in hyps[0, n, :lens[0, n]]), 0.0) if lens[0, n] >= 0 else 0.0 for n in range(N)])
		part = P > 0
		loss, grad, nll, post, w = mwer_ref(lp, hyps, lens, olen, risk, blank, scale)
		assert np.array_equal(np.isfinite(nll[0]), part)
		assert np.allclose(np.exp(-nll[0][part]), P[part], rtol = 1e-12, atol = 0)
		if part.sum() == 0:
			assert loss[0] == 0 and not post.any() and not grad.any()
			continue
		q = P ** scale
		q = q / q.sum()
		want = float((q * np.where(part, risk[0], 0)).sum() - risk[0][part].mean()) if part.sum() >= 2 else 0.0
		assert np.allclose(post[0], q, rtol = 1e-11, atol = 1e-14) and abs(loss[0] - want) <= 1e-11, (post, q, loss, want)
		if part.sum() < 2:
			assert loss[0] == 0.0 and not grad.any()
		seen_two += part.sum() >= 2
	assert seen_two >= 12


def torch_restatement(lp, hyps, lens, olen, risk, blank, scale):
	"""the same formula as torch float64 ops over F.ctc_loss, for autograd: lp (C, T) requires grad -> loss (0-d)"""
	T = int(olen)
	lls, rs = [], []
	for n in range(len(lens)):
		L = int(lens[n])
		if L < 0:
			continue
		nll = F.ctc_loss(lp[:, :T].t().unsqueeze(1), torch.as_tensor(hyps[n, :L]).reshape(1, L), torch.tensor([T]), torch.tensor([L]), blank = blank, reduction = 'none')[0]
		if bool(torch.isfinite(nll.detach())):
			lls.append(-nll)
			rs.append(float(risk[n]))
	if len(lls) < 2:
		return None
	p = torch.softmax(scale * torch.stack(lls), dim = 0)
	r = torch.tensor(rs, dtype = torch.float64)
	return (p * r).sum() - r.mean()


def test_gradient_against_float64_autograd():
	"""ATen's ctc_loss backward is exp(lp) - posterior per hypothesis; the weights sum to 0, so the exp(lp) terms cancel and autograd's
	tensor is the rule's sum of w posterior -- the identity the header states"""
	checked = 0
	for lp, hyps, lens, olen, risk, scale in small_cases(30, seed = 7, C = 4, N = 4) + [tuple(t.numpy() if hasattr(t, 'numpy') else t for t in near_base_batch(1, 5, 14, 4, 5, seed = 2)) + (1.0, )]:
		x = torch.from_numpy(np.asarray(lp[0], dtype = np.float64)).requires_grad_(True)
		loss = torch_restatement(x, hyps[0], lens[0], olen[0], risk[0], lp.shape[1] - 1, scale)
		got = mwer_ref(lp, hyps, lens, olen, risk, lp.shape[1] - 1, scale)
		if loss is None:
			assert got[0][0] == 0.0 and not got[1].any()
			continue
		loss.backward()
		assert abs(float(loss.detach()) - got[0][0]) <= 1e-11
		assert np.abs(x.grad.numpy() - got[1][0]).max() <= 1e-11, np.abs(x.grad.numpy() - got[1][0]).max()
		assert np.abs(got[1][0].sum(axis = 0)).max() <= 1e-12  # the class sum of every frame is 0
		checked += 1
	assert checked >= 15


def test_weights_edge_cases():
	inf = np.inf
	assert weights(np.array([-inf, -inf]), np.array([1.0, 2.0]), 1.0)[:1] == (0.0, )
	loss, p, w, E, rbar = weights(np.array([-inf, -3.0, -inf]), np.array([1.0, 2.0, 5.0]), 2.0)
	assert loss == 0.0 and p.tolist() == [0.0, 1.0, 0.0] and not w.any() and E == 2.0
	loss, p, w, E, rbar = weights(np.array([-3.0, -3.0, -inf]), np.array([0.0, 3.0, 100.0]), 0.5)
	assert p.tolist() == [0.5, 0.5, 0.0] and E == 1.5 and rbar == 1.5 and loss == 0.0 and w.tolist() == [-0.375, 0.375, 0.0]
	assert abs(w.sum()) <= 1e-15


def test_parity_inputs_are_informative():
	"""the shapes tests/test_mwer_gpu.py builds with near_base_batch, at its seeds: the weights must not be one-hot"""
	from test_mwer_gpu import PARITY, SCALE, most_labels
	for name, kw in PARITY.items():
		batch = near_base_batch(**kw)
		if name == 'the most labels':
			most_labels(batch)
		ref = mwer_ref(*[t.numpy() for t in batch], kw['C'] - 1, SCALE.get(name, 1.0))
		assert np.isfinite(ref[2]).all(), name
		assert informative(ref), (name, ref[3])


def test_mwer_option_refusals():
	from convasr_amd import ctc, models
	ok = ctc.MWER(4, 16, weight = 0.5, ctc_weight = 1, unit = 'words', space = 36)
	assert (ok.n_best, ok.beam_width, ok.weight, ok.ctc_weight, ok.unit, ok.space, ok.scale, ok.include_reference, ok.head) == (4, 16, 0.5, 1.0, 'words', 36, 1.0, False, 0)
	assert ctc.MWER(2, 2, 1.0, 0.0, unit = 'chars').space is None
	with pytest.raises(TypeError):
		ctc.MWER(4, 16)  # no defaults: nothing has been tuned
	with pytest.raises(TypeError):
		ctc.MWER(4, 16, weight = 1.0)
	for kw in (dict(unit = 'words'), dict(unit = 'bpe'), dict(n_best = 1), dict(n_best = 65), dict(beam_width = 3), dict(weight = -1.0), dict(ctc_weight = float('nan')), dict(weight = None), dict(scale = 0.0), dict(scale = float('inf'))):
		with pytest.raises(ValueError):
			ctc.MWER(**dict(dict(n_best = 4, beam_width = 16, weight = 1.0, ctc_weight = 1.0, unit = 'chars'), **kw))
	assert 'self.ctc_mwer = None' in open(os.path.join(ROOT, 'convasr_amd', 'models.py')).read() and hasattr(models.JasperNet, 'forward')


def test_wiring_and_the_envelope_checked_before_any_launch():
	from convasr_amd import _lib, functional, ops
	header = open(os.path.join(ROOT, 'include', 'convasr_hip.h')).read()
	lib = _lib.load()
	for name in NEW:
		assert re.search(r'\b' + name + r'\s*\(', header), name
		assert name in _lib._SIGNATURES and hasattr(lib, name), name
	assert callable(ops.mwer_loss) and callable(functional.mwer_loss) and issubclass(functional.MwerLossFunction, torch.autograd.Function)
	per_wave, renorm, max_labels, max_hyps = ops.mwer_tiles()
	assert (per_wave, renorm, max_labels, max_hyps) == (lib.convasr_mwer_states_per_wave(), lib.convasr_mwer_renorm_frames(), lib.convasr_mwer_max_labels(), lib.convasr_mwer_max_hyps())
	assert per_wave >= 2 and per_wave % 2 == 0 and renorm >= 1 and max_labels >= 511 and max_hyps == 64
	assert ops.MWER_WORKSPACE_CAP == 8 << 30
	einval, eunsupported = -1, -3
	for shape in ((1, 1, 1, 2, 0), (64, 8, 753, 38, 150), (2, 64, 4096, 512, max_labels)):
		assert lib.convasr_mwer_supported(*shape) == 1, shape
		assert lib.convasr_mwer_workspace_bytes(*shape) > 0, shape
	ls = 2 * 150 + 2
	assert lib.convasr_mwer_workspace_bytes(64, 8, 753, 38, 150) == (2 * 512 * 753 * ls + 512 * (753 // renorm + 1) * ls + 5 * 512) * 4  # the formula the header states
	# no GPU is touched: every refusal precedes the first HIP call
	one = ctypes.cast(_DUMMY, ctypes.c_void_p)
	def call(B = 1, N = 3, T = 8, C = 38, L = 3, blank = 37, scale = 1.0, lp = one, hyps = one, risk = one, loss = one, ws = one):
		return lib.convasr_mwer_loss(lp, hyps, one, one, risk, scale, loss, one, one, one, ws, B, N, T, C, L, blank, None)
	for kw in (dict(L = max_labels + 1), dict(N = max_hyps + 1), dict(T = 1 << 20), dict(C = 8193), dict(B = 1 << 16)):
		shape = dict(dict(B = 1, N = 3, T = 8, C = 38, L = 3), **kw)
		assert lib.convasr_mwer_supported(*[shape[k] for k in 'BNTCL']) == 0, kw
		assert lib.convasr_mwer_workspace_bytes(*[shape[k] for k in 'BNTCL']) == eunsupported, kw
		assert call(**kw, **({'blank': 0} if 'C' in kw else {})) == eunsupported, kw
		assert b'mwer' in lib.convasr_last_error() and b'envelope' in lib.convasr_last_error()
	for kw in (dict(B = 0), dict(N = 0), dict(T = 0), dict(C = 1, blank = 0), dict(L = -1), dict(blank = 38), dict(blank = -1), dict(scale = 0.0), dict(scale = -1.0), dict(scale = float('nan')), dict(scale = float('inf')),
	           dict(lp = None), dict(hyps = None), dict(risk = None), dict(loss = None), dict(ws = None)):
		assert call(**kw) == einval, kw
		assert b'mwer_loss' in lib.convasr_last_error()
