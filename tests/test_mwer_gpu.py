"""The N-best MWER kernels (csrc/mwer.hip) against the float64 restatement of the rule (tests/_mwer_ref.py, itself pinned against
F.ctc_loss, a brute force and float64 autograd in tests/test_mwer_ref.py), and the option up to the model's surface.

The bars are the project's existing ones carried through the rule.  hyp_nll: rtol 1e-5 / atol 1e-4 on finite rows, infinite rows agree
exactly.  With eps_b = 1e-4 + 1e-5 max_n |nll| (the nll bar), R_b = max(1, max risk - min risk) over the hypotheses that take part and
grad_atol(T) = 2e-4 max(1, T / 1100)^1.5 (the short CTC kernel's bar): grad rtol 1e-4 / atol R_b (grad_atol(T) + 3 scale eps_b) -- the
posteriors' bar times sum |w| <= R_b, plus the nll bar carried through the softmax; loss rtol 1e-5 / atol 2 scale eps_b R_b;
hyp_posterior atol 2 scale eps_b.  Every check prints its worst share of each bar before it asserts (pytest -s shows them).

A random hypothesis list on random log-probs makes the weights one-hot and the gradient vanish, so the parity inputs lean towards a base
labelling and the hypotheses are one- to three-edit variants of it (test_mwer_ref.near_base_batch); every parity check asserts, on the
restatement's values, that at least half of the utterances have two hypotheses with p >= 0.05 and that max |grad| >= 1e-2."""
import numpy as np
import pytest
import torch

from _mwer_ref import mwer_ref
from test_mwer_ref import informative, near_base_batch

pytestmark = pytest.mark.gpu

# the parity shapes (near_base_batch's arguments) and the scale each runs at.  L is the base's length; a hypothesis has up to L + 3 labels.
# T <= 400 except the 753-frame workload row and the 511-label case, which cannot fit in fewer than 512 frames.
PARITY = {
	'N = 2, C = 5': dict(B = 3, C = 5, T = 30, L = 4, N = 2, seed = 22, lean = 0.3),
	'N = 5, C = 38, ragged': dict(B = 4, C = 38, T = 60, L = 8, N = 5, seed = 2, lean = 2.0, olen = [60, 41, 33, 60], lengths = [8, 5, 1, 8]),
	'N = 64': dict(B = 2, C = 38, T = 40, L = 5, N = 64, seed = 3, lean = 2.0),
	'one wave of states exactly': dict(B = 2, C = 38, T = 150, L = 60, N = 3, seed = 4, lean = 2.0),
	'either side of a wave': dict(B = 3, C = 38, T = 160, L = 65, N = 3, seed = 5, lean = 2.0, lengths = [63, 64, 65]),
	'C = 512, slab not staged': dict(B = 2, C = 512, T = 100, L = 6, N = 3, seed = 6, lean = 3.0),
	'753 frames x 150 labels': dict(B = 2, C = 38, T = 753, L = 147, N = 4, seed = 7, lean = 2.0, olen = [753, 700]),
	'the most labels': dict(B = 1, C = 38, T = 540, L = 508, N = 3, seed = 8, lean = 2.0),
}
SCALE = {'N = 2, C = 5': 3.0, 'one wave of states exactly': 0.1, 'either side of a wave': 0.1, '753 frames x 150 labels': 0.1, 'the most labels': 0.1}


def most_labels(batch):
	"""hypothesis 1 of the 508-label case becomes 511 labels (1,023 states): the base with three more labels around it"""
	hyps, lens = batch[1], batch[2]
	hyps[0, 1, :] = hyps[0, 0, :].roll(1)
	lens[0, 1] = hyps.shape[2]


def dev():
	return torch.device('cuda:0')


def grad_atol(T):
	return 2e-4 * max(1.0, T / 1100) ** 1.5


def share(a, b, rtol, atol):
	"""worst |a - b| / (atol + rtol |b|) over all elements (<= 1: within the bar)"""
	a, b = np.asarray(a, dtype = np.float64), np.asarray(b, dtype = np.float64)
	assert a.shape == b.shape, (a.shape, b.shape)
	return float((np.abs(a - b) / (atol + rtol * np.abs(b))).max()) if a.size else 0.0


def run(lp, hyps, lens, olen, risk, scale, need_grad = True):
	from convasr_amd import ops
	d = dev()
	out = ops.mwer_loss(ops.as_cl(lp.to(d)), hyps.to(d), lens.to(d), olen.to(d), risk.to(d), lp.shape[1] - 1, scale, need_grad = need_grad)
	torch.cuda.synchronize()
	return out


def check(what, out, lp, hyps, lens, olen, risk, scale, infeasible = 0, parity = True):
	"""the four bars against the restatement, each share printed before anything is asserted; `infeasible`: how many PRESENT hypotheses
	have no alignment (the rows built so).  Returns the restatement's values."""
	T = lp.shape[2]
	ref = mwer_ref(lp.numpy(), hyps.numpy(), lens.numpy(), olen.numpy(), risk.numpy(), lp.shape[1] - 1, scale)
	r_loss, r_grad, r_nll, r_post, _ = ref
	loss, grad, nll, post = (t.cpu().numpy() for t in out)
	fin = np.isfinite(r_nll)
	s_nll = share(nll[fin], r_nll[fin], 1e-5, 1e-4)
	s_loss = s_grad = s_post = 0.0
	for b in range(len(r_loss)):
		eps = 1e-4 + 1e-5 * (np.abs(r_nll[b][fin[b]]).max() if fin[b].any() else 0.0)
		rb = risk.numpy()[b][fin[b]]
		R = max(1.0, float(rb.max() - rb.min())) if fin[b].any() else 1.0
		s_loss = max(s_loss, share(loss[b], r_loss[b], 1e-5, 2 * scale * eps * R))
		s_grad = max(s_grad, share(grad[b], r_grad[b], 1e-4, R * (grad_atol(T) + 3 * scale * eps)))
		s_post = max(s_post, share(post[b], r_post[b], 0.0, 2 * scale * eps))
	present = lens.numpy() >= 0
	print(f'mwer {what}: share of the nll bar {s_nll:.3f}, of the loss bar {s_loss:.3f}, of the gradient bar {s_grad:.3f}, of the posterior bar {s_post:.3f} '
	      f'({int((present & ~fin).sum())} infeasible of {int(present.sum())} present; max |grad_ref| {np.abs(r_grad).max():.3g})')
	assert np.array_equal(np.isfinite(nll), fin) and (nll[~fin] == np.inf).all(), (what, nll, r_nll)
	assert int((present & ~fin).sum()) == infeasible, (what, r_nll)
	if parity:
		assert informative(ref), (what, r_post)
	assert s_nll <= 1.0, (what, 'nll', s_nll)
	assert s_loss <= 1.0, (what, 'loss', s_loss)
	assert s_grad <= 1.0, (what, 'grad', s_grad)
	assert s_post <= 1.0, (what, 'hyp_posterior', s_post)
	return ref


@pytest.mark.parametrize('name', list(PARITY))
def test_parity(name):
	from convasr_amd import ops
	per_wave, _, max_labels, _ = ops.mwer_tiles()
	batch = near_base_batch(**PARITY[name])
	scale = SCALE.get(name, 1.0)
	lens = batch[2]
	if name == 'one wave of states exactly':
		assert 2 * batch[1].shape[2] + 1 == per_wave - 1  # 63 labels wide: 127 states, one wave of a sweep
	if name == 'either side of a wave':
		assert [int(v) for v in lens[:, 0]] == [per_wave // 2 - 1, per_wave // 2, per_wave // 2 + 1]  # hypothesis 0 is the base itself: 127, 129 and 131 states
	if name == 'the most labels':
		assert batch[1].shape[2] == max_labels == 511
		most_labels(batch)
		assert int(lens.max()) == max_labels
	out = run(*batch, scale)
	check(name, out, *batch, scale)
	olen = batch[3]
	for b in range(len(olen)):
		assert not out[1][b, :, int(olen[b]):].any()  # exactly 0 beyond olen


def edge_batch():
	"""ten utterances of near-base hypotheses, then rows rebuilt on purpose: lengths 0 and 1, absent hypotheses in the middle of the list,
	a row with every hypothesis absent, a row with one hypothesis only, an infeasible hypothesis (a doubled label with olen one frame short)
	beside feasible ones, a -inf log-prob on a hypothesis' only path, negative and non-integer risks"""
	lp, hyps, lens, olen, risk = near_base_batch(B = 10, C = 5, T = 12, L = 3, N = 5, seed = 33, lean = 0.3)
	lens[0, 1], lens[0, 3] = -1, -7                      # absent in the middle
	lens[1, :] = -1                                      # every hypothesis absent
	lens[2, 1:] = -1                                     # one hypothesis: loss and gradient exactly 0
	lens[3, 0], lens[3, 1] = 0, 1                        # the empty transcript and a single label beside the variants
	hyps[4, 2, :6], lens[4, 2], olen[4] = torch.tensor([0, 0, 1, 1, 2, 2]), 6, 8   # "a a b b c c" needs 9 frames, olen is 8: infeasible
	hyps[4, 3, :5], lens[4, 3] = torch.tensor([0, 0, 1, 1, 2]), 5                   # ... and this one fits exactly (8 frames): a single path
	hyps[5, 1, :6], lens[5, 1], olen[5] = torch.tensor([3, 2, 3, 2, 3, 2]), 6, 6   # six labels in six frames: one path only
	lp[5, 3, 2] = -float('inf')                          # ... which a -inf log-prob closes
	risk[6] = torch.tensor([-2.5, 0.125, 7.75, -0.5, 1.0])
	olen[7] = 11
	return lp, hyps, lens, olen, risk


@pytest.mark.parametrize('scale', [0.1, 1.0, 3.0])
def test_edge_rows(scale):
	batch = edge_batch()
	out = run(*batch, scale)
	ref = check(f'edge rows, scale {scale}', out, *batch, scale, infeasible = 2)
	loss, grad, nll, post = out
	assert float(loss[1]) == 0.0 and not grad[1].any() and not post[1].any() and bool(torch.isinf(nll[1]).all())
	assert float(loss[2]) == 0.0 and not grad[2].any() and float(post[2, 0]) == 1.0 and not post[2, 1:].any()
	assert float(post[0, 1]) == 0.0 and float(post[0, 3]) == 0.0 and float(post[4, 2]) == 0.0 and float(post[5, 1]) == 0.0
	assert np.isfinite(ref[2][4, 3]) and not grad[7, :, 11:].any()


def test_one_hypothesis_is_exactly_zero_and_the_envelope_is_refused():
	from convasr_amd import _lib, ops
	_, _, max_labels, max_hyps = ops.mwer_tiles()
	lp, hyps, lens, olen, risk = near_base_batch(B = 2, C = 5, T = 12, L = 3, N = 1, seed = 12)
	loss, grad, nll, post = run(lp, hyps, lens, olen, risk + 2.0, 1.0)
	assert not loss.any() and not grad.any() and bool(torch.isfinite(nll).all()) and bool((post == 1.0).all())
	with pytest.raises(_lib.ConvasrHipError, match = 'envelope'):
		run(*near_base_batch(B = 1, C = 5, T = 12, L = 3, N = max_hyps + 1, seed = 0), 1.0)
	lp, hyps, lens, olen, risk = near_base_batch(B = 1, C = 5, T = 12, L = 3, N = 2, seed = 0)
	with pytest.raises(_lib.ConvasrHipError, match = 'envelope'):
		run(lp, torch.nn.functional.pad(hyps, (0, max_labels + 1 - hyps.shape[2])), lens, olen, risk, 1.0)


def test_olen_on_both_sides_of_the_renormalisation_block():
	from convasr_amd import ops
	R = ops.mwer_tiles()[1]
	base = R * -(-6 // R)
	olen = [base - 1, base, base + 1, 2 * base, 2 * base + 1]
	batch = near_base_batch(B = 5, C = 38, T = 2 * base + 1, L = 2, N = 3, seed = 13, lean = 1.0, olen = olen)
	out = run(*batch, 1.0)
	check(f'olen {olen}', out, *batch, 1.0)


def test_repeated_runs_are_bit_equal_and_need_grad_false_is_the_same_forward():
	batch = near_base_batch(B = 4, C = 38, T = 200, L = 40, N = 5, seed = 14, lean = 2.0, olen = [200, 150, 120, 200])
	first = run(*batch, 0.1)
	again = run(*batch, 0.1)
	assert all(torch.equal(a, b) for a, b in zip(first, again))
	assert float(first[1].abs().max()) > 0
	forward_only = run(*batch, 0.1, need_grad = False)
	assert forward_only[1] is None and all(torch.equal(forward_only[i], first[i]) for i in (0, 2, 3))
	for b in range(4):   # a row alone in a batch: the same bits
		alone = run(*[t[b:b + 1] for t in batch], 0.1)
		assert all(torch.equal(alone[i], first[i][b:b + 1]) for i in range(4))


def test_every_guard_message(monkeypatch):
	from convasr_amd import _lib, ops
	d = dev()
	lp, hyps, lens, olen, risk = (t.to(d) for t in near_base_batch(B = 2, C = 5, T = 12, L = 3, N = 3, seed = 15))
	lp = ops.as_cl(lp)
	with pytest.raises(_lib.ConvasrHipError, match = 'MI355X only'):
		ops.mwer_loss(lp.cpu(), hyps, lens, olen, risk, 4)
	with pytest.raises(ValueError, match = 'int64 hyps of shape'):
		ops.mwer_loss(lp, hyps.int(), lens, olen, risk, 4)
	with pytest.raises(ValueError, match = 'int64 hyps of shape'):
		ops.mwer_loss(lp, hyps[:1], lens, olen, risk, 4)
	with pytest.raises(ValueError, match = 'hyp_lengths and risk of shape'):
		ops.mwer_loss(lp, hyps, lens[:, :2], olen, risk, 4)
	with pytest.raises(ValueError, match = 'hyp_lengths and risk of shape'):
		ops.mwer_loss(lp, hyps, lens, olen, risk[:, :2], 4)
	with pytest.raises(ValueError, match = 'olen of shape'):
		ops.mwer_loss(lp, hyps, lens, olen[:1], risk, 4)
	for bad in (0, -1.0, float('nan'), float('inf'), None):
		with pytest.raises(ValueError, match = 'scale must be a finite number > 0'):
			ops.mwer_loss(lp, hyps, lens, olen, risk, 4, scale = bad)
	with pytest.raises(_lib.ConvasrHipError, match = 'bad arguments'):
		ops.mwer_loss(lp, hyps, lens, olen, risk, 5)  # blank outside [0, C)
	need = ops._query('convasr_mwer_workspace_bytes', 2, 3, 12, 5, hyps.shape[2])
	monkeypatch.setattr(ops, 'MWER_WORKSPACE_CAP', need - 1)
	with pytest.raises(_lib.ConvasrHipError, match = f'mwer_loss: {need} bytes of workspace needed'):
		ops.mwer_loss(lp, hyps, lens, olen, risk, 4)
	monkeypatch.setattr(ops, 'MWER_WORKSPACE_CAP', need)
	assert ops.mwer_loss(lp, hyps, lens, olen, risk, 4)[0].shape == (2, )


def test_functional_mwer_loss_against_float64_autograd_on_the_logits():
	"""through LogSoftmaxFunction, seeded per utterance; the float64 side is autograd through log_softmax and the torch restatement over
	F.ctc_loss (tests/test_mwer_ref.py)"""
	from convasr_amd import functional as Fn, ops
	from test_mwer_ref import torch_restatement
	d = dev()
	B, C, T, scale = 3, 5, 14, 1.0
	_, hyps, lens, olen, risk = near_base_batch(B = B, C = C, T = T, L = 4, N = 4, seed = 16, lean = 1.0, olen = [14, 11, 14])
	logits = near_base_batch(B = B, C = C, T = T, L = 4, N = 4, seed = 16, lean = 1.0, olen = [14, 11, 14])[0] + torch.randn(B, 1, T, generator = torch.Generator().manual_seed(1))  # (un-normalised again)
	seed = torch.tensor([0.5, -2.0, 1.5])
	want_loss, want_grad = np.zeros(B), np.zeros((B, C, T))
	x = logits.double().requires_grad_(True)
	lp64 = x.log_softmax(dim = 1)
	total = 0
	for b in range(B):
		l = torch_restatement(lp64[b], hyps[b].numpy(), lens[b].numpy(), olen[b], risk[b].numpy(), C - 1, scale)
		want_loss[b] = float(l.detach())
		total = total + l * float(seed[b])
	total.backward()
	want_grad = x.grad.numpy()
	ref = mwer_ref(logits.log_softmax(dim = 1).numpy(), hyps.numpy(), lens.numpy(), olen.numpy(), risk.numpy(), C - 1, scale)
	assert informative(ref)
	lg = ops.as_cl(logits.to(d)).requires_grad_(True)
	loss, nll, post = Fn.mwer_loss(Fn.LogSoftmaxFunction.apply(lg), hyps.to(d), lens.to(d), olen.to(d), risk.to(d), C - 1, scale)
	assert not nll.requires_grad and not post.requires_grad and loss.requires_grad
	loss.backward(seed.to(d))
	torch.cuda.synchronize()
	s_loss = s_grad = 0.0
	for b in range(B):
		eps = 1e-4 + 1e-5 * np.abs(ref[2][b]).max()
		R = max(1.0, float(risk[b].max() - risk[b].min()))
		s_loss = max(s_loss, share(loss.detach().cpu().numpy()[b], want_loss[b], 1e-5, 2 * scale * eps * R))
		s_grad = max(s_grad, share(lg.grad.cpu().numpy()[b], want_grad[b], 1e-4, abs(float(seed[b])) * R * (grad_atol(T) + 3 * scale * eps)))
	print(f'functional.mwer_loss vs float64 autograd: share of the loss bar {s_loss:.3f}, of the gradient bar {s_grad:.3f}')
	assert s_loss <= 1.0 and s_grad <= 1.0, (s_loss, s_grad)


def test_a_descent_step_raises_the_better_hypothesis():
	"""no tolerance: two hypotheses of near-equal likelihood with risks 0 and 3; a plain-SGD step on the logits along -grad must raise p of
	the risk-0 hypothesis and lower the loss"""
	from convasr_amd import functional as Fn, ops
	d = dev()
	C, T = 4, 12
	logits = (torch.randn(1, C, T, generator = torch.Generator().manual_seed(3)) * 0.1).to(d)
	hyps, lens = torch.tensor([[[0, 1], [0, 2]]], device = d), torch.tensor([[2, 2]], device = d)
	olen, risk = torch.tensor([T], device = d), torch.tensor([[0.0, 3.0]], device = d)

	def at(lg):
		lg = ops.as_cl(lg).requires_grad_(True)
		loss, _, post = Fn.mwer_loss(Fn.LogSoftmaxFunction.apply(lg), hyps, lens, olen, risk, C - 1, 1.0)
		loss.sum().backward()
		return float(loss.detach()[0]), float(post[0, 0]), lg.grad

	loss0, p0, g = at(logits)
	assert 0.3 < p0 < 0.7 and float(g.abs().max()) > 0
	loss1, p1, _ = at(logits - 1.0 * g)
	assert p1 > p0 and loss1 < loss0, (p0, p1, loss0, loss1)


def peaked(paths, C, T, hi = 6.0):
	"""log-probs (B, C, T) sharply peaked on a frame labelling per utterance"""
	logits = torch.full((len(paths), C, T), -hi)
	for b, path in enumerate(paths):
		logits[b, path, torch.arange(len(path))] = hi
	return logits.log_softmax(dim = 1)


def test_hypotheses_against_beam_search_and_edit_distance_by_hand():
	from convasr_amd import _lib, ctc, ops
	d = dev()
	C, T, sp = 38, 50, 36
	lp, _, _, olen, _ = near_base_batch(B = 4, C = C, T = T, L = 10, N = 2, seed = 17, lean = 2.0, olen = [50, 44, 30, 50])
	lp, olen = ops.as_cl(lp.to(d)), olen.to(d)
	g = torch.Generator().manual_seed(4)
	y = torch.randint(0, 36, (4, 12), generator = g)
	y[:, 3::4] = sp
	y, ylen = y.to(d), torch.tensor([12, 9, 5, 12], device = d)
	for unit in ('words', 'chars'):
		mwer = ctc.MWER(4, 16, weight = 1.0, ctc_weight = 1.0, unit = unit, space = sp if unit == 'words' else None)
		hyps, lens, risk = mwer.hypotheses(lp, olen, y, ylen)
		tokens, _, out_lengths, score = ops.ctc_beam_search(lp, olen, C - 1, 16, topk = 4)
		L = int(out_lengths.max())
		dist, _ = ops.edit_distance(tokens[:, :, :L].contiguous(), out_lengths, y, ylen, *((_lib.METRIC_WORDS, sp) if unit == 'words' else (_lib.METRIC_CHARS, )))
		assert bool(torch.isfinite(score).all()) and int(mwer.skipped) == 0
		assert hyps.dtype == torch.int64 and risk.dtype == torch.float32 and hyps.shape == (4, 4, L)
		assert torch.equal(hyps, tokens[:, :, :L]) and torch.equal(lens, out_lengths) and torch.equal(risk, dist.float())
		assert float(risk.max()) > 0


def test_include_reference_when_it_is_and_is_not_in_the_list():
	from convasr_amd import ctc, ops
	d = dev()
	C, T = 6, 24
	paths = [[5, 0, 0, 5, 1, 5, 2, 2, 5, 3] + [5] * 14, [5, 4, 5, 3, 5, 2] + [5] * 18]
	lp = ops.as_cl(peaked(paths, C, T).to(d))
	olen = torch.tensor([T, T], device = d)
	y = torch.tensor([[0, 1, 2, 3, 0, 0], [0, 1, 0, 1, 0, 1]], device = d)  # row 0: the best hypothesis (4 labels; the padding differs); row 1: not in the list, and longer than every hypothesis
	ylen = torch.tensor([4, 6], device = d)
	plain = ctc.MWER(3, 8, weight = 1.0, ctc_weight = 1.0, unit = 'chars')
	with_ref = ctc.MWER(3, 8, weight = 1.0, ctc_weight = 1.0, unit = 'chars', include_reference = True)
	h0, l0, r0 = plain.hypotheses(lp, olen, y, ylen)
	h1, l1, r1 = with_ref.hypotheses(lp, olen, y, ylen)
	L0 = h0.shape[2]
	assert 4 <= L0 < 6 and h1.shape[2] == 6  # (the list is padded to the reference's length where that is longer)
	assert int(l0[0, 0]) == 4 and h0[0, 0, :4].tolist() == [0, 1, 2, 3] and float(r0[0, 0]) == 0.0
	assert torch.equal(h1[0, :, :L0], h0[0]) and torch.equal(l1[0], l0[0]) and torch.equal(r1[0], r0[0])  # in the list: untouched
	assert torch.equal(h1[1, :2, :L0], h0[1, :2]) and torch.equal(l1[1, :2], l0[1, :2]) and torch.equal(r1[1, :2], r0[1, :2])
	assert h1[1, 2].tolist() == [0, 1, 0, 1, 0, 1] and int(l1[1, 2]) == 6 and float(r1[1, 2]) == 0.0 and float(r0[1].min()) > 0
	out = ops.mwer_loss(lp, h1, l1, olen, r1, C - 1)
	assert bool(torch.isfinite(out[2][1, 2]))


def test_an_utterance_with_a_hypothesis_past_the_envelope_is_counted_not_raised_on():
	from convasr_amd import ctc, ops
	d = dev()
	max_labels = ops.mwer_tiles()[2]
	C, T = 5, max_labels + 9
	paths = [[t % 2 for t in range(T)], [4, 0, 4, 1, 4, 2] + [4] * (T - 6)]  # "a b a b ...": a label every frame
	lp = ops.as_cl(peaked(paths, C, T).to(d))
	olen = torch.tensor([T, 20], device = d)
	y, ylen = torch.tensor([[0, 1, 0], [0, 1, 2]], device = d), torch.tensor([3, 3], device = d)
	mwer = ctc.MWER(2, 4, weight = 1.0, ctc_weight = 1.0, unit = 'chars')
	hyps, lens, risk = mwer.hypotheses(lp, olen, y, ylen)
	assert int(mwer.skipped) == 1 and hyps.shape[2] <= max_labels
	assert bool((lens[0] == -1).all()) and int(lens[1, 0]) == 3 and float(risk[1, 0]) == 0.0
	loss, grad, nll, post = ops.mwer_loss(lp, hyps, lens, olen, risk, C - 1)
	assert float(loss[0]) == 0.0 and not grad[0].any() and bool(torch.isinf(nll[0]).all()) and bool(torch.isfinite(loss[1]))


def tiny_model(d, seed = 0):
	import convasr_amd as ca
	torch.manual_seed(seed)
	fe = ca.models.LogFilterBankFrontend(64, 8000, 0.02, 0.01, 'hann_window')
	return ca.models.Wav2Letter(64, [38], frontend = fe, dropout = 0, base_width = 64, check_time_dim_padded = False).to(d)


def tiny_batch(d):
	rng = np.random.default_rng(0)
	x = torch.from_numpy(rng.uniform(-1, 1, (3, 8192)).astype(np.float32)).to(d)
	y = torch.from_numpy(rng.integers(0, 37, (3, 1, 9))).to(d)
	y[:, 0, 4] = 36
	return x, torch.tensor([1.0, 0.8, 0.6], device = d), y, torch.tensor([[9], [7], [5]], device = d)


def test_model_option_train_step_eval_and_refusals():
	from convasr_amd import ctc, functional as Fn, train
	d = dev()
	batch = tiny_batch(d)
	x, xlen, y, ylen = batch
	mwer = ctc.MWER(4, 16, weight = 0.7, ctc_weight = 0.5, unit = 'words', space = 36, include_reference = True)
	model = tiny_model(d, seed = 5).train()
	assert model.ctc_mwer is None
	plain = model(x, xlen, y = y, ylen = ylen)
	del model.ctc_mwer  # the same model without the attribute: ctc_mwer = None must equal it bit for bit
	bare = model(x, xlen, y = y, ylen = ylen)
	assert not any(k.startswith('mwer') for k in plain) and torch.equal(plain['loss'], bare['loss']) and torch.equal(plain['log_probs'][0], bare['log_probs'][0])
	model.ctc_mwer = mwer
	out = model(x, xlen, y = y, ylen = ylen)
	for k, shape in (('mwer_loss', (3, )), ('mwer_expected_risk', (3, )), ('mwer_best_risk', (3, )), ('mwer_skipped', ())):
		assert tuple(out[k].shape) == shape, k
	ctc_part = Fn.ctc_loss(out['log_probs'][0].detach(), y[:, 0], out['olen'][0], ylen[:, 0], 37, norm = ylen[:, 0])
	assert torch.equal(out['loss'].detach(), 0.5 * ctc_part + 0.7 * out['mwer_loss'].detach())  # ctc_weight * the plain loss + weight * mwer_loss
	assert int(out['mwer_skipped']) == 0 and bool(torch.isfinite(out['loss']).all()) and bool((out['mwer_expected_risk'] >= 0).all())
	# eval(): the plain loss, bit for bit, whatever ctc_mwer holds
	model.eval()
	with torch.no_grad():
		with_option = model(x, xlen, y = y, ylen = ylen)
		del model.ctc_mwer
		without = model(x, xlen, y = y, ylen = ylen)
	assert not any(k.startswith('mwer') for k in with_option) and torch.equal(with_option['loss'], without['loss']) and torch.equal(with_option['log_probs'][0], without['log_probs'][0])
	# one training step
	model = tiny_model(d, seed = 5).train()
	model.ctc_mwer = mwer
	opt = train.SGD(train.FlatParameters(model), lr = 1e-2, momentum = 0.9, weight_decay = 1e-3)
	before = opt.flat.data.clone()
	res = train.train_step(model, opt, *batch)
	torch.cuda.synchronize()
	assert bool(torch.isfinite(res['loss'])) and bool(torch.isfinite(res['grad_norm'])) and not torch.equal(opt.flat.data, before) and bool(torch.isfinite(opt.flat.data).all())
	assert all(k in res for k in ('mwer_loss', 'mwer_expected_risk', 'mwer_best_risk', 'mwer_skipped')) and not res['mwer_loss'].requires_grad
	plain_model = tiny_model(d, seed = 5).train()
	res_plain = train.train_step(plain_model, train.SGD(train.FlatParameters(plain_model), lr = 1e-2, momentum = 0.9, weight_decay = 1e-3), *batch)
	assert not any(k.startswith('mwer') for k in res_plain)
	# refusals
	with pytest.raises(ValueError, match = 'eager only'):
		train.GraphedTrainStep(model, opt)
	stepper = train.GraphedTrainStep(plain_model, train.SGD(train.FlatParameters(plain_model), lr = 1e-2, momentum = 0.9, weight_decay = 1e-3))
	plain_model.ctc_mwer = mwer
	with pytest.raises(ValueError, match = 'beam search allocates per call'):
		stepper(*batch)
	model.ctc_star = ctc.StarCTC('ends', penalty = -0.5, enter = -1.0)
	with pytest.raises(ValueError, match = 'ctc_mwer and ctc_star'):
		model(x, xlen, y = y, ylen = ylen)
