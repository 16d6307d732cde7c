"""The star-token CTC kernel (csrc/star_ctc.hip) against the float64 restatement of its lattice (tests/_star_ctc_ref.py, itself pinned
against a subset sum through F.ctc_loss in tests/test_star_ctc_ref.py), and the option up to the model's surface.

The error bars are those of tests/test_kernels_gpu.py and tests/test_ctc_loss_long_gpu.py: nll rtol 1e-5 / atol 1e-4, gradient rtol 1e-4 /
atol 2e-4 max(1, T / 1100)^1.5, and for star_frames rtol 1e-4 / atol the gradient's atol times olen[b] (each of its olen summands is a
posterior like the gradient's).  Every check prints its worst share of each bar before it asserts (pytest -s shows them)."""
import numpy as np
import pytest
import torch

from _star_ctc_ref import star_ctc_ref

pytestmark = pytest.mark.gpu


def dev():
	return torch.device('cuda:0')


def grad_atol(T):
	return 2e-4 * max(1.0, T / 1100) ** 1.5


def share(a, b, rtol, atol):
	"""worst |a - b| / (atol + rtol |b|) over all elements (<= 1: within the bar)"""
	a, b = np.asarray(a, dtype = np.float64), np.asarray(b, dtype = np.float64)
	assert a.shape == b.shape, (a.shape, b.shape)
	return float((np.abs(a - b) / (atol + rtol * np.abs(b))).max()) if a.size else 0.0


def random_batch(B, C, T, S, seed, scale = 1.0, space = None):
	torch.manual_seed(seed)
	lp = (torch.randn(B, C, T) * scale).log_softmax(dim = 1)
	y = torch.randint(0, C - 1, (B, S))
	if S >= 3:
		y[-1, : S // 3] = y[-1, 0]  # repeats: no s-2 move there
	if space is not None and S >= 8:
		y[:, 3::5] = space
	return lp, y


def run(lp, y, olen, ylen, mask, penalty, enter, need_grad = True):
	from convasr_amd import ops
	d = dev()
	out = ops.star_ctc_loss(ops.as_cl(lp.to(d)), y.to(d), olen.to(d), ylen.to(d), lp.shape[1] - 1, mask.to(d), penalty, enter, need_grad = need_grad)
	torch.cuda.synchronize()
	return out


def check(what, out, lp, y, olen, ylen, mask, penalty, enter, infeasible = 0):
	"""the three bars against the restatement, each share printed before anything is asserted; `infeasible`: how many rows have no path"""
	T = lp.shape[2]
	rn, rg, rf = star_ctc_ref(lp.numpy(), y.numpy(), olen.numpy(), ylen.numpy(), lp.shape[1] - 1, mask.numpy(), penalty, enter)
	nll, grad, frames = out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy()
	fin = np.isfinite(rn)
	s_nll = share(nll[fin], rn[fin], 1e-5, 1e-4)
	s_grad = share(grad, rg, 1e-4, grad_atol(T))
	s_fr = max([share(frames[b], rf[b], 1e-4, grad_atol(T) * max(int(olen[b]), 1)) for b in range(len(rn))])
	print(f'star_ctc {what}: share of the nll bar {s_nll:.3f}, of the gradient bar {s_grad:.3f}, of the star_frames bar {s_fr:.3f} ({int((~fin).sum())} infeasible of {len(rn)})')
	assert np.array_equal(np.isfinite(nll), fin) and (nll[~fin] == np.inf).all(), (what, nll, rn)
	assert int((~fin).sum()) == infeasible, (what, rn)
	assert s_nll <= 1.0, (what, 'nll', s_nll)
	assert s_grad <= 1.0, (what, 'grad', s_grad)
	assert s_fr <= 1.0, (what, 'star_frames', s_fr)
	return rn, rg, rf


def padded(rows, S_max, T, C, seed, scale = 2.0):
	"""rows of (labels, mask of len(labels) + 1 entries, olen) -> a batch; labels and mask entries past ylen are set (they must be ignored)"""
	torch.manual_seed(seed)
	B = len(rows)
	lp = (torch.randn(B, C, T) * scale).log_softmax(dim = 1)
	y = torch.full((B, S_max), C - 2, dtype = torch.int64)
	mask = torch.ones(B, S_max + 1, dtype = torch.bool)
	for b, (labels, m, _) in enumerate(rows):
		y[b, :len(labels)] = torch.tensor(labels, dtype = torch.int64)
		mask[b, :len(m)] = torch.tensor(m, dtype = torch.bool)
	return lp, y, torch.tensor([r[2] for r in rows]), torch.tensor([len(r[0]) for r in rows]), mask


a, b_ = 0, 1
EDGES = [([], [0], 1), ([], [1], 1), ([], [1], 2), ([], [0], 2), ([], [1], 6),
         ([a], [0, 0], 1), ([a], [1, 1], 1), ([a], [1, 0], 2), ([a], [0, 1], 2), ([a], [1, 1], 6),
         ([a, a], [0, 1, 0], 3), ([a, a], [0, 1, 0], 6), ([a, a], [1, 1, 1], 3), ([a, a], [0, 0, 0], 2),  # the last one: no path on purpose ("a a" needs three frames)
         ([a, b_, a], [0, 1, 1, 0], 3), ([a, b_, a], [1, 1, 1, 1], 6), ([a, b_, a], [0, 0, 0, 0], 6), ([a, b_, a], [0, 0, 1, 0], 4), ([b_, a, a], [0, 0, 1, 1], 5)]


@pytest.mark.parametrize('penalty, enter', [(0.0, 0.0), (-0.3, -0.7), (-2.0, 0.0)])
def test_edge_lattices_and_repeated_labels(penalty, enter):
	"""T = 1 and 2, S = 0 with and without a star, S = 1, "a a" with a star between (where the s - 4 arc must not exist), "a b a"; with both
	penalties 0 a wrong extra arc shows as double counting"""
	batch = padded(EDGES, 3, 6, 5, seed = 1)
	out = run(*batch, penalty, enter)
	check(f'edges, penalties {penalty} {enter}', out, *batch, penalty, enter, infeasible = 1)


def test_ragged_batch_with_mask_entries_past_ylen():
	lp, y = random_batch(5, 38, 60, 12, seed = 2)
	olen, ylen = torch.tensor([60, 31, 47, 25, 60]), torch.tensor([12, 7, 0, 1, 12])
	torch.manual_seed(3)
	mask = torch.rand(5, 13) < 0.5
	mask[1, 8:] = True
	mask[2, 1:] = True
	out = run(lp, y, olen, ylen, mask, -0.4, -1.0)
	check('ragged', out, lp, y, olen, ylen, mask, -0.4, -1.0)
	assert not out[1].cpu()[1, :, 31:].any() and not out[2].cpu()[2, 1:].any()  # zero beyond olen; no star_frames beyond ylen


@pytest.mark.parametrize('k', [1, 2])
def test_state_counts_on_both_sides_of_a_lane_group(k):
	from convasr_amd import ops
	per_wave = ops.star_ctc_tiles()[0]
	assert per_wave % 4 == 0
	# every gap starred: 4 S + 3 states; one gap left out: 4 S + 1
	S_lo, S_hi = (k * per_wave - 4) // 4, k * per_wave // 4
	T = 3 * S_hi
	lp, y = random_batch(3, 38, T, S_hi + 2, seed = 10 + k)
	ylen = torch.tensor([S_lo, S_hi, S_hi + 2])
	mask = torch.ones(3, S_hi + 3, dtype = torch.bool)
	mask[1, S_hi // 2] = False
	states = [2 * (int(ylen[i]) + int(mask[i, :int(ylen[i]) + 1].sum())) + 1 for i in range(3)]
	assert states[:2] == [k * per_wave - 1, k * per_wave + 1], states
	olen = torch.tensor([T, T - 5, T])
	out = run(lp, y, olen, ylen, mask, -0.2, -0.5)
	check(f'{states} states', out, lp, y, olen, ylen, mask, -0.2, -0.5)


def test_the_largest_lattice():
	from convasr_amd import ops
	max_states = ops.star_ctc_tiles()[2]
	S = (max_states - 3) // 4
	lp, y = random_batch(1, 38, S + 100, S, seed = 20)
	olen, ylen, mask = torch.tensor([S + 100]), torch.tensor([S]), torch.ones(1, S + 1, dtype = torch.bool)
	assert 4 * S + 3 == max_states == 1023
	out = run(lp, y, olen, ylen, mask, -0.5, -1.0)
	check(f'{max_states} states', out, lp, y, olen, ylen, mask, -0.5, -1.0)
	with pytest.raises(Exception, match = 'envelope'):
		run(*random_batch(1, 38, 8, S + 1, seed = 0), torch.tensor([8]), torch.tensor([1]), torch.ones(1, S + 2, dtype = torch.bool), -0.5, -1.0)


def test_frames_on_both_sides_of_the_renormalisation_block():
	from convasr_amd import ops
	R = ops.star_ctc_tiles()[1]
	base = R * -(-5 // R)  # the first block boundary at which three labels fit on its short side
	olen = torch.tensor([base - 1, base, base + 1, 2 * base, 2 * base + 1])  # both sides of a block's end, and whole blocks plus one frame
	lp, y = random_batch(5, 38, 2 * base + 1, 3, seed = 30, scale = 3.0)
	ylen, mask = torch.full((5, ), 3), torch.ones(5, 4, dtype = torch.bool)
	out = run(lp, y, olen, ylen, mask, -0.3, -0.7)
	check(f'olen {olen.tolist()}', out, lp, y, olen, ylen, mask, -0.3, -0.7)


@pytest.mark.parametrize('mode', ['ends', 'words', 'all'])
def test_each_mode_of_star_gaps(mode):
	from convasr_amd import ctc
	space = 36
	lp, y = random_batch(4, 38, 200, 40, seed = 40, space = space)
	olen, ylen = torch.tensor([200, 150, 120, 200]), torch.tensor([40, 31, 20, 40])
	mask = ctc.star_gaps(y.to(dev()), ylen.to(dev()), mode, space = space).cpu()
	words = sum(len({0, int(ylen[i])} | {g for g in range(int(ylen[i])) if int(y[i, g]) == space}) for i in range(4))
	assert mask.shape == (4, 41) and int(mask.sum()) == {'ends': 8, 'words': words, 'all': int(ylen.sum()) + 4}[mode] and words > 24
	out = run(lp, y, olen, ylen, mask, -0.5, -2.0)
	check(f'mode {mode}', out, lp, y, olen, ylen, mask, -0.5, -2.0)


def test_the_workload_row_753_frames_603_states():
	lp, y = random_batch(2, 38, 753, 150, seed = 50)
	olen, ylen, mask = torch.tensor([753, 700]), torch.tensor([150, 131]), torch.ones(2, 151, dtype = torch.bool)
	out = run(lp, y, olen, ylen, mask, -0.5, -1.0)
	check('2 x 753 x 150, all gaps', out, lp, y, olen, ylen, mask, -0.5, -1.0)


def test_512_classes():
	lp, y = random_batch(2, 512, 40, 8, seed = 60)
	olen, ylen = torch.tensor([40, 33]), torch.tensor([8, 5])
	mask = torch.tensor([[1, 0, 1, 0, 1, 0, 1, 0, 1], [1, 1, 1, 1, 1, 1, 1, 1, 1]], dtype = torch.bool)
	out = run(lp, y, olen, ylen, mask, -1.0, -1.0)
	check('C = 512', out, lp, y, olen, ylen, mask, -1.0, -1.0)


def test_infinite_log_probs_and_rows_without_a_path():
	from convasr_amd import ops
	lp, y = random_batch(4, 38, 30, 6, seed = 70)
	y[:, :] = torch.tensor([3, 4, 5, 6, 7, 8])
	lp[0, 5, :] = -float('inf')   # a needed label, everywhere: no path, star or not
	lp[1, 20, :] = -float('inf')  # a class no path needs
	lp[2, 5, 10:] = -float('inf')  # a needed label on most frames: it has to be early
	olen, ylen, mask = torch.tensor([30, 30, 30, 5]), torch.full((4, ), 6), torch.ones(4, 7, dtype = torch.bool)  # row 3: six labels in five frames
	out = run(lp, y, olen, ylen, mask, -0.3, -0.7)
	check('-inf log-probs', out, lp, y, olen, ylen, mask, -0.3, -0.7, infeasible = 2)
	d = dev()
	plain = ops.ctc_loss(ops.as_cl(lp.to(d)), y.to(d), olen.to(d), ylen.to(d), 37)
	for b in (0, 3):  # what the plain loss gives for them: +inf and a zero gradient
		assert float(plain[0][b]) == float('inf') == float(out[0][b]) and torch.equal(out[1][b], plain[1][b]) and not out[1][b].any() and not out[2][b].any()


def test_an_all_false_mask_is_the_plain_loss():
	from convasr_amd import ops
	d = dev()
	lp, y = random_batch(4, 38, 300, 50, seed = 80)
	olen, ylen = torch.tensor([300, 211, 90, 300]), torch.tensor([50, 30, 50, 0])
	mask = torch.zeros(4, 51, dtype = torch.bool)
	out = run(lp, y, olen, ylen, mask, -0.3, -0.7)
	plain = ops.ctc_loss(ops.as_cl(lp.to(d)), y.to(d), olen.to(d), ylen.to(d), 37)
	torch.cuda.synchronize()
	fin = torch.isfinite(plain[0]).cpu().numpy()
	s_nll = share(out[0].cpu().numpy()[fin], plain[0].cpu().numpy()[fin], 1e-5, 1e-4)
	s_grad = share(out[1].cpu().numpy(), plain[1].cpu().numpy(), 1e-4, grad_atol(300))
	print(f'star_ctc all-false mask vs ops.ctc_loss: share of the nll bar {s_nll:.3f}, of the gradient bar {s_grad:.3f}')
	assert fin.all() and torch.equal(torch.isfinite(out[0]).cpu(), torch.isfinite(plain[0]).cpu())
	assert s_nll <= 1.0 and s_grad <= 1.0 and not out[2].any()
	check('all-false mask', out, lp, y, olen, ylen, mask, -0.3, -0.7)


def test_a_row_alone_in_a_batch_and_twice_is_the_same_nll_bit_for_bit():
	lp, y = random_batch(4, 38, 200, 40, seed = 90)
	olen, ylen = torch.tensor([200, 150, 120, 200]), torch.tensor([40, 31, 20, 40])
	torch.manual_seed(91)
	mask = torch.rand(4, 41) < 0.5
	first = run(lp, y, olen, ylen, mask, -0.5, -1.0)
	again = run(lp, y, olen, ylen, mask, -0.5, -1.0)
	assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
	for b in range(4):
		alone = run(lp[b:b + 1], y[b:b + 1], olen[b:b + 1], ylen[b:b + 1], mask[b:b + 1], -0.5, -1.0)
		assert torch.equal(alone[0], first[0][b:b + 1]) and torch.equal(alone[1], first[1][b:b + 1])
	forward_only = run(lp, y, olen, ylen, mask, -0.5, -1.0, need_grad = False)
	assert forward_only[1] is None and torch.equal(forward_only[0], first[0])
	assert share(forward_only[2].cpu().numpy(), first[2].cpu().numpy(), 1e-4, 1e-4) <= 1.0


def test_functional_star_ctc_loss_with_norm_against_float64_autograd_on_the_logits():
	"""through LogSoftmaxFunction; the float64 side is autograd through the subset sum over F.ctc_loss (tests/test_star_ctc_ref.py)"""
	from convasr_amd import functional as Fn, ops
	from test_star_ctc_ref import subset_sum, C, BLANK
	d = dev()
	rng = np.random.default_rng(4)
	B, T, S = 3, 10, 4
	logits = rng.standard_normal((B, C, T)).astype(np.float32) * 2
	y = torch.tensor(rng.integers(0, C - 1, (B, S)))
	ylen, olen = torch.tensor([4, 2, 3]), torch.tensor([10, 7, 10])
	mask = torch.tensor([[1, 0, 1, 0, 1], [1, 1, 1, 1, 1], [0, 1, 0, 1, 0]], dtype = torch.bool)
	seed = torch.tensor([0.5, -2.0, 1.5])
	want_loss, want_grad, want_frames = np.zeros(B), np.zeros((B, C, T)), np.zeros((B, S + 1))
	for b in range(B):
		Tb, Sb = int(olen[b]), int(ylen[b])
		nll, g, fr = subset_sum(logits[b, :, :Tb].astype(np.float64), y[b, :Sb].numpy(), mask[b, :Sb + 1].numpy(), -0.3, -0.7)
		want_loss[b], want_frames[b, :Sb + 1] = nll / Sb, fr
		want_grad[b, :, :Tb] = g * float(seed[b]) / Sb
	lg = ops.as_cl(torch.from_numpy(logits).to(d)).requires_grad_(True)
	lp = Fn.LogSoftmaxFunction.apply(lg)
	loss, frames = Fn.star_ctc_loss(lp, y.to(d), olen.to(d), ylen.to(d), BLANK, mask.to(d), -0.3, -0.7, norm = ylen.to(d))
	assert not frames.requires_grad
	loss.backward(seed.to(d))
	torch.cuda.synchronize()
	s = (share(loss.detach().cpu().numpy(), want_loss, 1e-5, 1e-4), share(lg.grad.cpu().numpy(), want_grad, 1e-4, grad_atol(T)), share(frames.cpu().numpy(), want_frames, 1e-4, grad_atol(T) * T))
	print(f'functional.star_ctc_loss vs float64 autograd: shares of the bars {s[0]:.3f} {s[1]:.3f} {s[2]:.3f}')
	assert max(s) <= 1.0, s


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


def test_model_option_train_step_eval_and_graph_replay():
	from convasr_amd import ctc, train
	d = dev()
	batch = tiny_batch(d)
	star = ctc.StarCTC('words', penalty = -0.5, enter = -1.0, space = 36)

	def make(with_star):
		model = tiny_model(d, seed = 5).train()
		assert model.ctc_star is None
		model.ctc_star = star if with_star else None
		return model, train.SGD(train.FlatParameters(model), lr = 1e-2, momentum = 0.9, weight_decay = 1e-3)

	model, opt = make(True)
	before = opt.flat.data.clone()
	res = train.train_step(model, opt, *batch)
	torch.cuda.synchronize()
	assert not torch.equal(opt.flat.data, before) and bool(torch.isfinite(res['loss']))
	frames = res['star_frames']
	assert len(frames) == 1 and frames[0].shape == (3, 10) and bool((frames[0] >= 0).all()) and float(frames[0].sum()) > 0
	assert not frames[0][~star.mask(batch[2][:, 0], batch[3][:, 0])].any()
	plain_model, plain_opt = make(False)
	res_plain = train.train_step(plain_model, plain_opt, *batch)
	assert 'star_frames' not in res_plain and float(res['loss_cur']) < float(res_plain['loss_cur'])  # a star only adds paths (from the same initial weights)
	# eval(): the plain loss, bit for bit, whatever ctc_star holds
	model.eval()
	with torch.no_grad():
		with_option = model(batch[0], batch[1], y = batch[2], ylen = batch[3])
		model.ctc_star = None
		without = model(batch[0], batch[1], y = batch[2], ylen = batch[3])
	assert 'star_frames' not in with_option and torch.equal(with_option['loss'], without['loss'])
	# a captured step holds kernel nodes only, and its replay is the eager step
	eager_model, eager_opt = make(True)
	graph_model, graph_opt = make(True)
	stepper = train.GraphedTrainStep(graph_model, graph_opt)
	losses = []
	for step in range(3):
		e = train.train_step(eager_model, eager_opt, *batch)
		g = stepper(*batch)
		torch.cuda.synchronize()
		losses.append((e['loss'].clone(), g['loss'].clone(), e['star_frames'][0].clone(), g['star_frames'][0].clone()))
	assert stepper.captures == 1 and stepper.replays >= 1 and not stepper.non_kernel_nodes
	assert all(set(k['node_kinds']) == {'kernel'} for k in stepper.graphs.values()), [k['node_kinds'] for k in stepper.graphs.values()]
	for e_loss, g_loss, e_fr, g_fr in losses:
		assert torch.equal(e_loss, g_loss)
		assert share(g_fr.cpu().numpy(), e_fr.cpu().numpy(), 1e-4, 1e-4) <= 1.0  # (star_frames: fp32 atomics between workgroups, equal to rounding)
	assert torch.equal(eager_opt.flat.data, graph_opt.flat.data)


def test_missing_words_show_up_in_star_frames():
	"""no tolerance: log-probs sharply peaked on the path of "a b c d", the transcript says "a d": the star of gap 1 absorbs the frames, and
	the star loss is below the plain loss"""
	from convasr_amd import ctc, ops
	d = dev()
	C, T = 6, 40
	path = [5] * 4 + [0] * 6 + [5] * 3 + [1] * 7 + [5] * 2 + [2] * 6 + [5] * 3 + [3] * 6 + [5] * 3
	assert len(path) == T
	logits = torch.full((1, C, T), -4.0)
	logits[0, path, torch.arange(T)] = 4.0
	lp = ops.as_cl(logits.log_softmax(dim = 1).to(d))
	y, olen, ylen = torch.tensor([[0, 3]], device = d), torch.tensor([T], device = d), torch.tensor([2], device = d)
	nll, _, frames = ops.star_ctc_loss(lp, y, olen, ylen, 5, ctc.star_gaps(y, ylen, 'all'), -0.5, -1.0)
	plain = ops.ctc_loss(lp, y, olen, ylen, 5)[0]
	torch.cuda.synchronize()
	assert int(frames[0].argmax()) == 1 and float(frames[0, 1]) > 10
	assert float(nll[0]) < float(plain[0])
