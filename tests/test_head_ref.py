"""The float64 restatement tests/_head_ref.py against known answers on the CPU: torch's own float64 ops (F.log_softmax with autograd,
F.instance_norm with running statistics, torch.argmax), the oracle, and the committed goldens helpers.npz / instnorm.npz.  This is what
makes the reference of tests/test_head_kernels_gpu.py trustworthy; nothing here loads the library."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _head_ref as R  # noqa: E402

from oracle import convasr_oracle as O  # noqa: E402

T_ = lambda a: torch.as_tensor(a)


def same(a, b, what, rel = 1e-12):
	"""`rel` of the largest magnitude of the quantity (1e-12: float64 against float64; looser where the other side is an fp32 golden)"""
	a, b = a.detach().double(), b.detach().double()
	assert a.shape == b.shape, (what, a.shape, b.shape)
	err, bar = float((a - b).abs().max()), rel * max(float(b.abs().max()), 1e-30)
	assert err <= bar, f'{what}: max abs err {err:.3e} > {bar:.3e}'


def logits64(B, C, T, scale, seed):
	return torch.randn(B, C, T, dtype = torch.float64, generator = torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize('scale', [3, 30])
@pytest.mark.parametrize('C', [1, 2, 38, 129])
def test_log_softmax_equals_torch_and_its_autograd(C, scale):
	x = logits64(3, C, 17, scale, C).requires_grad_(True)
	g = torch.randn(3, C, 17, dtype = torch.float64, generator = torch.Generator().manual_seed(1))
	lp = F.log_softmax(x, dim = 1)
	lp.backward(g)
	same(R.log_softmax(x), lp, 'log_softmax')
	same(R.log_softmax_bwd(g, lp), x.grad, 'log_softmax backward')
	if C > 1:  # a -inf logit: probability 0, log-probability -inf, the others as if it were not there
		y = x.detach().clone()
		y[1, 0, 5] = float('-inf')
		r = R.log_softmax(y)
		assert torch.equal(r == float('-inf'), y == float('-inf')) and bool(torch.isfinite(r[y != float('-inf')]).all())
		same(r[1, 1:, 5], F.log_softmax(y[1, 1:, 5], dim = 0), 'row with a -inf logit')


def test_entropies_equal_the_oracle():
	lp = F.log_softmax(logits64(4, 38, 23, 3, 2), dim = 1)
	for olen in (None, torch.tensor([23, 0, 1, 22]), torch.tensor([28, 23, 7, 1])):  # (28 > T: the divisor follows olen)
		same(R.entropy(lp, olen), O.entropy(lp, olen), f'entropy {olen}')
		for eps_id in (-1, 0, 3, 37):
			same(R.weighted_mean_entropy(lp, olen, eps_id = eps_id), O.weighted_mean_entropy(lp, olen, eps_id = eps_id), f'weighted_mean_entropy {olen} {eps_id}')
	same(R.entropy(lp, torch.tensor([5, 5, 5, 5]), eps = 0.5), O.entropy(lp, torch.tensor([5, 5, 5, 5]), eps = 0.5), 'entropy, eps 0.5')
	assert torch.equal(R.entropy(lp, torch.tensor([0, 0, 0, 0])), torch.zeros(4, dtype = torch.float64))


def test_helpers_golden(golden):
	g = golden('helpers.npz')
	lp, olen = T_(g['log_probs']), T_(g['olen'])
	same(R.weighted_mean_entropy(lp, olen), T_(g['wme_len']), 'wme_len', 2e-6)  # (the goldens are the reference's fp32 results)
	same(R.weighted_mean_entropy(lp), T_(g['wme_all']), 'wme_all', 2e-6)
	same(R.weighted_mean_entropy(lp, olen, eps_id = 3), T_(g['wme_id3']), 'wme_id3', 2e-6)
	same(R.entropy(lp, olen), T_(g['ent_len']), 'ent_len', 2e-6)
	same(R.normalize_signal(T_(g['signal'])), T_(g['signal_norm']), 'signal_norm', 2e-7)
	same(R.normalize_signal(T_(g['signal']), denom_multiplier = 2.5), T_(g['signal_norm_mult']), 'signal_norm_mult', 2e-7)


def test_normalize_signal_equals_the_oracle_for_float_and_int16():
	gen = torch.Generator().manual_seed(4)
	x = torch.rand(3, 65, generator = gen) * 2 - 1
	x[1] = 0
	x16 = torch.randint(-32768, 32767, (3, 65), generator = gen, dtype = torch.int16)
	x16[0, 0] = -32768
	for s in (x, x16):
		for m in (1.0, 2.5):
			same(R.normalize_signal(s, denom_multiplier = m), O.normalize_signal(s.double(), denom_multiplier = m), 'normalize_signal')
	assert float(R.normalize_signal(x16)[0, 0]) == -32768 / (32768 + 1e-5) and not bool(R.normalize_signal(x)[1].any())


def argmax_rows():
	"""rows of 130 classes with planted ties, infinities and NaNs"""
	gen = torch.Generator().manual_seed(5)
	rows = []
	for plant in ([(3, 9.0), (67, 9.0)], [(10, 9.0), (11, 9.0)], [(40, float('inf')), (100, float('inf'))], [(5, float('nan'))], [(70, float('nan')), (6, float('nan'))],
	              [(5, float('nan')), (37, 50.0)], [(129, float('nan')), (0, float('inf'))], []):
		r = torch.randn(130, generator = gen)
		for c, v in plant:
			r[c] = v
		rows.append(r)
	rows.append(torch.full((130, ), float('-inf')))
	rows.append(torch.full((130, ), float('nan')))
	return torch.stack(rows).t().unsqueeze(0).contiguous()  # (1, C, rows)


def test_argmax_equals_torch_argmax_with_ties_infinities_and_nan():
	x = argmax_rows()
	ref = R.argmax(x)
	assert torch.equal(ref, x.argmax(dim = 1)) and torch.equal(ref, x.double().argmax(dim = 1))
	assert ref[0].tolist() == [3, 10, 40, 5, 6, 5, 129, int(x[0, :, 7].argmax()), 0, 0]
	y = torch.randn(4, 38, 50, generator = torch.Generator().manual_seed(6))
	assert torch.equal(R.argmax(y), y.argmax(dim = 1))


def test_scale_rows_and_loss_head_equal_the_reference_expressions():
	gen = torch.Generator().manual_seed(7)
	g = torch.randn(3, 5, 7, generator = gen)
	sc, dv = torch.rand(3, generator = gen) + 0.5, torch.tensor([3, 11, 200])
	same(R.scale_rows(g, sc), g.double() * sc.double().view(3, 1, 1), 'gscale')
	same(R.scale_rows(g, None, dv), g.double() / dv.double().view(3, 1, 1), 'gdiv')
	same(R.scale_rows(g, sc, dv), g.double() * (sc.double() / dv.double()).view(3, 1, 1), 'both')
	# train.py:754-756 with autograd for d loss / d loss_vec, in fp32 like the reference runs it (gvec is exact) and in float64 for the means
	for B, accum in ((1, 1), (7, 4), (300, 2)):
		lv = (torch.rand(B, generator = gen) * 5 + 0.1).requires_grad_(True)
		ylen, ent = torch.randint(1, 200, (B, ), generator = gen), torch.rand(B, generator = gen)
		((lv * ylen).mean() / accum).backward()
		out3, gvec, skipped = R.loss_head(lv, ylen, ent, accum, metric_scale = 0.25)
		same(out3, torch.stack([(lv.double() * ylen).mean() / accum, lv.double().mean() * 0.25, ent.double().mean() * 0.25]), 'out3')
		assert gvec.dtype == torch.float32 and not skipped
		same(gvec, lv.grad, 'gvec against autograd (fp32, any order of the three factors)', 2e-7)
		assert torch.equal(R.loss_head(lv, ylen, None, accum, loss_scale = 4096.0)[1], gvec * 4096.0)
		assert float(R.loss_head(lv, ylen, None, accum)[0][2]) == 0.0
	for bad in ([float('inf')], [float('-inf')], [float('nan')], [float('inf'), float('-inf')]):
		v = lv.detach().clone()
		v[:len(bad)] = torch.tensor(bad)
		assert R.loss_head(v, ylen)[2] is True


def test_output_lengths_equal_the_oracle_and_the_golden(golden):
	g = golden('instnorm.npz')
	assert torch.equal(R.output_lengths(T_(g['xlen']), 4, 201), T_(g['lengths']))
	assert torch.equal(R.output_lengths(None, 3, 7), torch.full((3, ), 7))
	for T in (1, 2, 753, 1501):
		k = torch.arange(0, T + 1, max(1, T // 50), dtype = torch.float32)
		frac = k / T
		xl = torch.cat([frac, torch.nextafter(frac, torch.tensor(2.0)), torch.nextafter(frac, torch.tensor(-1.0)).clamp_min(0)])
		assert torch.equal(R.output_lengths(xl, xl.numel(), T), O.compute_output_lengths(T, xl))
	assert R.output_lengths(torch.tensor([0.0, 1.0]), 2, 753).tolist() == [0, 753]


def test_instnorm_golden_and_oracle(golden):
	g = golden('instnorm.npz')
	x, xlen = T_(g['x']), T_(g['xlen'])
	eps = float(torch.finfo(torch.float16).tiny)
	same(R.instnorm(x, xlen, eps), T_(g['y_masked']), 'y_masked', 2e-6)
	same(R.instnorm(x, None, eps), T_(g['y_legacy']), 'y_legacy', 2e-6)
	same(R.instnorm(x, xlen, eps), O.masked_instance_norm(x.double(), T_(g['mask']).reshape(4, 201), eps), 'against the oracle in float64')
	same(R.instnorm(x, None, eps), O.masked_instance_norm(x.double(), None, eps), 'legacy against the oracle in float64')
	y = R.instnorm(x, torch.tensor([0.0, 0.5 / 201, 1.0, 0.3]), eps, T_out = 202)
	assert y.shape == (4, x.shape[1], 202) and not bool(y[0].any()) and not bool(y[1, :, 1:].any()) and not bool(y[:, :, 201].any()) and bool(torch.isfinite(y).all())


@pytest.mark.parametrize('T', [2, 37])
def test_instnorm_running_equals_torch_instance_norm(T):
	gen = torch.Generator().manual_seed(8)
	B, C, eps, mom = 3, 5, 1e-5, 0.1
	rm, rv, nbt = torch.randn(C, dtype = torch.float64, generator = gen), torch.rand(C, dtype = torch.float64, generator = gen) + 0.5, 0
	m = torch.nn.InstanceNorm1d(C, eps = eps, momentum = mom, affine = False, track_running_stats = True).double()
	m.running_mean.copy_(rm); m.running_var.copy_(rv)
	for _ in range(3):
		x = torch.randn(B, C, T, dtype = torch.float64, generator = gen) * 2 + 1
		y, rm, rv, nbt = R.instnorm_running(x, rm, rv, nbt, mom, eps, True)
		same(y, m(x), 'training output')
		same(rm, m.running_mean, 'running_mean'); same(rv, m.running_var, 'running_var')
		assert int(m.num_batches_tracked) == 0  # (torch's InstanceNorm never counts; the kernel's counter, given one, counts the training calls)
	m.eval()
	y, rm2, rv2, nbt2 = R.instnorm_running(x, rm, rv, nbt, mom, eps, False, T_out = T + 1)
	same(y[:, :, :T], m(x), 'eval output')
	assert not bool(y[:, :, T].any()) and torch.equal(rm2, rm) and torch.equal(rv2, rv) and nbt2 == nbt == 3


def test_instnorm_running_one_frame_uses_the_biased_variance():
	"""T = 1 (F.instance_norm refuses it in training mode): every instance's variance is 0, biased or not, so running_var decays by 1 - momentum"""
	x = torch.tensor([[[2.0], [4.0]], [[6.0], [-4.0]]])
	y, rm, rv, nbt = R.instnorm_running(x, torch.zeros(2), torch.ones(2), 5, 0.1, 1e-5, True)
	assert not bool(y.any()) and nbt == 6
	same(rm, torch.tensor([0.4, 0.0], dtype = torch.float64), 'running_mean'); same(rv, torch.tensor([0.9, 0.9], dtype = torch.float64), 'running_var')


def test_exact_ops_are_torch_casts():
	x = torch.tensor([1.0, -0.0, 65520.0, 65519.9, 6e-8, 2.9e-8, 3.1e-8, 1e-40, float('inf'), float('nan'), 1 + 2.0 ** -11, 1 + 2.0 ** -10 + 2.0 ** -11])
	h = R.convert_layout(x, torch.float16)
	assert h[:9].tolist() == [1.0, -0.0, float('inf'), 65504.0, 2.0 ** -24, 0.0, 2.0 ** -24, 0.0, float('inf')] and bool(h[9].isnan()) and torch.signbit(h[1])
	assert h[10:].tolist() == [1.0, 1 + 2.0 ** -9]  # (two ties: each goes to the even neighbour, one down and one up)
	a, b = torch.tensor([1.0, 65504.0, 2.0 ** -24], dtype = torch.float16), torch.tensor([2.0 ** -11, 65504.0, 2.0 ** -24], dtype = torch.float16)
	assert R.add16(a, b).tolist() == [1.0, float('inf'), 2.0 ** -23]  # (1 + 2^-11: a tie, to even)
	assert R.cast_scale(torch.tensor([3.0, 1e30]), 1e10, torch.bfloat16).tolist() == [float(torch.tensor(3e10).to(torch.bfloat16)), float('inf')]
	assert R.cast_scale(torch.tensor([3.0], dtype = torch.float16), 0.125, torch.float32).tolist() == [0.375]
	s = [torch.arange(6, dtype = torch.int16).reshape(2, 3) + 1, torch.zeros(2, 0, dtype = torch.int16), torch.full((2, 4), 7, dtype = torch.int16)]
	out = R.collate_pad(s, 2, 4)
	assert out.tolist() == [[[1, 2, 3, 0], [4, 5, 6, 0]], [[0] * 4, [0] * 4], [[7] * 4, [7] * 4]]
	assert R.copy(torch.arange(9, dtype = torch.uint8), 4).tolist() == [0, 1, 2, 3]
