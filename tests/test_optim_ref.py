"""The float64 restatement tests/_optim_ref.py against known answers on the CPU: torch.optim.SGD and torch.optim.AdamW run in float64 with
torch.nn.utils.clip_grad_norm_, oracle.convasr_oracle.novograd_step, the committed golden novograd.npz, and apex's update_scale() for the
loss scaler.  This is what makes the reference of tests/test_optim_kernels_gpu.py trustworthy; nothing here loads the library.

Hyper-parameters are rounded to fp32 first (R.r32: what a `float` argument of the C ABI holds), so both sides compute with the same numbers.
Without clipping the two sides agree to float64 rounding (1e-12).  With clip_grad_norm_ ACTIVE the restatement takes the coefficient in the
kernels' fp32 order while torch takes it in float64: sqrt -> fp32, + 1e-6f, the division -- three fp32 roundings, 3 x 2^-24 = 1.8e-7 on every
clipped gradient and step; three steps are held to 1e-6.  The oracle's NovoGrad takes the coefficient in fp32 in the same order as the
kernel (total.float(), then torch's fp32 arithmetic), so that comparison stays at 1e-12 with clipping too."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _optim_ref as R  # noqa: E402

from oracle import convasr_oracle as O  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
INF, NAN = float('inf'), float('nan')


def same(a, b, what, rel = 1e-12):
	"""`rel` of the largest magnitude of the quantity"""
	a, b = torch.as_tensor(a, dtype = torch.float64).detach(), torch.as_tensor(b, dtype = torch.float64).detach()
	assert a.shape == b.shape, (what, a.shape, b.shape)
	err, bar = float((a - b).abs().max()), rel * max(float(b.abs().max()), 1e-30)
	assert err <= bar, f'{what}: max abs err {err:.3e} > {bar:.3e}'


def rand32(n, seed, scale = 1.0):
	"""fp32 values (what the device holds)"""
	return torch.randn(n, generator = torch.Generator().manual_seed(seed)) * scale


class ApexLossScaler:
	"""apex/amp/scaler.py LossScaler.update_scale(), restated -- a copy of the class tests/test_fp16_gpu.py holds the kernels to."""

	def __init__(self, init = 2.0 ** 16, factor = 2.0, window = 2000, min_scale = None, max_scale = 2.0 ** 24):
		self.scale, self.unskipped, self.factor, self.window, self.min, self.max = init, 0, factor, window, min_scale, max_scale

	def update(self, overflow):
		if overflow:
			self.scale = max(self.min, self.scale / self.factor) if self.min else self.scale / self.factor
			self.unskipped = 0
		else:
			self.unskipped += 1
		if self.unskipped == self.window:
			self.scale = min(self.max, self.scale * self.factor)
			self.unskipped = 0
		return overflow


# ------------------------------------------------------------------------------------------------ gradient norm, fp32 decisions

def test_sumsq_and_grad_norm_equal_torch_float64():
	g = rand32(1027, 0, 3.0)
	same(R.sumsq(g), g.double().pow(2).sum(), 'sumsq')
	same(R.grad_norm(R.sumsq(g)), torch.linalg.vector_norm(g.double()), 'norm')
	same(R.grad_norm(R.sumsq(g), 0.25, R.scaler_state(1024.0, 3)), torch.linalg.vector_norm(g.double()) * 0.25 / 1024, 'norm, scaled')
	assert R.grad_norm(INF) == INF and np.isnan(R.grad_norm(NAN))


@pytest.mark.parametrize('ss', [0.0, 1e-14, 1.0, 99.0 ** 2, 101.0 ** 2, 3e9, INF, NAN])
@pytest.mark.parametrize('grad_scale, scale', [(1.0, None), (0.25, None), (1.0, 1024.0), (0.25, 65536.0)])
def test_clip_coefficient_is_the_fp32_expression(ss, grad_scale, scale):
	"""clip_coef against the same expression written with torch's fp32 0-d tensors (another fp32 implementation of the same order), and against
	clip_grad_norm_'s float64 value to three fp32 roundings"""
	scaler = None if scale is None else R.scaler_state(scale, 5)
	one, max_norm = torch.tensor(1.0), torch.tensor(100.0)
	gs = torch.tensor(grad_scale) * (one / torch.tensor(scale) if scale is not None else one)
	total = torch.tensor(ss, dtype = torch.float64).sqrt().float() * gs
	c = max_norm / (total + torch.tensor(1e-6))
	exp = float((c if bool(c < 1) else one) * gs)
	got = R.clip_coef(torch.tensor([ss], dtype = torch.float64), 100.0, grad_scale, scaler)
	assert got == exp or (np.isnan(got) and np.isnan(exp)), (got, exp)
	assert R.clip_coef(None, 100.0, grad_scale, scaler) == float(gs) and R.clip_coef(ss, 0.0, grad_scale, scaler) == float(gs), 'no sumsq / max_norm 0: the scale alone'
	if np.isfinite(ss):
		unscale = grad_scale / (scale or 1.0)
		ref = min(1.0, 100.0 / (ss ** 0.5 * unscale + 1e-6)) * unscale
		assert abs(got - ref) <= 4 * 2.0 ** -24 * ref, (got, ref)
	elif ss == INF:
		assert got == 0.0, 'an infinite norm without an overflow verdict clips everything away, as clip_grad_norm_ does'


def test_gate_overflow_and_counters():
	assert not R.is_gated(None) and not R.is_gated(torch.tensor([3.5])) and all(R.is_gated(torch.tensor([v])) for v in (INF, -INF, NAN))
	dyn, static = R.scaler_state(1024.0, 3), R.scaler_state(128.0, 0)
	assert not R.loss_scale_overflow(None, INF) and not R.loss_scale_overflow(static, INF) and not R.loss_scale_overflow(dyn, 1e300)
	assert R.loss_scale_overflow(dyn, INF) and R.loss_scale_overflow(dyn, NAN) and R.loss_scale_overflow(dyn, -INF)
	assert [R.counter_next(v) for v in (0.0, 5.0, 2.0 ** 24 - 1, 2.0 ** 24)] == [1.0, 6.0, 2.0 ** 24, 2.0 ** 24]


# ------------------------------------------------------------------------------------------------ SGD

SGD_CASES = [(0.0, False, 0.0), (0.0, False, 1e-3), (0.9, False, 1e-3), (0.9, True, 1e-3), (0.9, True, 0.0), (0.5, False, 0.0)]


@pytest.mark.parametrize('max_norm', [None, 1e9, 2.0])
@pytest.mark.parametrize('momentum, nesterov, wd', SGD_CASES)
def test_sgd_equals_torch_optim_sgd_float64(momentum, nesterov, wd, max_norm):
	n, lr = 37, R.r32(1e-2)
	momentum, wd = R.r32(momentum), R.r32(wd)
	p0 = rand32(n, 1)
	tp = torch.nn.Parameter(p0.double())
	opt = torch.optim.SGD([tp], lr = lr, momentum = momentum, weight_decay = wd, nesterov = nesterov)
	p, buf = p0.double(), (torch.zeros(n, dtype = torch.float64) if momentum != 0 else None)
	for it in range(3):
		g = rand32(n, 10 + it, 0.5 * (it + 1))
		tp.grad = g.double()
		if max_norm is not None:
			torch.nn.utils.clip_grad_norm_([tp], max_norm)
		opt.step()
		r = R.sgd_step(p, g, buf, R.sumsq(g) if max_norm is not None else None, max_norm or 0.0, lr, momentum, wd, nesterov, it == 0)
		assert r['applied']
		same(r['grad_out'], tp.grad, f'clipped gradient, step {it}', 1e-6 if max_norm == 2.0 else 1e-12)
		p, buf = r['p'], r['buf']
		same(p, tp.detach(), f'parameters, step {it}', 1e-6 if max_norm == 2.0 else 1e-12)
		if momentum != 0:
			same(buf, opt.state[tp]['momentum_buffer'], f'momentum, step {it}', 1e-6 if max_norm == 2.0 else 1e-12)
		else:
			assert buf is None


def test_sgd_grad_scale_loss_scale_and_skipped_steps():
	"""4 x the gradient with grad_scale 1/4, and 1024 x the gradient under a loss scale of 1024, are the plain step (powers of two: exactly);
	a gated or overflowed step returns its inputs and only the scaler moves"""
	n = 21
	p, g, buf = rand32(n, 2), rand32(n, 3), rand32(n, 4)
	plain = R.sgd_step(p, g, buf, R.sumsq(g), 2.0, 1e-2, 0.9, 1e-3, True, False)
	scaled = R.sgd_step(p, g * 4, buf, R.sumsq(g * 4), 2.0, 1e-2, 0.9, 1e-3, True, False, grad_scale = 0.25)
	state = R.scaler_state(1024.0, 3, unskipped = 1.0)
	amp = R.sgd_step(p, g * 1024, buf, R.sumsq(g * 1024), 2.0, 1e-2, 0.9, 1e-3, True, False, scaler = state)
	for k in ('p', 'buf', 'grad_out'):
		same(scaled[k], plain[k], k + ' (grad_scale)', 1e-15)
		same(amp[k], plain[k], k + ' (loss scale)', 1e-15)
	assert amp['scaler_out'].tolist() == [1024.0, 2.0, 0.0, 3.0, 0.0, 2.0 ** 24, 2.0, 0.0]
	same(R.sgd_step(p, g, buf, None, 0.0, 1e-2, 0.9, 1e-3, False, False, lr_dev = torch.tensor([0.5]))['p'], R.sgd_step(p, g, buf, None, 0.0, 0.5, 0.9, 1e-3, False, False)['p'], 'lr_dev')
	for kw, exp_state in ((dict(loss_gate = torch.tensor([NAN]), scaler = state), state.tolist()),
	                      (dict(scaler = state, ss = INF), [512.0, 0.0, 1.0, 3.0, 0.0, 2.0 ** 24, 2.0, 1.0])):
		ss = torch.tensor([kw.pop('ss', float(R.sumsq(g)))], dtype = torch.float64)
		r = R.sgd_step(p, g, buf, ss, 2.0, 1e-2, 0.9, 1e-3, True, False, **kw)
		assert not r['applied'] and r['grad_out'] is None and torch.equal(r['p'], p.double()) and torch.equal(r['buf'], buf.double())
		assert r['scaler_out'].tolist() == exp_state


# ------------------------------------------------------------------------------------------------ AdamW

@pytest.mark.parametrize('max_norm', [None, 1e9, 2.0])
@pytest.mark.parametrize('betas, wd', [((0.9, 0.999), 1e-2), ((0.9, 0.98), 0.0), ((0.0, 0.0), 1e-2)])
def test_adamw_equals_torch_optim_adamw_float64(betas, wd, max_norm):
	n, lr, eps = 37, R.r32(1e-3), R.r32(1e-8)
	betas, wd = (R.r32(betas[0]), R.r32(betas[1])), R.r32(wd)
	p0 = rand32(n, 1)
	tp = torch.nn.Parameter(p0.double())
	opt = torch.optim.AdamW([tp], lr = lr, betas = betas, eps = eps, weight_decay = wd)
	p, m, v, step = p0.double(), torch.zeros(n, dtype = torch.float64), torch.zeros(n, dtype = torch.float64), 0.0
	for it in range(4):
		g = rand32(n, 10 + it, 0.5 * (it + 1))
		g[::5] = 0  # (elements without a gradient: m decays, v decays, with betas (0, 0) the update is 0 / (0 + eps))
		tp.grad = g.double()
		if max_norm is not None:
			torch.nn.utils.clip_grad_norm_([tp], max_norm)
		opt.step()
		r = R.adamw_step(p, g, m, v, R.sumsq(g) if max_norm is not None else None, max_norm or 0.0, lr, betas[0], betas[1], eps, wd, step)
		p, m, v, step = r['p'], r['exp_avg'], r['exp_avg_sq'], r['step_out']
		assert r['applied'] and step == it + 1 == float(opt.state[tp]['step'])
		rel = 1e-6 if max_norm == 2.0 else 1e-12
		same(p, tp.detach(), f'parameters, step {it}', rel)
		same(m, opt.state[tp]['exp_avg'], f'exp_avg, step {it}', rel)
		same(v, opt.state[tp]['exp_avg_sq'], f'exp_avg_sq, step {it}', 2 * rel)


@pytest.mark.parametrize('t0', [999, 10 ** 6])
def test_adamw_bias_corrections_at_a_large_step_count(t0):
	"""torch.optim.AdamW with its step counter preloaded, one step"""
	n, lr, eps, betas, wd = 19, R.r32(1e-3), R.r32(1e-8), (R.r32(0.9), R.r32(0.999)), R.r32(1e-2)
	p0, g, m0, v0 = rand32(n, 1), rand32(n, 2), rand32(n, 3, 0.1), rand32(n, 4).abs() * 0.01
	tp = torch.nn.Parameter(p0.double())
	opt = torch.optim.AdamW([tp], lr = lr, betas = betas, eps = eps, weight_decay = wd)
	opt.state[tp] = dict(step = torch.tensor(float(t0)), exp_avg = m0.double(), exp_avg_sq = v0.double())
	tp.grad = g.double()
	opt.step()
	r = R.adamw_step(p0, g, m0, v0, None, 0.0, lr, betas[0], betas[1], eps, wd, torch.tensor([float(t0)]))
	assert r['step_out'] == t0 + 1
	same(r['p'], tp.detach(), 'parameters')
	same(r['exp_avg_sq'], opt.state[tp]['exp_avg_sq'], 'exp_avg_sq')


def test_adamw_skipped_steps_and_counter_cap():
	n = 9
	p, g, m, v = rand32(n, 1), rand32(n, 2), rand32(n, 3), rand32(n, 4).abs()
	state = R.scaler_state(2.0, 3, min_scale = 2.0)
	for kw, exp_scale in ((dict(loss_gate = torch.tensor([-INF])), 2.0), (dict(ss = NAN), 2.0)):  # (the overflow halves 2 to 1, the min_scale clamp holds it at 2)
		ss = torch.tensor([kw.pop('ss', 1.0)], dtype = torch.float64)
		r = R.adamw_step(p, g, m, v, ss, 0.0, 1e-3, 0.9, 0.999, 1e-8, 1e-2, torch.tensor([7.0]), scaler = state, **kw)
		assert not r['applied'] and r['step_out'] == 7.0 and float(r['scaler_out'][R.LS_SCALE]) == exp_scale
		assert all(torch.equal(r[k], t.double()) for k, t in (('p', p), ('exp_avg', m), ('exp_avg_sq', v)))
	assert R.adamw_step(p, g, m, v, None, 0.0, 1e-3, 0.9, 0.999, 1e-8, 1e-2, torch.tensor([2.0 ** 24]))['step_out'] == 2.0 ** 24


# ------------------------------------------------------------------------------------------------ NovoGrad

def arena(sizes, align = 64):
	"""FlatParameters' layout: every segment starts on a multiple of `align`, the padding belongs to the segment in front of it"""
	offsets = [0]
	for s in sizes:
		offsets.append(offsets[-1] + (s + align - 1) // align * align)
	return offsets


def scatter(offsets, tensors):
	flat = torch.zeros(offsets[-1], dtype = tensors[0].dtype)
	for o, t in zip(offsets, tensors):
		flat[o:o + t.numel()] = t.flatten()
	return flat


@pytest.mark.parametrize('max_norm', [None, 1e9, 0.5])
@pytest.mark.parametrize('wd, dampening', [(0.0, False), (1e-3, False), (1e-3, True)])
def test_novograd_equals_the_oracle_float64(wd, dampening, max_norm):
	"""the oracle on float64 tensors is float64 throughout except for the clip coefficient, which it takes in fp32 in the kernel's order"""
	sizes = [5, 64, 130, 1]
	offsets = arena(sizes)
	lr, b1, b2, eps, wd = R.r32(1e-2), R.r32(0.95), R.r32(0.98), R.r32(1e-8), R.r32(wd)
	params = [rand32(s, 10 + i).double() for i, s in enumerate(sizes)]
	p, mom, ema = scatter(offsets, params), torch.zeros(offsets[-1], dtype = torch.float64), torch.zeros(len(sizes) + 1, dtype = torch.float64)
	state = {}
	for it in range(3):
		grads = [rand32(s, 100 + 10 * it + i, 0.3 * (it + 1)) for i, s in enumerate(sizes)]
		if it == 1:
			grads[1] = torch.zeros(sizes[1])  # a parameter without a gradient: its EMA decays, its update is 0 / sqrt(ema + eps)
		norm = O.novograd_step(params, [g.double() for g in grads], state, lr = lr, betas = (b1, b2), eps = eps, weight_decay = wd, dampening = dampening, max_norm = max_norm)
		r = R.novograd_step(offsets, p, scatter(offsets, grads), mom, ema, max_norm, lr, b1, b2, eps, wd, dampening, -1)
		assert r['applied'] and r['counter'] == it + 1
		p, mom, ema = r['p'], r['mom'], torch.cat([r['ema_out'], torch.tensor([r['counter']], dtype = torch.float64)])
		same(torch.tensor(r['total_norm']), norm.double(), f'norm, step {it}', 2.0 ** -24)  # (the oracle rounds its norm to fp32)
		same(r['ema_out'], torch.stack(state['ema']), f'EMAs, step {it}')
		for i, (o, s) in enumerate(zip(offsets, sizes)):
			same(p[o:o + s], params[i], f'parameter {i}, step {it}')
			same(mom[o:o + s], state['mom'][i], f'momentum {i}, step {it}')
		assert not p[offsets[0] + sizes[0]:offsets[1]].any(), 'the padding stays zero'


def test_novograd_matches_the_reference_golden():
	"""tests/golden/novograd.npz: the reference's own fp32 run, 4 steps, two hyper-parameter sets, at the bars tests/test_oracle_golden.py holds
	the oracle to; every step starts from the golden's state before it"""
	g = np.load(os.path.join(GOLDEN, 'novograd.npz'))
	for case in (0, 1):
		lr, b1, b2, eps, wd, damp, max_norm = [float(v) for v in g[f'c{case}/hyper']]
		n = len([k for k in g.files if k.startswith(f'c{case}/p0/')])
		T_ = lambda k: [torch.from_numpy(g[f'c{case}/{k}/{i}']) for i in range(n)]
		offsets = arena([t.numel() for t in T_('p0')])
		mom = torch.zeros(offsets[-1], dtype = torch.float64)
		for step in range(4):
			ema = torch.zeros(n) if step == 0 else torch.stack([e.reshape(()) for e in T_(f'ema{step}')])
			r = R.novograd_step(offsets, scatter(offsets, T_(f'p{step}')), scatter(offsets, T_(f'g{step}')), mom, ema, max_norm, lr, b1, b2, eps, wd, bool(damp), int(step == 0))
			mom = r['mom']
			assert abs(r['total_norm'] - float(g[f'c{case}/norm{step}'])) <= 1e-5 * r['total_norm']
			np.testing.assert_allclose(r['ema_out'].numpy(), np.array([float(e) for e in T_(f'ema{step + 1}')]), rtol = 2e-5)
			np.testing.assert_allclose(r['p'].numpy(), scatter(offsets, T_(f'p{step + 1}')).numpy(), rtol = 2e-5, atol = 2e-6)


def test_novograd_first_flag_grad_scale_empty_segment_and_skipped_steps():
	offsets = [0, 64, 64, 200, 200]  # segments 1 and 3 are empty
	n = offsets[-1]
	p, g, mom = rand32(n, 1), rand32(n, 2), rand32(n, 3)
	ema = torch.tensor([0.5, 0.25, 2.0, 0.125, 5.0])  # (counter 5 behind the four EMAs)
	args = (0.5, 1e-2, 0.95, 0.98, 1e-8, 1e-3, False)
	by_counter, by_flag = R.novograd_step(offsets, p, g, mom, ema, *args, -1), R.novograd_step(offsets, p, g, mom, ema[:4], *args, 0)
	assert by_counter['counter'] == 6.0 and by_flag['counter'] is None
	same(by_counter['p'], by_flag['p'], 'first = -1 with counter 5 is first = 0', 0)
	same(by_counter['ema_out'][[1, 3]], torch.tensor([0.25, 0.125]).double() * R.r32(0.98), 'an empty segment: g2 = 0, its EMA decays', 1e-15)
	ema0 = ema.clone()
	ema0[4] = 0.0
	fresh, flag1 = R.novograd_step(offsets, p, g, mom, ema0, *args, -1), R.novograd_step(offsets, p, g, mom, ema[:4], *args, 1)
	assert fresh['counter'] == 1.0
	same(fresh['p'], flag1['p'], 'first = -1 with counter 0 is first = 1', 0)
	same(fresh['ema_out'][[1, 3]], torch.zeros(2), 'first step, empty segment', 0)
	scaled = R.novograd_step(offsets, p, g * 4, mom, ema, 0.5, 1e-2, 0.95, 0.98, 1e-8, 1e-3, False, -1, grad_scale = 0.25)
	for k in ('p', 'mom', 'ema_out'):
		same(scaled[k], by_counter[k], k + ' (grad_scale)', 1e-15)
	assert scaled['total_norm'] == by_counter['total_norm']
	state = R.scaler_state(4.0, 2, unskipped = 1.0, max_scale = 4.0)
	bad = g.clone()
	bad[70] = INF
	for r, exp in ((R.novograd_step(offsets, p, g, mom, ema, *args, -1, loss_gate = torch.tensor([INF]), scaler = state), state.tolist()),
	               (R.novograd_step(offsets, p, bad, mom, ema, *args, -1, scaler = state), [2.0, 0.0, 1.0, 2.0, 0.0, 4.0, 2.0, 1.0])):
		assert not r['applied'] and r['counter'] == 5.0 and torch.equal(r['ema_out'], ema[:4].double()) and torch.equal(r['p'], p.double()) and torch.equal(r['mom'], mom.double())
		assert r['scaler_out'].tolist() == exp
	clean = R.novograd_step(offsets, p, g * 4, mom, ema, *args, -1, scaler = state)
	assert clean['applied'] and clean['scaler_out'].tolist() == [4.0, 0.0, 0.0, 2.0, 0.0, 4.0, 2.0, 0.0], 'the window closes: 4 x 2 clamped at max_scale 4'
	same(clean['p'], by_counter['p'], 'loss scale 4 on 4 x the gradient', 1e-15)


# ------------------------------------------------------------------------------------------------ loss scaler

@pytest.mark.parametrize('init, window, min_scale, max_scale', [(2.0 ** 10, 3, None, 2.0 ** 12), (2.0 ** 3, 2, 2.0, 2.0 ** 24), (2.0 ** 16, 1, None, 2.0 ** 16), (1.5, 4, 1.0, 5.0)])
def test_loss_scaler_follows_apex_update_scale(init, window, min_scale, max_scale):
	"""a random overflow / clean / gated sequence: scale and unskipped follow apex step for step (apex never sees a gated step: the reference
	skips backward then), the overflow flag names the last verdict, skipped_steps counts the overflows"""
	apex = ApexLossScaler(init = init, window = window, min_scale = min_scale, max_scale = max_scale)
	state = R.scaler_state(init, window, min_scale = min_scale or 0.0, max_scale = max_scale)
	rng = np.random.RandomState(window)
	skipped = 0
	for ev in rng.choice(['clean', 'overflow', 'gated'], size = 200, p = [0.6, 0.25, 0.15]):
		nxt = R.loss_scale_advance(state, ev == 'overflow', ev == 'gated')
		if ev == 'gated':
			assert torch.equal(nxt, state)
		else:
			apex.update(ev == 'overflow')
			skipped += ev == 'overflow'
			assert nxt.tolist() == [apex.scale, float(apex.unskipped), float(ev == 'overflow'), float(window), min_scale or 0.0, max_scale, 2.0, float(skipped)], (ev, nxt.tolist())
		state = nxt


def test_static_loss_scale_never_moves():
	state = R.scaler_state(128.0, 0)
	for overflow, gated in ((False, False), (True, False), (False, True)):
		out = R.loss_scale_advance(state, overflow, gated).tolist()
		assert out[R.LS_SCALE] == 128.0 and out[R.LS_UNSKIPPED] == 0.0 and out[R.LS_SKIPPED_STEPS] == 0.0
