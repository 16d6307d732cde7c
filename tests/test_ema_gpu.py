"""The weight average on the MI355X: convasr_ema_update and convasr_swap (convasr_amd/csrc/ema.hip) against the float64 restatement
tests/_ema_ref.py (itself held to the closed form in tests/test_ema_ref.py), and train.WeightEMA through a small Wav2Letter.

Kernel bar: after m updates from k = 0 every element is within m x 2^-23 x max(|w|, |e|) of the restatement, the max taken over the values
the element saw (its weights and its averages so far).  The update rounds twice, the difference and the fused multiply-add, at most 2^-24
relative to the larger operand each; the first update copies and is exact.  The bar is purely relative, so where fp32 rounds on the
SUBNORMAL grid (2^-150 absolute) it cannot hold: the subnormal inputs are therefore elements whose weight stays the same subnormal over the
five updates (exact: the difference is zero -- a kernel that flushed them would miss by the whole value) and subnormal weights that alternate
with normal ones (the element's max is the normal one).  Exact quantities are compared bit for bit: the mirror against torch's rounding of the
fp32 average the kernel wrote, everything a skipped update leaves alone, the counter, a second run, the swaps.

Sizes: 64 and 128 elements (the arena's granule), one granule below / at / above the span one workgroup covers per grid pass
(convasr_ema_update_span), and one granule more than max_blocks x span, where the grid loops."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ema_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

INF, NAN = float('inf'), float('nan')
HALF = dict(bf16 = torch.bfloat16, f16 = torch.float16)
UPDATES = 5
# ONE update from an average that is already off the weights (k > 0), as the skip tests make: the difference of operands of opposite sign is up
# to twice the larger one, so its rounding is up to 2^-23 of it, times 1 - d <= 1; the fused multiply-add adds 2^-24 of the result: 1.5 x 2^-23.
# (From k = 0 the first update is exact, which is why m updates stay inside m x 2^-23.)
ONE_UPDATE = 1.5 * 2.0 ** -23


def dev():
	return torch.device('cuda:0')


def bits(t):
	t = t.detach().cpu().contiguous()
	return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b, what):
	assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
	assert torch.equal(bits(a), bits(b)), f'{what}: {int((bits(a) != bits(b)).sum())} of {a.numel()} elements differ'


def geometry():
	from convasr_amd import _lib
	lib = _lib.load()
	return int(lib.convasr_ema_update_span()), int(lib.convasr_ema_update_max_blocks()), int(lib.convasr_swap_span_bytes())


def weights_sequence(n, seed):
	"""UPDATES fp32 weight vectors of n elements: magnitudes 1e-3 .. 1e4 of both signs, zeros, subnormals (see the module docstring)."""
	rng = np.random.default_rng(seed)
	scale = rng.choice(np.array([1e-3, 1.0, 30.0, 1e4], dtype = np.float32), size = n)
	ws = [(rng.standard_normal(n).astype(np.float32) * scale) for _ in range(UPDATES)]
	idx = np.arange(n)
	for j, w in enumerate(ws):  # (where two rules meet the later one holds, in every update alike)
		w[idx % 7 == 0] = 0.0 if j % 2 == 0 else w[idx % 7 == 0]  # zeros alternating with values
		w[idx % 11 == 3] = 0.0                                      # always zero
		w[idx % 13 == 5] = np.float32(1e-40) * (1 + (idx[idx % 13 == 5] % 5)).astype(np.float32)  # the same subnormal in every update
		w[idx % 19 == 1] = np.float32(1e4) * (1 if j % 2 == 0 else -1)  # the largest magnitude, changing sign
		w[idx % 17 == 9] = np.float32(2.5) if j % 2 == 0 else np.float32(-3e-41)  # a subnormal alternating with a normal value
	return ws


def run_updates(ws, decay, mirror, k0 = 0, e0 = None):
	"""The sequence on the device through ops.ema_update, the counter rows swapped by hand.  Returns per update (e fp32, mirror or None, k)."""
	from convasr_amd import ops
	d = dev()
	n = ws[0].size
	e = torch.zeros(n, dtype = torch.float32, device = d) if e0 is None else torch.from_numpy(e0.copy()).to(d)
	e16 = None if mirror is None else torch.zeros(n, dtype = HALF[mirror], device = d)
	count = torch.tensor([[float(k0)], [-1.0]], dtype = torch.float32, device = d)
	cur, out = 0, []
	for w in ws:
		ops.ema_update(torch.from_numpy(w).to(d), e, decay, count[cur], count[1 - cur], e16 = e16)
		cur = 1 - cur
		out.append((e.clone(), None if e16 is None else e16.clone(), float(count[cur, 0])))
	torch.cuda.synchronize()
	return out


def check_against_restatement(ws, got, decay, mirror, what):
	n = ws[0].size
	e, k = np.zeros(n), 0
	seen = np.zeros(n)
	worst = 0.0
	for m, (w, (ge, g16, gk)) in enumerate(zip(ws, got), start = 1):
		seen = np.maximum(seen, np.maximum(np.abs(w.astype(np.float64)), np.abs(e)))
		e, k = R.update(w, e, k, decay)
		seen = np.maximum(seen, np.abs(e))
		assert gk == k, (what, m, gk, k)
		err = np.abs(ge.cpu().numpy().astype(np.float64) - e)
		tol = m * 2.0 ** -23 * seen
		bad = err > tol
		with np.errstate(divide = 'ignore', invalid = 'ignore'):
			worst = max(worst, float(np.nanmax(np.where(tol > 0, err / tol, 0.0))))
		assert not bad.any(), f'{what}: update {m}: {int(bad.sum())} elements beyond m 2^-23 max; worst err {err[bad].max():.3e} at tol {tol[bad][err[bad].argmax()]:.3e}'
		if mirror is not None:
			same_bits(g16, ge.to(HALF[mirror]), f'{what}: mirror after update {m}')
			exp = torch.from_numpy(R.mirror_bits(ge.cpu().numpy(), mirror).view(np.int16).copy())
			nan = torch.isnan(ge.cpu())
			assert torch.equal(bits(g16)[~nan], exp[~nan]), f'{what}: mirror against the restatement after update {m}'
	print(f'    EMA {what}: worst share of the m 2^-23 max bar {worst:.3f}')


def sizes():
	span, max_blocks, _ = geometry()
	return [64, 128, span - 64, span, span + 64, max_blocks * span + 64]


@pytest.mark.parametrize('mirror', [None, 'bf16', 'f16'])
def test_ema_update_matches_restatement_at_every_size(mirror):
	for n in sizes():
		ws = weights_sequence(n, seed = n % 1000 + 1)
		got = run_updates(ws, 0.999, mirror)
		check_against_restatement(ws, got, 0.999, mirror, f'n {n} mirror {mirror}')
		again = run_updates(ws, 0.999, mirror)
		for (a, a16, ak), (b, b16, bk) in zip(got, again):
			same_bits(a, b, f'n {n}: second run')
			assert ak == bk
			if mirror is not None:
				same_bits(a16, b16, f'n {n}: second run, mirror')
	# the first update is a copy, the counter counts, and a subnormal weight is not flushed
	ws = weights_sequence(128, seed = 3)
	got = run_updates(ws, 0.999, mirror)
	same_bits(got[0][0], torch.from_numpy(ws[0]), 'first update')
	assert [g[2] for g in got] == [1.0, 2.0, 3.0, 4.0, 5.0]
	assert float(got[-1][0][5]) == float(np.float32(1e-40)) != 0.0


@pytest.mark.parametrize('decay', [0.0, 0.15, 1.0])
def test_ema_update_decay_cap(decay):
	"""decay 0: the average is the weights after every update; 0.15: the cap binds from k = 1 on; 1: the warm-up schedule alone."""
	span, _, _ = geometry()
	for n in (128, span + 64):
		ws = weights_sequence(n, seed = 40 + n % 7)
		got = run_updates(ws, decay, 'bf16')
		check_against_restatement(ws, got, decay, 'bf16', f'n {n} decay {decay}')


def test_ema_update_refuses_bad_arguments_before_any_launch():
	from convasr_amd import ops, _lib
	d = dev()
	w, e, k = torch.zeros(64, device = d), torch.zeros(64, device = d), torch.zeros(2, 1, device = d)
	with pytest.raises(_lib.ConvasrHipError):
		ops.ema_update(w, e, 1.5, k[0], k[1])
	with pytest.raises(_lib.ConvasrHipError):
		ops.ema_update(w, w, 0.9, k[0], k[1])
	with pytest.raises(_lib.ConvasrHipError):
		ops.ema_update(w[:60], e[:60], 0.9, k[0], k[1])
	with pytest.raises(_lib.ConvasrHipError):
		ops.ema_update(w.cpu(), e, 0.9, k[0], k[1])
	with pytest.raises(_lib.ConvasrHipError):
		ops.swap_(w, w)
	with pytest.raises(_lib.ConvasrHipError):
		ops.swap_(w[:34], w[30:])
	torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ skip

def scaler_row(overflow):
	"""A loss scaler's state the documented way (include/convasr_hip.h: [0] scale ... [2] did the last step overflow ...)."""
	return torch.tensor([65536.0, 3.0, 1.0 if overflow else 0.0, 2000.0, 0.0, 2.0 ** 24, 2.0, 1.0], dtype = torch.float32)


@pytest.mark.parametrize('mirror', ['bf16', 'f16'])
def test_skipped_update_changes_nothing_and_the_next_one_uses_the_same_k(mirror):
	from convasr_amd import ops
	d = dev()
	span, _, _ = geometry()
	n = span + 64
	ws = weights_sequence(n, seed = 77)
	cases = [dict(loss_gate = NAN), dict(loss_gate = INF), dict(loss_gate = -INF), dict(scaler_state = scaler_row(True)), dict(loss_gate = 1.5, scaler_state = scaler_row(True)),
	         dict(loss_gate = NAN, scaler_state = scaler_row(False))]
	for k0 in (0, 2):
		for kw in cases:
			e_host = ws[1].copy()
			e = torch.from_numpy(e_host).to(d)
			e16 = torch.from_numpy(ws[2]).to(d).to(HALF[mirror])  # (deliberately NOT the rounded average: a skip must not rewrite it)
			e16_0 = e16.clone()
			count = torch.tensor([[float(k0)], [-7.0]], dtype = torch.float32, device = d)
			args = {k: (torch.tensor([v], dtype = torch.float32, device = d) if k == 'loss_gate' else v.to(d)) for k, v in kw.items()}
			assert R.skipped(kw.get('loss_gate'), None if 'scaler_state' not in kw else kw['scaler_state'].numpy())
			ops.ema_update(torch.from_numpy(ws[0]).to(d), e, 0.999, count[0], count[1], e16 = e16, **args)
			same_bits(e, torch.from_numpy(e_host), f'skip {kw} k0 {k0}: average')
			same_bits(e16, e16_0, f'skip {kw} k0 {k0}: mirror')
			assert count[:, 0].tolist() == [float(k0), float(k0)], (kw, count)  # the row the launch writes carries the un-advanced counter
			# the next update, from the row the skipped launch wrote: the update that would have come without the skip
			clean = dict(loss_gate = torch.tensor([0.25], dtype = torch.float32, device = d), scaler_state = scaler_row(False).to(d))
			ops.ema_update(torch.from_numpy(ws[0]).to(d), e, 0.999, count[1], count[0], e16 = e16, **clean)
			ref, k1 = R.update(ws[0], e_host.astype(np.float64), k0, 0.999)
			assert float(count[0, 0]) == k1 == k0 + 1
			err = np.abs(e.cpu().numpy().astype(np.float64) - ref)
			assert (err <= ONE_UPDATE * np.maximum(np.abs(ws[0]), np.maximum(np.abs(e_host), np.abs(ref)))).all()
			same_bits(e16, e.to(HALF[mirror]), 'mirror after the update that followed the skip')


class _Tiny(torch.nn.Module):
	def __init__(self):
		super().__init__()
		self.a = torch.nn.Parameter(torch.randn(40, 30, generator = torch.Generator().manual_seed(1)))
		self.b = torch.nn.Parameter(torch.randn(70, generator = torch.Generator().manual_seed(2)))


@pytest.mark.parametrize('optname', ['sgd', 'adamw', 'novograd'])
def test_weight_ema_skips_the_step_a_loss_scaler_skipped(optname):
	"""A real optimizer step under a dynamic loss scaler with an inf planted in the gradient: the optimizer skips it on the device and records
	the overflow in the scaler state it writes; WeightEMA.update reads it there and changes nothing.  The clean step after it is averaged with
	the un-advanced counter."""
	import convasr_amd as ca
	d = dev()
	model = _Tiny().to(d)
	flat = ca.train.FlatParameters(model)
	flat.mirror(torch.float16)
	opt = dict(sgd = lambda: ca.train.SGD(flat, lr = 0.1, momentum = 0.9, weight_decay = 0.0), adamw = lambda: ca.optimizers.AdamW(flat, lr = 0.1),
	           novograd = lambda: ca.optimizers.NovoGrad(flat, lr = 0.1))[optname]()
	flat.loss_scaler = ca.train.LossScaler(d, init_scale = 1024.0)
	ema = ca.train.WeightEMA(flat, decay = 0.5)
	assert ema.average16 is not None and ema.average16.dtype == torch.float16
	gen = torch.Generator().manual_seed(9)

	def step(plant):
		for p in flat.params:  # gradients of the SCALED loss, written by hand (the arena's padding keeps its zeros)
			p._convasr_grad.copy_((torch.randn(p.shape, generator = gen) * 1024.0).to(d))
			p._convasr_fresh = False
		if plant:
			flat.params[0]._convasr_grad[0, 5] = INF
		opt.step()
		ema.update()
		opt.zero_grad()

	step(False)
	step(False)
	assert ema.updates == 2 and flat.loss_scaler.current[R.LS_OVERFLOW] == 0
	avg, avg16, w = ema.average.clone(), ema.average16.clone(), flat.data.clone()
	step(True)
	assert flat.loss_scaler.current[R.LS_OVERFLOW] == 1 and flat.loss_scaler.loss_scale() == 512.0
	same_bits(flat.data, w, 'the optimizer skipped the overflowed step')
	same_bits(ema.average, avg, 'average after the overflowed step')
	same_bits(ema.average16, avg16, 'mirror after the overflowed step')
	assert ema.updates == 2
	step(False)
	assert ema.updates == 3 and flat.loss_scaler.current[R.LS_OVERFLOW] == 0 and not torch.equal(flat.data, w)
	ref, _ = R.update(flat.data.cpu().numpy(), avg.cpu().numpy().astype(np.float64), 2, 0.5)
	err = np.abs(ema.average.cpu().numpy().astype(np.float64) - ref)
	assert (err <= ONE_UPDATE * np.maximum(np.abs(ref), np.maximum(np.abs(avg.cpu().numpy()), np.abs(flat.data.cpu().numpy())))).all()
	same_bits(ema.average16, ema.average.to(torch.float16), 'mirror')
	# a non-finite loss gate, the other device-side skip
	gate = torch.tensor([NAN], device = d)
	avg = ema.average.clone()
	ema.update(loss_gate = gate)
	same_bits(ema.average, avg, 'gated update')
	assert ema.updates == 3


# ------------------------------------------------------------------------------------------------ swap

@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
def test_swap_exchanges_contents_in_place(dtype):
	from convasr_amd import ops
	d = dev()
	_, _, span_bytes = geometry()
	per = span_bytes // torch.empty(0, dtype = dtype).element_size()
	for n in (64, per + 64, 3 * per - 64, 2048 * per + 64):  # 64 elements; not a multiple of the span; beyond the largest grid
		g = torch.Generator().manual_seed(n % 97)
		a0, b0 = torch.randn(n, generator = g).to(dtype), torch.randn(n, generator = g).to(dtype)
		a0[0], b0[-1] = NAN, INF
		pad = 64
		abuf, bbuf = torch.full((n + 2 * pad, ), 7.0, dtype = dtype, device = d), torch.full((n + 2 * pad, ), -7.0, dtype = dtype, device = d)
		a, b = abuf[pad:pad + n], bbuf[pad:pad + n]
		a.copy_(a0)
		b.copy_(b0)
		pa, pb = a.data_ptr(), b.data_ptr()
		ops.swap_(a, b)
		same_bits(a, b0, f'swap n {n}: a')
		same_bits(b, a0, f'swap n {n}: b')
		ops.swap_(b, a)  # the other direction restores both
		same_bits(a, a0, f'swap back n {n}: a')
		same_bits(b, b0, f'swap back n {n}: b')
		ops.swap_(a, b)
		ops.swap_(a, b)
		same_bits(a, a0, f'two swaps n {n}: a')
		same_bits(b, b0, f'two swaps n {n}: b')
		assert (a.data_ptr(), b.data_ptr()) == (pa, pb)
		for buf, v in ((abuf, 7.0), (bbuf, -7.0)):  # nothing outside the two ranges was written
			assert bool((buf[:pad] == v).all()) and bool((buf[pad + n:] == v).all())


# ------------------------------------------------------------------------------------------------ model level

COMBOS = [(dt, o) for dt in ('bf16', 'fp32') for o in ('sgd', 'novograd')]
DTYPES = dict(bf16 = torch.bfloat16, fp32 = torch.float32)


def _model(ca, dt, seed = 3):
	torch.manual_seed(seed)
	fe = ca.models.LogFilterBankFrontend(64, 16000, 0.02, 0.01, 'hann_window')
	return ca.models.Wav2Letter(64, [38], frontend = fe, dropout = 0, base_width = 128, check_time_dim_padded = False, compute_dtype = DTYPES[dt]).to(dev()).train()


def _optimizer(ca, flat, name):
	if name == 'sgd':
		return ca.train.SGD(flat, lr = 1e-2, momentum = 0.9, weight_decay = 1e-3)
	return ca.optimizers.NovoGrad(flat, lr = 1e-2, betas = (0.95, 0.98), weight_decay = 1e-3)


def _batches(n):
	g = torch.Generator().manual_seed(5)
	out = []
	for _ in range(n):
		x = torch.rand(2, 16000, generator = g) * 2 - 1
		xlen = torch.tensor([1.0, 0.8])
		y = torch.randint(0, 37, (2, 1, 8), generator = g)
		ylen = torch.tensor([[8], [5]])
		out.append(tuple(t.to(dev()) for t in (x, xlen, y, ylen)))
	return out


def _setup(ca, dt, optname, decay = 0.999):
	ca.functional.manual_seed(17)
	model = _model(ca, dt)
	flat = ca.train.FlatParameters(model)
	opt = _optimizer(ca, flat, optname)
	return model, flat, opt, ca.train.WeightEMA(flat, decay = decay)


def _eval_logits(model, batch):
	model.eval()
	try:
		with torch.no_grad():
			out = model(batch[0], batch[1], y = batch[2], ylen = batch[3])
	finally:
		model.train()
	return out['logits'][0].clone(), out['log_probs'][0].clone()


@pytest.mark.parametrize('dt,optname', COMBOS)
def test_weight_ema_through_training_evaluation_and_checkpoint(dt, optname):
	import convasr_amd as ca
	from convasr_amd import _lib
	batches = _batches(4)
	model, flat, opt, ema = _setup(ca, dt, optname)
	assert (flat.data16 is None) == (ema.average16 is None)
	snaps, losses = [], []
	for it in range(3):
		losses.append(float(ca.train.train_step(model, opt, *batches[it], iteration = it, ema = ema)['loss']))
		snaps.append([t.cpu().numpy() for t in flat.export_state(flat.data)])
	# Average: the restatement over the parameter snapshots
	sd = ema.state_dict()
	assert sd['updates'] == 3 and sd['decay'] == 0.999 and len(sd['average']) == len(flat.params)
	for i, (p, got) in enumerate(zip(flat.params, sd['average'])):
		assert tuple(got.shape) == tuple(p.shape) and got.is_contiguous()
		e, k, seen = np.zeros(p.shape), 0, np.zeros(p.shape)
		for snap in snaps:
			seen = np.maximum(seen, np.maximum(np.abs(snap[i].astype(np.float64)), np.abs(e)))
			e, k = R.update(snap[i], e, k, 0.999)
			seen = np.maximum(seen, np.abs(e))
		assert (np.abs(got.cpu().numpy().astype(np.float64) - e) <= 3 * 2.0 ** -23 * seen).all(), f'parameter {i}'
	if dt == 'bf16':
		assert flat.data16 is not None and ema.average16 is not None
		same_bits(ema.average16, ema.average.to(torch.bfloat16), 'the average\'s mirror')
	assert not torch.equal(ema.average, flat.data)
	# Evaluation: a second model holding the average as ordinary parameters, and this model's buffers
	other = _model(ca, dt, seed = 11)
	with torch.no_grad():
		for p, t in zip([p for p in other.parameters() if p.requires_grad], sd['average']):
			p.copy_(t)
		for b, src in zip(other.buffers(), model.buffers()):
			b.copy_(src)
	expected = _eval_logits(other, batches[3])
	before = _eval_logits(model, batches[3])
	raw, raw16, ptr = flat.data.clone(), None if flat.data16 is None else flat.data16.clone(), flat.data.data_ptr()
	with ema.average_parameters():
		inside = _eval_logits(model, batches[3])
		assert flat.data.data_ptr() == ptr
		same_bits(flat.data, sd_flat(flat, sd), 'the arena inside the context')
		# Guards
		with pytest.raises(_lib.ConvasrHipError):
			opt.step()
		with pytest.raises(_lib.ConvasrHipError):
			ema.update()
		with pytest.raises(_lib.ConvasrHipError):
			ema.copy_to()
		with pytest.raises(_lib.ConvasrHipError):
			with ema.average_parameters():
				pass
		assert all(torch.equal(a, b) for a, b in zip(ema.state_dict()['average'], sd['average']))  # (the average is still what state_dict exports)
	same_bits(inside[0], expected[0], 'logits inside the context')
	same_bits(inside[1], expected[1], 'log-probs inside the context')
	assert not torch.equal(inside[0], before[0])
	# Restore: also after an exception
	same_bits(flat.data, raw, 'the arena after the context')
	if raw16 is not None:
		same_bits(flat.data16, raw16, 'the mirror after the context')
	same_bits(_eval_logits(model, batches[3])[0], before[0], 'logits after the context')
	with pytest.raises(ZeroDivisionError):
		with ema.average_parameters():
			1 / 0
	assert flat.averaged is None
	same_bits(flat.data, raw, 'the arena after a context that raised')
	same_bits(_eval_logits(model, batches[3])[0], before[0], 'logits after a context that raised')
	# Training continues: the fourth step against a run that never entered the context
	loss4 = float(ca.train.train_step(model, opt, *batches[3], iteration = 3, ema = ema)['loss'])
	m2, f2, o2, e2 = _setup(ca, dt, optname)
	l2 = [float(ca.train.train_step(m2, o2, *batches[it], iteration = it, ema = e2)['loss']) for it in range(4)]
	assert losses + [loss4] == l2, (losses + [loss4], l2)
	same_bits(flat.data, f2.data, 'parameters after the fourth step')
	same_bits(ema.average, e2.average, 'average after the fourth step')
	assert ema.updates == e2.updates == 4
	# Checkpoint: a fresh WeightEMA restores the average, the counter and the next update's result
	e3 = ca.train.WeightEMA(flat, decay = 0.5)
	e3.load_state_dict(ema.state_dict())
	assert e3.decay == 0.999 and e3.updates == 4
	same_bits(e3.average, ema.average, 'restored average')
	if ema.average16 is not None:
		same_bits(e3.average16, ema.average16, 'restored mirror')
	flat.data.mul_(1.01)  # (any change of the weights: both averages see the same ones)
	ema.update()
	e3.update()
	same_bits(e3.average, ema.average, 'the update after the restore')
	assert e3.updates == ema.updates == 5
	# copy_to: the parameters ARE the average, for good
	ema.copy_to()
	same_bits(flat.data, ema.average, 'copy_to')
	if flat.data16 is not None:
		same_bits(flat.data16, ema.average16, 'copy_to, mirror')
	final = _eval_logits(model, batches[3])[0]
	with ema.average_parameters():
		same_bits(_eval_logits(model, batches[3])[0], final, 'after copy_to the context changes nothing')
	torch.cuda.synchronize()


def sd_flat(flat, sd):
	"""The exported average put back into arena order (what the arena must hold inside the context)."""
	out = torch.zeros_like(flat.data)
	flat.import_state(out, sd['average'], 'test')
	return out


@pytest.mark.parametrize('dt,optname', COMBOS)
def test_weight_ema_in_step_graphs_is_bitwise_the_eager_average(dt, optname):
	import convasr_amd as ca
	from convasr_amd import _lib
	batches = _batches(2)
	runs = {}
	for graphed in (False, True):
		model, flat, opt, ema = _setup(ca, dt, optname)
		stepper = ca.train.GraphedTrainStep(model, opt, warmup = 1, enabled = graphed, ema = ema)
		losses = [float(stepper(*batches[it % 2], iteration = it)['loss']) for it in range(6)]
		torch.cuda.synchronize()
		runs[graphed] = (losses, flat.data.clone(), ema.average.clone(), None if ema.average16 is None else ema.average16.clone(), ema.updates, stepper)
		if graphed:
			assert stepper.captures == 1 and stepper.replays == 5, (stepper.captures, stepper.replays)
			assert not stepper.non_kernel_nodes
			for g in stepper.graphs.values():
				assert g['node_kinds'] is not None and set(g['node_kinds']) == {'kernel'}, g['node_kinds']
			with ema.average_parameters():  # Guards: a replay inside the context
				with pytest.raises(_lib.ConvasrHipError):
					stepper(*batches[0], iteration = 6)
			assert stepper.replays == 5 and ema.updates == 6
			same_bits(flat.data, runs[True][1], 'the refused replay changed nothing')
	eager, graph = runs[False], runs[True]
	assert eager[0] == graph[0], (eager[0], graph[0])
	same_bits(eager[1], graph[1], 'parameters')
	same_bits(eager[2], graph[2], 'averages')
	if eager[3] is not None:
		same_bits(eager[3], graph[3], 'mirrors of the averages')
	assert eager[4] == graph[4] == 6
	assert not torch.equal(eager[2], eager[1])


def test_evaluate_model_with_ema_scores_the_averaged_weights():
	"""train.evaluate_model(..., ema = ema) is evaluate_model on a model that holds the average; without ema it is what it was."""
	import convasr_amd as ca
	batches = _batches(3)
	model, flat, opt, ema = _setup(ca, 'bf16', 'sgd', decay = 0.5)
	for it in range(3):
		ca.train.train_step(model, opt, *batches[it], iteration = it, ema = ema)
	from convasr_amd.transcript_generators import CharTokenizerLegacy
	tok = CharTokenizerLegacy('абвгдеёжзийклмнопрстуфхцчшщъыьэюя')
	val = [([{}] * 2, None) + batches[0]]
	raw = ca.train.evaluate_model(model, val, tok)
	w = flat.data.clone()
	avg = ca.train.evaluate_model(model, val, tok, ema = ema)
	same_bits(flat.data, w, 'parameters after the averaged validation pass')
	assert model.training and flat.averaged is None
	with ema.average_parameters():
		inside = ca.train.evaluate_model(model, val, tok)
	assert torch.equal(avg['utterances']['loss'], inside['utterances']['loss']) and avg['cer'] == inside['cer']
	assert not torch.equal(avg['utterances']['loss'], raw['utterances']['loss'])
	again = ca.train.evaluate_model(model, val, tok)
	assert torch.equal(again['utterances']['loss'], raw['utterances']['loss'])
