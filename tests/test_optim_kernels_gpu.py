"""The fused optimizer tail on the MI355X -- sumsq, sgd_step, adamw_step (convasr_amd/csrc/misc.hip), novograd_step (csrc/next.hip) and the loss
scaler they advance (csrc/common.h) -- against the float64 restatement tests/_optim_ref.py (itself held to torch.optim in float64, the oracle,
the golden and apex's update_scale() in tests/test_optim_ref.py), at the sizes where each kernel takes another path: the float4 body and the
n & 3 tail, fewer elements than one float4, the launch caps that turn sumsq (2048 x 1024) and the steps (4096 x 1024) into grid-stride loops,
and for NovoGrad the NG_CHUNK (8192) a workgroup owns, segment boundaries on, before and behind a chunk edge, segments cut into several
NG_ITEM (65536) items, the NG_TABLE (2048) limit of the offsets staged in LDS, more than 256 segments in one chunk, and empty segments.

Protocol: before every launch the device's own fp32 state (p, momentum / moments, EMAs, counter) is copied to the host and the reference
starts from it, so one step's arithmetic is compared, not accumulated drift; one three-step trajectory per optimizer on top keeps its own
float64 state.  The sum of squares sgd_step / adamw_step clip by is the device's own fp64 buffer (the launch's input), so the fp32 clip factor
of the reference is the kernel's, bit for bit; NovoGrad's is taken from the reference's own float64 per-segment sums.

Exact quantities are compared bit for bit: the 16-bit mirror (= the fp32 result rounded once by torch; its subnormals, ties and overflow in
test_mirror_rounding_edges, with lr = 0 so that the planted values ARE the fp32 result), everything a gated or overflowed
step leaves alone, the scaler's eight floats, the applied-step counters, `buf` with zero momentum, and a second launch on the same inputs.
fp32 arithmetic is compared over every element against atol + rtol |ref| with (rtol, atol) = SHARE[quantity] x the project's bar for that
quantity (PROJECT).  SHARE is 4x the worst share measured on the MI355X over every check of the quantity in this file, and never above 1
(the measured values are next to the constants).  Every check prints what it measured next to its bar, and next to what torch's own fp32
CPU optimizer scores against the same float64 where there is one; the table is in profiles/NOTEBOOK.md, section 16.

Empty segments: FlatParameters accepts a trainable parameter with numel() == 0, which becomes a zero-length segment at the offset of its
successor -- on a chunk edge or at the arena's end whenever the sizes in front of it add up to one.  ng_step_kernel used to leave the
ema_out of such a segment unwritten (no element finds it); it publishes them now, and layout 'f' and
test_classes_accept_a_parameter_without_elements hold it to that."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _optim_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

INF, NAN = float('inf'), float('nan')
HALF = dict(bf16 = torch.bfloat16, f16 = torch.float16)
U32 = 2.0 ** -24  # unit roundoff of fp32

# (rtol, atol) each quantity may never exceed: the bar the project already holds it to --
#   SGD parameters and momentum 1e-5 / 1e-6 (tests/test_kernels_gpu.py::test_sumsq_and_sgd_step_match_torch), AdamW parameters 2e-6 / 1e-7 and
#   moments 1e-5 / 1e-8, 1e-5 / 1e-12 (tests/test_training_features_gpu.py), NovoGrad parameters 2e-5 / 2e-6 and EMAs 2e-5 / 0, gradient norms
#   1e-5 / 0 (tests/test_models_gpu.py::test_novograd_matches_reference_golden).
# The three without one are derived:
#   grad_out: at most ONE rounding -- one fp32 product g x clip, the reference's clip being the kernel's bit for bit: |err| <= u |ref|, and
#     below fp32's normal range half the spacing of the subnormals, 2^-150
#   ng_mom: NovoGrad's momentum is the update the parameter bar was set for, divided by lr <= 1: the parameters' bar
#   ng_g2: the per-segment sum of squares is the square of a gradient norm: twice the norms' relative bar
PROJECT = dict(norm = (1e-5, 0.0), sgd_p = (1e-5, 1e-6), sgd_buf = (1e-5, 1e-6), grad_out = (U32, 2.0 ** -150), adamw_p = (2e-6, 1e-7), exp_avg = (1e-5, 1e-8),
               exp_avg_sq = (1e-5, 1e-12), ng_p = (2e-5, 2e-6), ng_mom = (2e-5, 2e-6), ng_ema = (2e-5, 0.0), ng_g2 = (2e-5, 0.0),
               sgd_traj = (1e-5, 1e-6), adamw_traj = (2e-6, 1e-7), ng_traj = (2e-5, 2e-6))
# share of the bar above each quantity is held to = min(1, 4 x the worst share measured on the MI355X over every check of this file); the comment
# gives that measured worst share, and torch fp32 on the CPU against the same float64 where there is such an optimizer
SHARE = dict(
	norm = 0.042,        # 0.0105 measured (sumsq n 1023 with one segment x 1e4, norm_out x 0.25); torch.linalg.vector_norm in fp32 0.0194 on that input, 2.88 at worst (n 2098183)
	sgd_p = 0.023,       # 0.00567 measured (n 4195507); torch 0.00567
	sgd_buf = 0.12,      # 0.0282 measured (n 1023); torch 0.0406
	grad_out = 1.0,      # 0.9996 measured: the one rounding of the product (0.4998 of a 2 u bar, now stated as the 1 u it is); torch's fp32 product the same
	adamw_p = 1.0,       # 0.250 measured (n 4195507, t0 1, betas (0.9, 0.98): p decay and the update cancel to a result near 0, 2.5e-8 of the 1e-7); torch 0.82 there, 3.5 at worst; 0.061 / 0.037 elsewhere
	exp_avg = 1.0,       # 0.604 measured (trajectory, step 2; 0.341 in one step, n 4195507: b1 m and (1 - b1) g cancel); torch 0.73 there, 2.3 at worst
	exp_avg_sq = 0.086,  # 0.0215 measured (trajectory, step 2); torch 1.31
	ng_p = 0.012,        # 0.00283 measured (the classes' second step)
	ng_mom = 0.23,       # 0.0558 measured (layout d2047)
	ng_ema = 0.027,      # 0.00655 measured (layout e)
	ng_g2 = 0.019,       # 0.00455 measured (layout e)
	sgd_traj = 0.55,     # 0.135 measured (momentum after step 2); torch 0.166
	adamw_traj = 0.35,   # 0.0853 measured (parameters after step 2); torch 0.144
	ng_traj = 0.03,      # 0.00747 measured (parameters after step 2)
)


def dev():
	return torch.device('cuda:0')


def gen(seed):
	return torch.Generator().manual_seed(seed)


def share_of(a, b, bar):
	"""worst err / (atol + rtol |ref|) over every element; where the reference is infinite, or the bar is zero (a reference of exactly 0
	under a purely relative bar), the two must agree exactly"""
	a, b = torch.as_tensor(a, dtype = torch.float64).detach().cpu().reshape(-1), torch.as_tensor(b, dtype = torch.float64).detach().cpu().reshape(-1)
	assert a.shape == b.shape, (a.shape, b.shape)
	tol = bar[1] + bar[0] * b.abs()
	exact = torch.isinf(b) | (tol == 0)
	assert torch.equal(a[exact], b[exact]), 'entries that have to be exact (an infinite or zero reference) differ'
	assert bool(torch.isfinite(a[~exact]).all()), 'non-finite result'
	if int((~exact).sum()) == 0:
		return 0.0
	return float(((a - b)[~exact].abs() / tol[~exact]).max())


def close(key, got, ref, what, cpu32 = None):
	"""got against the float64 ref at SHARE[key] of the project's bar; cpu32: torch fp32 on the CPU, for the record"""
	proj, allowed = PROJECT[key], SHARE[key]
	s = share_of(got, ref, proj)
	note = '' if cpu32 is None else f', torch fp32 cpu {share_of(cpu32, ref, proj):.3e}'
	print(f'    OPTIM {key} {what}: measured {s:.3e} of ({proj[0]:.1e}, {proj[1]:.1e}), bar {allowed:.3e}{note}')
	assert s <= allowed, f'{key} {what}: {s:.3e} of the bar ({proj[0]:.1e}, {proj[1]:.1e}), allowed {allowed:.3e}'


def bits(t):
	t = t.detach().cpu().contiguous()
	return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(got, exp, what):
	"""bit for bit; where the expected value is NaN the result must be a NaN (any payload)"""
	got, exp = got.detach().cpu(), exp.detach().cpu()
	assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
	nan = torch.isnan(exp)
	assert torch.equal(torch.isnan(got), nan), f'{what}: NaN positions'
	got, exp = torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(exp), exp)
	bad = bits(got) != bits(exp)
	assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.flatten().nonzero()[0].item()}'


def mirror_is_the_rounded_result(p16, p, what):
	same_bits(p16, p.detach().cpu().to(p16.dtype), f'{what}: the {p16.dtype} mirror is the fp32 result rounded once')


def f64dev(v):
	return torch.tensor([v], dtype = torch.float64, device = dev())


def f32dev(v):
	return torch.tensor([v] if not isinstance(v, (list, tuple)) else v, dtype = torch.float32, device = dev())


def scaler_pair(state):
	"""(state read, state written) on the device; the written one starts as NaNs, so a float the kernel leaves out shows"""
	return (state.to(dev()), torch.full((R.LOSS_SCALER_FLOATS, ), NAN, device = dev()))


def plant_mirror_edges(p, dtype):
	"""a few parameters of unusual magnitude, where there is room.  After a step with lr ~ 1e-2 only the ones beyond fp16's largest finite
	65504 still say something about the mirror (-> inf); the small ones and the ties are moved away by the update.  The rounding edges
	themselves -- subnormals, ties, the last value below inf -- are held by test_mirror_rounding_edges, whose launches leave p where it is."""
	vals = torch.tensor([7e4, -1e5, 65520.0, 65519.0, 3e-6, -1e-7, 6e-8, 2.0 ** -25, 3.1e-8, 1.00390625])
	k = min(p.numel() // 2, vals.numel())
	if dtype is not None and k:
		p[-k:] = vals[:k]


SMALL = [1, 2, 3, 4, 5, 7, 1023, 1024, 1027]
WRAP = 4096 * 1024 + 4 * 300 + 3  # the steps' launch cap is 4096 workgroups x 256 lanes x 4 elements: one more trip for 1200 elements, and a tail


# ------------------------------------------------------------------------------------------------ sumsq

SUMSQ_WRAP = 2048 * 1024 + 4 * 257 + 3  # 2048 workgroups x 256 lanes x 4 elements, then a second trip of the loop for 257 lanes, and a tail of 3


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 1024, 1025, SUMSQ_WRAP])
def test_sumsq_sizes_norm_out_and_determinism(n):
	from convasr_amd import ops
	d = dev()
	g = torch.randn(n, generator = gen(n)) * 0.5
	variants = {'plain': g}
	if n >= 1023:
		big = g.clone()
		big[n // 3:n // 3 + max(n // 50, 1)] *= 1e4  # one segment 10^4 times larger than the rest
		variants['one segment x 1e4'] = big
	for name, x in variants.items():
		xd = x.to(d)
		ref = R.sumsq(x)
		out = ops.sumsq(xd).clone()
		close('norm', out.sqrt(), ref.sqrt(), f'n {n} {name}', cpu32 = torch.linalg.vector_norm(x))
		norm = torch.full((1, ), NAN, device = d)
		out2 = ops.sumsq(xd, norm_out = norm, norm_scale = 0.25)
		same_bits(out2, out, f'n {n} {name}: a second launch')
		close('norm', norm, R.grad_norm(ref, 0.25), f'n {n} {name} norm_out x 0.25')
		state = R.scaler_state(1024.0, 5)
		ops.sumsq(xd, norm_out = norm, norm_scale = 0.25, loss_scaler = state.to(d))
		close('norm', norm, R.grad_norm(ref, 0.25, state), f'n {n} {name} norm_out x 0.25 / loss scale 1024')


@pytest.mark.parametrize('where', ['body', 'tail'])
@pytest.mark.parametrize('value', [INF, -INF, NAN, 3e19])
def test_sumsq_non_finite_elements(value, where):
	"""an inf or NaN element gives an inf or NaN sum and norm, never a finite one -- in the float4 body and in the n & 3 tail.  3e19 is finite but
	its square (9e38) is beyond fp32: the kernel squares in fp32, so the sum is +inf -- what torch.linalg.vector_norm of an fp32 tensor returns
	too (clip_grad_norm_ in the reference), and what the loss scaler then treats as an overflow.  The float64 restatement would say 3e19; the
	kernel is pinned to fp32's answer here."""
	from convasr_amd import ops
	n = 1027
	g = torch.randn(n, generator = gen(3))
	g[{'body': 517, 'tail': n - 1}[where]] = value
	norm = torch.full((1, ), 0.0, device = dev())
	out = ops.sumsq(g.to(dev()), norm_out = norm).cpu()
	exp = torch.linalg.vector_norm(g)
	assert not bool(torch.isfinite(exp)) and not bool(torch.isfinite(out).any()) and not bool(torch.isfinite(norm).any()), (out, norm, exp)
	assert bool(torch.isnan(out).all()) == bool(torch.isnan(exp)) and bool(torch.isnan(norm).all()) == bool(torch.isnan(exp)), (out, norm, exp)


# ------------------------------------------------------------------------------------------------ sgd_step

# momentum (None: 0 without a buffer; 0.0: 0 with a buffer that must stay untouched), nesterov, first, weight decay, clip (none: max_norm 0 and no
# sumsq; inactive: a norm below max_norm; active), grad_scale, grad_out (None, a separate buffer, the gradient buffer itself), mirror, lr_dev
SGD_CASES = [
	dict(mom = None, nesterov = 0, first = 1, wd = 0.0, clip = 'none', gs = 1.0, gout = None, p16 = None, lr_dev = False),
	dict(mom = 0.0, nesterov = 0, first = 0, wd = 1e-3, clip = 'active', gs = 0.25, gout = 'separate', p16 = 'bf16', lr_dev = True),
	dict(mom = None, nesterov = 0, first = 0, wd = 1e-3, clip = 'inactive', gs = 1.0, gout = 'alias', p16 = 'f16', lr_dev = False),
	dict(mom = 0.9, nesterov = 0, first = 1, wd = 1e-3, clip = 'inactive', gs = 1.0, gout = 'alias', p16 = 'f16', lr_dev = False),
	dict(mom = 0.9, nesterov = 0, first = 0, wd = 0.0, clip = 'active', gs = 1.0, gout = 'alias', p16 = None, lr_dev = False),
	dict(mom = 0.9, nesterov = 1, first = 1, wd = 1e-3, clip = 'active', gs = 0.25, gout = 'separate', p16 = 'f16', lr_dev = True),
	dict(mom = 0.9, nesterov = 1, first = 0, wd = 1e-3, clip = 'none', gs = 1.0, gout = None, p16 = 'bf16', lr_dev = False),
	dict(mom = 0.9, nesterov = 1, first = 0, wd = 0.0, clip = 'inactive', gs = 0.25, gout = 'alias', p16 = 'f16', lr_dev = False),
	dict(mom = 0.9, nesterov = 0, first = 0, wd = 1e-3, clip = 'active', gs = 0.25, gout = None, p16 = 'bf16', lr_dev = True),
]


def case_id(c):
	return '-'.join(f'{k}={v}' for k, v in c.items())


def clip_setup(ops, gd, mode, gs):
	"""(sumsq buffer or None, max_norm) for a clip mode: active = half the scaled norm"""
	if mode == 'none':
		return None, 0.0
	ss = ops.sumsq(gd).clone()
	return ss, (1e9 if mode == 'inactive' else 0.5 * float(ss.sqrt()) * gs)


def sgd_case(n, c, seed, lr = 1e-2):
	"""one launch on fresh random state; returns what it wrote"""
	from convasr_amd import ops
	d = dev()
	g_ = gen(seed)
	p, g, buf = torch.randn(n, generator = g_), torch.randn(n, generator = g_) * 0.5, torch.randn(n, generator = g_) * 0.3
	dtype = HALF.get(c['p16'])
	plant_mirror_edges(p, dtype)
	momentum = c['mom'] or 0.0

	def launch(gout_mode):
		pd, gd = p.to(d), g.to(d)
		bd = None if c['mom'] is None else buf.to(d)
		p16 = None if dtype is None else torch.zeros(n, dtype = dtype, device = d)
		gout = dict(none = None, separate = torch.full((n, ), NAN, device = d), alias = gd)[gout_mode or 'none']
		ss, max_norm = clip_setup(ops, gd, c['clip'], c['gs'])
		ops.sgd_step(pd, gd, bd, n, ss, max_norm, 77.0 if c['lr_dev'] else lr, momentum, c['wd'], c['nesterov'], c['first'], grad_out = gout, grad_scale = c['gs'], p16 = p16, lr_dev = f32dev(lr) if c['lr_dev'] else None)
		return pd, bd, gout, p16, ss, max_norm

	pd, bd, gout, p16, ss, max_norm = launch(c['gout'])
	ref = R.sgd_step(p, g, None if c['mom'] is None else buf, ss, max_norm, lr, momentum, c['wd'], c['nesterov'], c['first'], grad_scale = c['gs'])
	what = f'n {n}'
	# torch.optim.SGD in fp32 on the CPU, for the record: its momentum preloaded, the gradient clipped by the same fp32 factor
	clip32 = torch.tensor(R.clip_coef(ss, max_norm, c['gs']), dtype = torch.float32)
	tp = torch.nn.Parameter(p.clone())
	opt = torch.optim.SGD([tp], lr = lr, momentum = momentum, weight_decay = c['wd'], nesterov = bool(c['nesterov']))
	if momentum != 0 and not c['first']:
		opt.state[tp] = dict(momentum_buffer = buf.clone())
	tp.grad = g * clip32
	opt.step()
	close('sgd_p', pd, ref['p'], what, cpu32 = tp.detach())
	if momentum != 0:
		close('sgd_buf', bd, ref['buf'], what, cpu32 = opt.state[tp]['momentum_buffer'])
	elif bd is not None:
		same_bits(bd, buf, f'{what}: zero momentum leaves a supplied buffer alone')
	if gout is not None:
		close('grad_out', gout, ref['grad_out'], what, cpu32 = g * clip32)
	if p16 is not None:
		mirror_is_the_rounded_result(p16, pd, what)
	if c['gout'] == 'alias':  # the production call of train.SGD(keep_clipped_grads): both pointers are __restrict__ and name one buffer
		pd2, bd2, gout2, p16_2, _, _ = launch('separate')
		same_bits(pd, pd2, f'{what}: grad_out = g against a separate grad_out, parameters')
		same_bits(gout, gout2, f'{what}: grad_out = g against a separate grad_out, clipped gradient')
		if bd is not None:
			same_bits(bd, bd2, f'{what}: grad_out = g against a separate grad_out, momentum')
	else:
		pd2, bd2, gout2, p16_2, _, _ = launch(c['gout'])
		same_bits(pd, pd2, f'{what}: a second launch')
		if bd is not None:
			same_bits(bd, bd2, f'{what}: a second launch, momentum')


@pytest.mark.parametrize('c', SGD_CASES, ids = case_id)
def test_sgd_step_small_sizes(c):
	"""n < 4 is the element-wise tail alone; 4, 1024: whole float4s; 5, 7, 1023, 1027: both"""
	for n in SMALL:
		sgd_case(n, c, 100 + n)


@pytest.mark.parametrize('c', [SGD_CASES[5], SGD_CASES[7]], ids = case_id)
def test_sgd_step_wraps_the_grid(c):
	sgd_case(WRAP, c, 7)


def test_sgd_three_step_trajectory():
	"""the reference keeps its own float64 state over three steps (momentum 0.9, Nesterov, weight decay, clipping active at step 2)"""
	from convasr_amd import ops
	d, n, lr = dev(), 1027, 1e-2
	p0 = torch.randn(n, generator = gen(1))
	pd, bd = p0.to(d), torch.zeros(n, device = d)
	p, buf = p0.double(), torch.zeros(n, dtype = torch.float64)
	tp = torch.nn.Parameter(p0.clone())
	opt = torch.optim.SGD([tp], lr = lr, momentum = 0.9, weight_decay = 1e-3, nesterov = True)
	for it in range(3):
		g = torch.randn(n, generator = gen(10 + it)) * (it + 1)
		gd = g.to(d)
		ss = ops.sumsq(gd).clone()
		ops.sgd_step(pd, gd, bd, n, ss, 50.0, lr, 0.9, 1e-3, True, it == 0)
		r = R.sgd_step(p, g, buf, ss, 50.0, lr, 0.9, 1e-3, True, it == 0)
		p, buf = r['p'], r['buf']
		tp.grad = g.clone()
		torch.nn.utils.clip_grad_norm_([tp], 50.0)
		opt.step()
		close('sgd_traj', pd, p, f'parameters after step {it}', cpu32 = tp.detach())
		close('sgd_traj', bd, buf, f'momentum after step {it}', cpu32 = opt.state[tp]['momentum_buffer'])


# ------------------------------------------------------------------------------------------------ adamw_step

ADAMW_CASES = [
	dict(t0 = 0.0, betas = (0.9, 0.999), wd = 1e-2, clip = 'none', gs = 1.0, p16 = None, lr_dev = False),
	dict(t0 = 1.0, betas = (0.9, 0.98), wd = 0.0, clip = 'active', gs = 0.25, p16 = 'bf16', lr_dev = True),
	dict(t0 = 999.0, betas = (0.0, 0.0), wd = 1e-2, clip = 'inactive', gs = 1.0, p16 = 'f16', lr_dev = False),
	dict(t0 = 1e6, betas = (0.9, 0.999), wd = 1e-2, clip = 'active', gs = 1.0, p16 = 'f16', lr_dev = False),
	dict(t0 = 0.0, betas = (0.0, 0.0), wd = 0.0, clip = 'active', gs = 0.25, p16 = None, lr_dev = False),
	dict(t0 = 999.0, betas = (0.9, 0.98), wd = 1e-2, clip = 'none', gs = 1.0, p16 = 'bf16', lr_dev = True),
	dict(t0 = 1e6, betas = (0.9, 0.98), wd = 0.0, clip = 'inactive', gs = 0.25, p16 = None, lr_dev = False),
]


def adamw_state(n, seed, t0, dtype):
	"""p, g, m, v with the first elements planted: g = m = v = 0; g = 0 alone; m = v = 0 alone (t0 = 0: the moments of a fresh optimizer are all 0)"""
	g_ = gen(seed)
	p, g, m, v = torch.randn(n, generator = g_), torch.randn(n, generator = g_) * 0.5, torch.randn(n, generator = g_) * 0.1, torch.randn(n, generator = g_).abs() * 0.01
	if t0 == 0:
		m.zero_(); v.zero_()
	for i, (gi, mi, vi) in enumerate([(0.0, 0.0, 0.0), (0.0, None, None), (None, 0.0, 0.0)][:n]):
		if gi is not None:
			g[i] = gi
		if mi is not None:
			m[i], v[i] = mi, vi
	plant_mirror_edges(p, dtype)
	return p, g, m, v


def adamw_case(n, c, seed, lr = 1e-3, eps = 1e-8):
	from convasr_amd import ops
	d = dev()
	dtype = HALF.get(c['p16'])
	p, g, m, v = adamw_state(n, seed, c['t0'], dtype)

	def launch():
		pd, gd, md, vd = p.to(d), g.to(d), m.to(d), v.to(d)
		p16 = None if dtype is None else torch.zeros(n, dtype = dtype, device = d)
		ss, max_norm = clip_setup(ops, gd, c['clip'], c['gs'])
		step_in, step_out = f32dev(c['t0']), f32dev(NAN)
		ops.adamw_step(pd, gd, md, vd, n, ss, max_norm, 77.0 if c['lr_dev'] else lr, c['betas'][0], c['betas'][1], eps, c['wd'], step_in, step_out, grad_scale = c['gs'], p16 = p16, lr_dev = f32dev(lr) if c['lr_dev'] else None)
		return pd, md, vd, p16, step_out, ss, max_norm

	pd, md, vd, p16, step_out, ss, max_norm = launch()
	ref = R.adamw_step(p, g, m, v, ss, max_norm, lr, c['betas'][0], c['betas'][1], eps, c['wd'], c['t0'], grad_scale = c['gs'])
	what = f'n {n}'
	# torch.optim.AdamW in fp32 on the CPU, for the record: its state preloaded, the gradient clipped by the same fp32 factor
	tp = torch.nn.Parameter(p.clone())
	opt = torch.optim.AdamW([tp], lr = lr, betas = c['betas'], eps = eps, weight_decay = c['wd'])
	opt.state[tp] = dict(step = torch.tensor(c['t0']), exp_avg = m.clone(), exp_avg_sq = v.clone())
	tp.grad = g * torch.tensor(R.clip_coef(ss, max_norm, c['gs']), dtype = torch.float32)
	opt.step()
	close('adamw_p', pd, ref['p'], what, cpu32 = tp.detach())
	close('exp_avg', md, ref['exp_avg'], what, cpu32 = opt.state[tp]['exp_avg'])
	close('exp_avg_sq', vd, ref['exp_avg_sq'], what, cpu32 = opt.state[tp]['exp_avg_sq'])
	assert float(step_out) == ref['step_out'] == c['t0'] + 1, (float(step_out), ref['step_out'])
	if p16 is not None:
		mirror_is_the_rounded_result(p16, pd, what)
	again = launch()
	for a, b, name in zip((pd, md, vd, step_out), (again[0], again[1], again[2], again[4]), ('parameters', 'exp_avg', 'exp_avg_sq', 'counter')):
		same_bits(a, b, f'{what}: a second launch, {name}')


@pytest.mark.parametrize('c', ADAMW_CASES, ids = case_id)
def test_adamw_step_small_sizes(c):
	for n in SMALL:
		adamw_case(n, c, 200 + n)


@pytest.mark.parametrize('c', [ADAMW_CASES[1], ADAMW_CASES[3]], ids = case_id)
def test_adamw_step_wraps_the_grid(c):
	adamw_case(WRAP, c, 9)


@pytest.mark.parametrize('n', [3, 1027])
@pytest.mark.parametrize('event', ['clean', 'overflow inf', 'overflow nan', 'gated inf', 'gated nan'])
def test_adamw_loss_scaler_and_skipped_steps(event, n):
	"""under a loss scale of 1024 a clean step is the plain step on g / 1024; an overflowed (non-finite sum of squares) or gated (non-finite
	loss) launch leaves p, m, v and the mirror bit-identical and the counter where it was"""
	from convasr_amd import ops
	d, lr, eps = dev(), 1e-3, 1e-8
	p, g, m, v = adamw_state(n, 300 + n, 5.0, torch.float16)
	pd, gd, md, vd, p16 = p.to(d), (g * 1024).to(d), m.to(d), v.to(d), p.to(d).to(torch.float16)
	p16_before = p16.clone()
	ss = ops.sumsq(gd).clone() if event == 'clean' else f64dev(INF if event == 'overflow inf' else NAN if event == 'overflow nan' else float(R.sumsq(g * 1024)))
	gate = f32dev(INF if event == 'gated inf' else NAN) if event.startswith('gated') else f32dev(2.5)
	state = R.scaler_state(1024.0, 4, unskipped = 3.0)
	s_in, s_out = scaler_pair(state)
	step_in, step_out = f32dev(5.0), f32dev(NAN)
	max_norm = 0.5 * float(R.sumsq(g).sqrt())
	ops.adamw_step(pd, gd, md, vd, n, ss, max_norm, lr, 0.9, 0.999, eps, 1e-2, step_in, step_out, loss_gate = gate, p16 = p16, scaler = (s_in, s_out))
	ref = R.adamw_step(p, g * 1024, m, v, ss, max_norm, lr, 0.9, 0.999, eps, 1e-2, 5.0, loss_gate = gate, scaler = state)
	same_bits(s_out, ref['scaler_out'], f'{event}: scaler state')
	same_bits(s_in, state, f'{event}: the state read is not written')
	assert float(step_out) == ref['step_out'] == (6.0 if event == 'clean' else 5.0)
	if event == 'clean':
		assert ref['applied'] and float(s_out[R.LS_SCALE]) == 2048.0, 'the window closes on this step'
		close('adamw_p', pd, ref['p'], f'n {n} under a loss scale')
		close('exp_avg', md, ref['exp_avg'], f'n {n} under a loss scale')
		close('exp_avg_sq', vd, ref['exp_avg_sq'], f'n {n} under a loss scale')
		mirror_is_the_rounded_result(p16, pd, 'under a loss scale')
	else:
		assert not ref['applied']
		for a, b, name in ((pd, p, 'parameters'), (md, m, 'exp_avg'), (vd, v, 'exp_avg_sq'), (p16, p16_before, 'mirror')):
			same_bits(a, b, f'{event}: {name}')


def test_adamw_three_step_trajectory():
	from convasr_amd import ops
	d, n, lr, eps = dev(), 1027, 1e-3, 1e-8
	p0 = torch.randn(n, generator = gen(1))
	pd, md, vd = p0.to(d), torch.zeros(n, device = d), torch.zeros(n, device = d)
	steps = torch.zeros(2, 1, device = d)
	p, m, v, t = p0.double(), torch.zeros(n, dtype = torch.float64), torch.zeros(n, dtype = torch.float64), 0.0
	tp = torch.nn.Parameter(p0.clone())
	opt = torch.optim.AdamW([tp], lr = lr, betas = (0.9, 0.999), eps = eps, weight_decay = 1e-2)
	for it in range(3):
		g = torch.randn(n, generator = gen(10 + it)) * (it + 1)
		gd = g.to(d)
		ss = ops.sumsq(gd).clone()
		ops.adamw_step(pd, gd, md, vd, n, ss, 50.0, lr, 0.9, 0.999, eps, 1e-2, steps[it % 2], steps[1 - it % 2])
		r = R.adamw_step(p, g, m, v, ss, 50.0, lr, 0.9, 0.999, eps, 1e-2, t)
		p, m, v, t = r['p'], r['exp_avg'], r['exp_avg_sq'], r['step_out']
		tp.grad = g.clone()
		torch.nn.utils.clip_grad_norm_([tp], 50.0)
		opt.step()
		assert float(steps[1 - it % 2]) == t == it + 1
		close('adamw_traj', pd, p, f'parameters after step {it}', cpu32 = tp.detach())
		close('exp_avg', md, m, f'trajectory, step {it}', cpu32 = opt.state[tp]['exp_avg'])
		close('exp_avg_sq', vd, v, f'trajectory, step {it}', cpu32 = opt.state[tp]['exp_avg_sq'])


# ------------------------------------------------------------------------------------------------ novograd_step

def cumulate(sizes):
	offsets = [0]
	for s in sizes:
		offsets.append(offsets[-1] + s)
	return offsets


LAYOUTS = {
	'a': [0, 64, 1000, 1003, 5000],                                       # everything inside one chunk, unaligned boundaries
	'b': [0, 8191, 8192, 8193, 28193, 30000],                             # boundaries at 8191, exactly 8192, 8193; one-element segments; 20000 elements over three chunks
	'c': cumulate([65536, 65537, 2 * 65536 + 17]),                        # one item exactly, one item and a 1-element item, two items and a 17-element one; every later item starts unaligned
	'd2047': cumulate([64] * 2047),                                       # n_seg + 1 = NG_TABLE: the offsets just fit the LDS table
	'd2048': cumulate([64] * 2048),                                       # one more: global offsets
	'd2100': cumulate([64] * 2100),
	'e': cumulate([16] * 2100),                                           # 512 segments per chunk: the publish loop and the norm loop stride by 256
	'f': [0, 0, 100, 100, 8192, 8192, 8192, 9000, 16384, 16384, 20000, 20000, 20000],  # empty segments: at 0, inside a chunk, on chunk edges (two in a row; one where a segment ends), at the arena's end
}

# first (1, 0, or -1 with the counter behind the EMAs), dampening, weight decay, clip, grad_scale, mirror, lr_dev, loss scale (None or a finite scale)
NG_CASES = [
	dict(layout = 'a', first = 1, counter = None, damp = 0, wd = 0.0, clip = 'none', gs = 1.0, p16 = None, lr_dev = False, scale = None),
	dict(layout = 'a', first = -1, counter = 5.0, damp = 1, wd = 1e-3, clip = 'active', gs = 0.25, p16 = 'f16', lr_dev = True, scale = 1024.0),
	dict(layout = 'b', first = 0, counter = None, damp = 0, wd = 1e-3, clip = 'active', gs = 1.0, p16 = 'bf16', lr_dev = False, scale = None),
	dict(layout = 'b', first = -1, counter = 0.0, damp = 1, wd = 0.0, clip = 'inactive', gs = 0.25, p16 = None, lr_dev = False, scale = None),
	dict(layout = 'b', first = -1, counter = 5.0, damp = 0, wd = 1e-3, clip = 'none', gs = 1.0, p16 = 'f16', lr_dev = True, scale = 64.0),
	dict(layout = 'c', first = 0, counter = None, damp = 0, wd = 1e-3, clip = 'active', gs = 1.0, p16 = 'f16', lr_dev = False, scale = None),
	dict(layout = 'c', first = 1, counter = None, damp = 1, wd = 0.0, clip = 'none', gs = 0.25, p16 = None, lr_dev = False, scale = None),
	dict(layout = 'd2047', first = -1, counter = 5.0, damp = 0, wd = 1e-3, clip = 'active', gs = 1.0, p16 = None, lr_dev = False, scale = None),
	dict(layout = 'd2048', first = 0, counter = None, damp = 0, wd = 0.0, clip = 'inactive', gs = 1.0, p16 = 'bf16', lr_dev = False, scale = None),
	dict(layout = 'd2100', first = 1, counter = None, damp = 1, wd = 1e-3, clip = 'active', gs = 0.25, p16 = None, lr_dev = False, scale = None),
	dict(layout = 'e', first = 0, counter = None, damp = 0, wd = 1e-3, clip = 'active', gs = 1.0, p16 = None, lr_dev = False, scale = None),
	dict(layout = 'e', first = -1, counter = 0.0, damp = 0, wd = 0.0, clip = 'none', gs = 1.0, p16 = 'bf16', lr_dev = False, scale = 1024.0),
	dict(layout = 'f', first = 0, counter = None, damp = 0, wd = 1e-3, clip = 'active', gs = 1.0, p16 = None, lr_dev = False, scale = None),
	dict(layout = 'f', first = -1, counter = 0.0, damp = 1, wd = 0.0, clip = 'none', gs = 1.0, p16 = 'f16', lr_dev = False, scale = None),
]
NG_HYPER = dict(lr = 1e-2, b1 = 0.95, b2 = 0.98, eps = 1e-8)


def ng_state(offsets, seed, counter, scale = 1.0):
	"""p, g, mom, ema_in for a layout; the segments' gradient scales differ (x 1 .. x 8), the second non-empty segment has no gradient at all"""
	n, n_seg = offsets[-1], len(offsets) - 1
	g_ = gen(seed)
	p, g, mom = torch.randn(n, generator = g_), torch.randn(n, generator = g_) * 0.1, torch.randn(n, generator = g_) * 0.5
	filled = [s for s in range(n_seg) if offsets[s + 1] > offsets[s]]
	for k, s in enumerate(filled):
		g[offsets[s]:offsets[s + 1]] *= (1 + k % 8) if k != 1 else 0.0
	ema = torch.rand(n_seg + (counter is not None), generator = g_) + 0.01
	if counter is not None:
		ema[n_seg] = counter
	return p, g * scale, mom, ema


def ng_launch(ops, offsets, state, c, max_norm, gate = None, scaler = None, lr = NG_HYPER['lr']):
	"""one launch from host state; the outputs start as NaNs, so whatever the kernel leaves unwritten shows"""
	d = dev()
	p, g, mom, ema = state
	n, n_seg = offsets[-1], len(offsets) - 1
	pd, gd, md, e_in = p.to(d), g.to(d), mom.to(d), ema.to(d)
	e_out = torch.full_like(e_in, NAN)
	dtype = HALF.get(c['p16'])
	p16 = None if dtype is None else pd.to(dtype)
	g2, total = torch.full((n_seg, ), NAN, dtype = torch.float64, device = d), torch.full((1, ), NAN, device = d)
	ops.novograd_step(pd, gd, md, e_in, e_out, g2, torch.tensor(offsets, dtype = torch.int64, device = d), n, ops.novograd_work_table(offsets, d), max_norm, 77.0 if c['lr_dev'] else lr,
	                  NG_HYPER['b1'], NG_HYPER['b2'], NG_HYPER['eps'], c['wd'], c['damp'], c['first'], loss_gate = gate, total_norm = total, grad_scale = c['gs'], p16 = p16, scaler = scaler,
	                  lr_dev = f32dev(lr) if c['lr_dev'] else None)
	return dict(p = pd, mom = md, ema_out = e_out, g2 = g2, total = total, p16 = p16)


def ng_max_norm(offsets, g, c):
	norm = float(R.sumsq(g).sqrt()) * c['gs'] / (c['scale'] or 1.0)
	return dict(none = 0.0, inactive = 1e9, active = 0.5 * norm)[c['clip']]


@pytest.mark.parametrize('c', NG_CASES, ids = case_id)
def test_novograd_step_layouts(c):
	"""every element of p and momentum, every segment's EMA (of the CLIPPED gradient) and sum of squares, the total norm, the counter"""
	from convasr_amd import ops
	offsets = LAYOUTS[c['layout']]
	n_seg = len(offsets) - 1
	state = ng_state(offsets, 400 + n_seg, c['counter'], c['scale'] or 1.0)
	p, g, mom, ema = state
	max_norm = ng_max_norm(offsets, g, c)
	sc = None if c['scale'] is None else R.scaler_state(c['scale'], 7, unskipped = 2.0)
	pair = None if sc is None else scaler_pair(sc)
	out = ng_launch(ops, offsets, state, c, max_norm, scaler = pair)
	ref = R.novograd_step(offsets, p, g, mom, ema, max_norm, NG_HYPER['lr'], NG_HYPER['b1'], NG_HYPER['b2'], NG_HYPER['eps'], c['wd'], c['damp'], c['first'], grad_scale = c['gs'], scaler = sc)
	assert ref['applied']
	what = f"layout {c['layout']}"
	close('ng_g2', out['g2'], ref['g2'], what)
	close('norm', out['total'], ref['total_norm'], what + ' total_norm')
	close('ng_ema', out['ema_out'][:n_seg], ref['ema_out'], what)
	close('ng_p', out['p'], ref['p'], what)
	close('ng_mom', out['mom'], ref['mom'], what)
	if c['first'] < 0:
		assert float(out['ema_out'][n_seg]) == ref['counter'] == c['counter'] + 1
	if out['p16'] is not None:
		mirror_is_the_rounded_result(out['p16'], out['p'], what)
	if pair is not None:
		same_bits(pair[1], ref['scaler_out'], what + ': scaler state')
	again = ng_launch(ops, offsets, state, c, max_norm, scaler = None if sc is None else scaler_pair(sc))
	for k in ('p', 'mom', 'ema_out', 'g2', 'total'):
		same_bits(out[k], again[k], f'{what}: a second launch, {k}')


def test_novograd_counter_stops_at_two_to_the_24():
	from convasr_amd import ops
	offsets = LAYOUTS['a']
	c = dict(NG_CASES[0], first = -1)
	for counter in (2.0 ** 24 - 1, 2.0 ** 24):
		out = ng_launch(ops, offsets, ng_state(offsets, 1, counter), c, 0.0)
		assert float(out['ema_out'][-1]) == R.counter_next(counter) == 2.0 ** 24


@pytest.mark.parametrize('layout', ['b', 'd2100'])
@pytest.mark.parametrize('event', ['overflow inf', 'overflow nan', 'gated inf', 'gated nan'])
def test_novograd_skipped_steps_carry_the_emas_over(event, layout):
	"""a gated or overflowed launch: p, momentum and the mirror bit-identical, every EMA and the counter carried into ema_out, the scaler
	advanced (overflow) or copied (gated), total_norm still reported (non-finite after an overflow)"""
	from convasr_amd import ops
	offsets = LAYOUTS[layout]
	n_seg = len(offsets) - 1
	c = dict(NG_CASES[1], layout = layout)
	p, g, mom, ema = ng_state(offsets, 500 + n_seg, 5.0, 1024.0)
	if event.startswith('overflow'):
		g[offsets[2] + 1] = INF if event.endswith('inf') else NAN
	gate = f32dev(INF if event == 'gated inf' else NAN) if event.startswith('gated') else None
	sc = R.scaler_state(1024.0, 7, unskipped = 6.0, min_scale = 1024.0)
	pair = scaler_pair(sc)
	out = ng_launch(ops, offsets, (p, g, mom, ema), c, 1.0, gate = gate, scaler = pair)
	ref = R.novograd_step(offsets, p, g, mom, ema, 1.0, NG_HYPER['lr'], NG_HYPER['b1'], NG_HYPER['b2'], NG_HYPER['eps'], c['wd'], c['damp'], -1, loss_gate = gate, grad_scale = c['gs'], scaler = sc)
	assert not ref['applied']
	same_bits(out['p'], p, f'{event}: parameters')
	same_bits(out['mom'], mom, f'{event}: momentum')
	same_bits(out['p16'], p.to(torch.float16), f'{event}: mirror')
	same_bits(out['ema_out'], ema, f'{event}: EMAs and counter carried over')
	same_bits(pair[1], ref['scaler_out'], f'{event}: scaler state')
	if event.startswith('overflow'):
		assert not bool(torch.isfinite(out['total']).any()) and float(pair[1][R.LS_SCALE]) == 1024.0 and float(pair[1][R.LS_SKIPPED_STEPS]) == 1.0, 'min_scale holds the scale'
	else:
		close('norm', out['total'], ref['total_norm'], f'{event}: total_norm')


def test_novograd_three_step_trajectory():
	"""layout b, the device's counter decides `first`; the reference keeps its own float64 state"""
	from convasr_amd import ops
	d = dev()
	offsets = LAYOUTS['b']
	n, n_seg = offsets[-1], len(offsets) - 1
	p0 = torch.randn(n, generator = gen(1))
	pd, md = p0.to(d), torch.zeros(n, device = d)
	emas = torch.zeros(2, n_seg + 1, device = d)
	g2, total = torch.zeros(n_seg, dtype = torch.float64, device = d), torch.zeros(1, device = d)
	table, off_d = ops.novograd_work_table(offsets, d), torch.tensor(offsets, dtype = torch.int64, device = d)
	p, mom, ema = p0.double(), torch.zeros(n, dtype = torch.float64), torch.zeros(n_seg + 1, dtype = torch.float64)
	for it in range(3):
		g = torch.randn(n, generator = gen(10 + it)) * 0.1 * (it + 1)
		ops.novograd_step(pd, g.to(d), md, emas[it % 2], emas[1 - it % 2], g2, off_d, n, table, 10.0, 1e-2, 0.95, 0.98, 1e-8, 1e-3, False, -1, total_norm = total)
		r = R.novograd_step(offsets, p, g, mom, ema, 10.0, 1e-2, 0.95, 0.98, 1e-8, 1e-3, False, -1)
		p, mom, ema = r['p'], r['mom'], torch.cat([r['ema_out'], torch.tensor([r['counter']], dtype = torch.float64)])
		close('ng_traj', pd, p, f'parameters after step {it}')
		close('ng_traj', md, mom, f'momentum after step {it}')
		close('ng_ema', emas[1 - it % 2, :n_seg], r['ema_out'], f'trajectory, step {it}')
		assert float(emas[1 - it % 2, n_seg]) == it + 1


# ------------------------------------------------------------------------------------------------ the 16-bit mirror at its rounding edges

F16_MIN_NORMAL, BF16_MIN_NORMAL = 2.0 ** -14, 2.0 ** -126
# (fp32 parameter, what one round-to-nearest-even into the 16-bit type gives, or None for "a subnormal": 0 < |result| < the smallest normal)
EDGES = {
	'f16': [(7e4, INF), (-1e5, -INF), (65520.0, INF), (65519.996, 65504.0), (3e-6, None), (-1e-7, None), (6e-8, None), (2.0 ** -25, 0.0), (3.1e-8, None), (1.5 * 2.0 ** -24, 2.0 ** -23),
	        (1 + 2.0 ** -11, 1.0), (-(1 + 3 * 2.0 ** -11), -(1 + 2.0 ** -9))],
	'bf16': [(3.4e38, INF), (-3.4e38, -INF), (2.0 ** 128 - 2.0 ** 119, INF), (3.396e38, 2.0 ** 128 - 2.0 ** 120), (1e-39, None), (-5e-40, None), (9.2e-41, None), (2.0 ** -134, 0.0), (4.7e-41, None),
	         (1.5 * 2.0 ** -133, 2.0 ** -132), (1 + 2.0 ** -8, 1.0), (-(1 + 3 * 2.0 ** -8), -(1 + 2.0 ** -6))],
}


@pytest.mark.parametrize('half', ['f16', 'bf16'])
@pytest.mark.parametrize('optimizer', ['sgd', 'adamw', 'novograd'])
def test_mirror_rounding_edges(optimizer, half):
	"""lr = 0 (and, for SGD / AdamW, no weight decay): the fp32 result IS the parameter it started from, bit for bit, so the mirror is
	round(p) with p chosen: beyond the largest finite value (-> inf), the tie between it and inf (-> inf) and the last value below that tie,
	subnormals of the 16-bit type, half the smallest subnormal (a tie -> 0) and just above it, a tie between two subnormals and two between
	normals (-> even).  Cycled through the array with every shift, at n = 1, 2, 3 (the element-wise tail alone), 7 and 1027 (float4 body and
	tail), so every value passes through the packed body store and through the tail store; the test checks that it did."""
	from convasr_amd import ops
	d, dtype = dev(), HALF[half]
	min_normal = F16_MIN_NORMAL if half == 'f16' else BF16_MIN_NORMAL
	vals = torch.tensor([v for v, _ in EDGES[half]], dtype = torch.float32)
	for (v, exp), x in zip(EDGES[half], vals):  # the table itself: torch rounds each value as it says
		r = x.to(dtype).float()
		assert (0 < abs(float(r)) < min_normal) if exp is None else float(r) == exp, (v, float(r), exp)
	seen = dict(body = set(), tail = set(), below4 = set())
	for n in (1, 2, 3, 7, 1027):
		for shift in range(len(vals)):
			p = vals[(torch.arange(n) + shift) % len(vals)].clone()
			g_ = gen(n + shift)
			g, aux = torch.randn(n, generator = g_) * 0.5, torch.randn(n, generator = g_).abs() * 0.1 + 0.01
			pd, p16 = p.to(d), torch.full((n, ), 7.0, dtype = dtype, device = d)
			if optimizer == 'sgd':
				ops.sgd_step(pd, g.to(d), aux.to(d), n, None, 0.0, 0.0, 0.9, 0.0, True, False, p16 = p16)
			elif optimizer == 'adamw':
				ops.adamw_step(pd, g.to(d), aux.to(d), aux.to(d), n, None, 0.0, 0.0, 0.9, 0.999, 1e-8, 0.0, f32dev(3.0), f32dev(NAN), p16 = p16)
			else:
				offsets = [0, n // 2, n] if n > 1 else [0, n]
				ema = torch.ones(len(offsets) - 1)
				ops.novograd_step(pd, g.to(d), aux.to(d), ema.to(d), torch.zeros_like(ema).to(d), torch.zeros(len(offsets) - 1, dtype = torch.float64, device = d), torch.tensor(offsets, dtype = torch.int64, device = d), n,
				                  ops.novograd_work_table(offsets, d), 0.0, 0.0, 0.95, 0.98, 1e-8, 0.0, False, 0, p16 = p16)
			same_bits(pd, p, f'{optimizer} n {n} shift {shift}: a step with lr = 0 leaves the fp32 parameters as they were')
			mirror_is_the_rounded_result(p16, pd, f'{optimizer} n {n} shift {shift}')
			for i in range(n):  # (pd == p bit for bit, checked above: the fp32 RESULT at position i is entry (i + shift) % len of the table)
				seen['below4' if n < 4 else 'tail' if i >= n - n % 4 else 'body'].add((i + shift) % len(vals))
	for where, entries in seen.items():  # every overflow, subnormal, zero and tie of the table went through that store
		assert entries == set(range(len(vals))), (where, entries)


# ------------------------------------------------------------------------------------------------ loss scaler: raw states through all three optimizers

# name: (state read, event).  scale, window, factor 2, then min / max / unskipped
SCALER_CASES = {
	'clean, inside the window': (R.scaler_state(1024.0, 4, unskipped = 1.0), 'clean'),
	'clean, the window closes': (R.scaler_state(1024.0, 4, unskipped = 3.0), 'clean'),
	'clean, the window closes at max_scale': (R.scaler_state(2.0 ** 12, 4, unskipped = 3.0, max_scale = 2.0 ** 12), 'clean'),
	'clean, the window closes just under max_scale': (R.scaler_state(2.0 ** 12, 4, unskipped = 3.0, max_scale = 5000.0), 'clean'),
	'clean, window 1': (R.scaler_state(4.0, 1), 'clean'),
	'overflow': (R.scaler_state(1024.0, 4, unskipped = 2.0, skipped_steps = 3.0), 'overflow'),
	'overflow at min_scale': (R.scaler_state(8.0, 4, unskipped = 2.0, min_scale = 8.0), 'overflow'),
	'overflow just above min_scale': (R.scaler_state(8.0, 4, unskipped = 3.0, min_scale = 5.0), 'overflow'),
	'overflow, factor 4': (R.scaler_state(1024.0, 4, factor = 4.0, unskipped = 3.0), 'overflow'),
	'gated': (R.scaler_state(1024.0, 4, unskipped = 3.0), 'gated'),
	'gated and overflowed': (R.scaler_state(1024.0, 4, unskipped = 3.0), 'gated overflow'),
	'static': (R.scaler_state(128.0, 0), 'clean'),
	'static, gated': (R.scaler_state(128.0, 0), 'gated'),
}


@pytest.mark.parametrize('optimizer', ['sgd', 'adamw', 'novograd'])
@pytest.mark.parametrize('name', list(SCALER_CASES))
def test_loss_scaler_raw_states(name, optimizer):
	"""scaler_out bit for bit against loss_scale_advance's restatement; the state read stays as it was; whether the step was applied follows
	the same verdict (a gated launch does not look at the gradient: the state is copied, overflow flag included)"""
	from convasr_amd import ops
	d, n = dev(), 1027
	state, event = SCALER_CASES[name]
	scale = float(state[R.LS_SCALE])
	g_ = gen(11)
	p, g, aux = torch.randn(n, generator = g_), torch.randn(n, generator = g_) * scale, torch.randn(n, generator = g_).abs() * 0.1
	overflow, gated = 'overflow' in event, 'gated' in event
	gate = f32dev(NAN) if gated else None
	pd, gd, ad, bd = p.to(d), g.to(d), aux.to(d), aux.to(d)
	s_in, s_out = scaler_pair(state)
	if optimizer == 'novograd':
		offsets = [0, 64, 1000, n]
		if overflow:
			g[999] = INF
		ema = torch.tensor([0.5, 0.25, 2.0, 3.0])
		out = ng_launch(ops, offsets, (p, g, aux, ema), dict(NG_CASES[0], first = -1), 0.0, gate = gate, scaler = (s_in, s_out))
		ref = R.novograd_step(offsets, p, g, aux, ema, 0.0, NG_HYPER['lr'], NG_HYPER['b1'], NG_HYPER['b2'], NG_HYPER['eps'], 0.0, 0, -1, loss_gate = gate, scaler = state)
		pd, changed = out['p'], float(out['ema_out'][3]) == 4.0
	else:
		ss = f64dev(INF) if overflow else ops.sumsq(gd).clone()
		if optimizer == 'sgd':
			ops.sgd_step(pd, gd, bd, n, ss, 0.0, 1e-2, 0.9, 1e-3, False, False, loss_gate = gate, scaler = (s_in, s_out))
			ref = R.sgd_step(p, g, aux, ss, 0.0, 1e-2, 0.9, 1e-3, False, False, loss_gate = gate, scaler = state)
			changed = not torch.equal(bd.cpu(), aux)
		else:
			step_out = f32dev(NAN)
			ops.adamw_step(pd, gd, ad, bd, n, ss, 0.0, 1e-3, 0.9, 0.999, 1e-8, 1e-2, f32dev(3.0), step_out, loss_gate = gate, scaler = (s_in, s_out))
			ref = R.adamw_step(p, g, aux, aux, ss, 0.0, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3.0, loss_gate = gate, scaler = state)
			changed = float(step_out) == 4.0
	same_bits(s_out, ref['scaler_out'], f'{name}: scaler_out')
	same_bits(s_in, state, f'{name}: the state read is not written')
	assert changed == ref['applied'] == (not gated and not overflow), (changed, ref['applied'])
	if not ref['applied']:
		same_bits(pd, p, f'{name}: parameters of a skipped step')


# ------------------------------------------------------------------------------------------------ through the classes

CLASS_SIZES = [8191, 1, 20000, 65536, 65537, 2 * 65536 + 17, 5]  # padded to 64: a boundary exactly on a chunk edge, a 64-element segment behind it, segments of one, two and three items


def holder(sizes, seed):
	h = torch.nn.Module()
	h.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, generator = gen(seed + i)).to(dev())) for i, s in enumerate(sizes)])
	return h


def set_grads(flat, seed, scale):
	for i, p in enumerate(flat.params):
		p._convasr_grad.copy_(torch.randn(p.numel(), generator = gen(seed + i)).to(dev()) * scale * (1 + i % 3))
		p._convasr_fresh = False


@pytest.mark.parametrize('optimizer', ['novograd', 'adamw', 'sgd'])
def test_classes_second_step_matches_the_reference(optimizer):
	"""FlatParameters + NovoGrad / AdamW / train.SGD(keep_clipped_grads) with a bf16 mirror: two steps, the second one against the reference
	started from the device's state after the first"""
	import convasr_amd as ca
	flat = ca.train.FlatParameters(holder(CLASS_SIZES, 1))
	offsets, n = list(flat.offsets) + [flat.numel], flat.numel
	assert offsets[1] == 8192 and offsets[2] == 8256
	flat.mirror(torch.bfloat16)
	lr, max_norm = 1e-2, 3.0
	if optimizer == 'novograd':
		opt = ca.optimizers.NovoGrad(flat, lr = lr, betas = (0.95, 0.98), weight_decay = 1e-3)
	elif optimizer == 'adamw':
		opt = ca.optimizers.AdamW(flat, lr = lr, betas = (0.9, 0.999), weight_decay = 1e-2)
	else:
		opt = ca.train.SGD(flat, lr = lr, momentum = 0.9, weight_decay = 1e-3, nesterov = True, keep_clipped_grads = True)
	for it in range(2):
		set_grads(flat, 50 + 10 * it, 0.02)
		p, g = flat.data.cpu(), flat.grad.cpu()
		if optimizer == 'novograd':
			mom, ema = opt.momentum_buffer.cpu(), opt.grads_ema[opt._cur].cpu()
		elif optimizer == 'adamw':
			m, v, t0 = opt.exp_avg.cpu(), opt.exp_avg_sq.cpu(), float(opt.applied[opt._cur, 0])
		else:
			buf = opt.momentum_buffer.cpu()
		norm = flat.clip_grad_norm_(max_norm)
		ss = flat._sumsq.clone()
		opt.step()
		assert float(norm) > max_norm, 'the clip is active'
		close('norm', norm, R.grad_norm(R.sumsq(g)), f'{optimizer} step {it} clip_grad_norm_')
		what = f'{optimizer} class, step {it}'
		if optimizer == 'novograd':
			r = R.novograd_step(offsets, p, g, mom, ema, max_norm, lr, 0.95, 0.98, 1e-8, 1e-3, False, -1)
			close('norm', opt.total_norm, r['total_norm'], what + ' total_norm')
			close('ng_ema', opt.grads_ema[opt._cur, :opt.n_seg], r['ema_out'], what)
			close('ng_p', flat.data, r['p'], what)
			close('ng_mom', opt.momentum_buffer, r['mom'], what)
			assert float(opt.grads_ema[opt._cur, opt.n_seg]) == it + 1
		elif optimizer == 'adamw':
			r = R.adamw_step(p, g, m, v, ss, max_norm, lr, 0.9, 0.999, 1e-8, 1e-2, t0)
			close('adamw_p', flat.data, r['p'], what)
			close('exp_avg', opt.exp_avg, r['exp_avg'], what)
			close('exp_avg_sq', opt.exp_avg_sq, r['exp_avg_sq'], what)
			assert float(opt.applied[opt._cur, 0]) == it + 1
		else:
			r = R.sgd_step(p, g, buf, ss, max_norm, lr, 0.9, 1e-3, True, it == 0)
			close('sgd_p', flat.data, r['p'], what)
			close('sgd_buf', opt.momentum_buffer, r['buf'], what)
			close('grad_out', flat.grad, r['grad_out'], what + ' (the clipped gradient kept in .grad)')
		mirror_is_the_rounded_result(flat.data16, flat.data, what)
		opt.zero_grad()


def test_classes_accept_a_parameter_without_elements():
	"""trainable parameters with numel() == 0: one whose (empty) segment starts on a chunk edge, one at the arena's end.  Their EMAs are
	written every step (first step: 0, the squared norm of nothing) -- preloaded with a marker to see it -- and the others are unaffected"""
	import convasr_amd as ca
	sizes = [8192, 0, 100, 0]
	flat = ca.train.FlatParameters(holder(sizes, 3))
	offsets = list(flat.offsets) + [flat.numel]
	assert offsets == [0, 8192, 8192, 8320, 8320]
	opt = ca.optimizers.NovoGrad(flat, lr = 1e-2, betas = (0.95, 0.98), weight_decay = 1e-3)
	opt.grads_ema[:, :4] = 7.0
	for it in range(2):
		set_grads(flat, 60 + it, 0.1)
		p, g, mom, ema = flat.data.cpu(), flat.grad.cpu(), opt.momentum_buffer.cpu(), opt.grads_ema[opt._cur].cpu()
		opt.step()
		r = R.novograd_step(offsets, p, g, mom, ema, 0.0, 1e-2, 0.95, 0.98, 1e-8, 1e-3, False, -1)
		close('ng_ema', opt.grads_ema[opt._cur, :4], r['ema_out'], f'empty parameters, step {it}')
		close('ng_p', flat.data, r['p'], f'empty parameters, step {it}')
		opt.zero_grad()
	assert opt.grads_ema[opt._cur, [1, 3]].tolist() == [0.0, 0.0]
