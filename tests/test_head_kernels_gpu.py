"""The log-prob head and the plumbing kernels (convasr_amd/csrc/misc.hip, collate_pad of csrc/next.hip, signal_absmax of csrc/frontend.hip) on
the MI355X against the float64 restatement tests/_head_ref.py (itself held to torch float64, the oracle and the goldens in
tests/test_head_ref.py), at the shapes where each kernel takes another path: the 64-lane class stride and four rows per workgroup of
log_softmax / argmax, the 1024 / 2048-element walk of entropy, the 16 frames in flight of weighted_mean_entropy, the 16-channel x 64-lane
blocks of instnorm, the 64 x 64 tile of convert_layout, the launch caps that turn scale_rows / add16 / cast_scale / copy into grid-stride
loops, copy's aligned / byte split and loss_head's 256-thread tree.

Exact ops (argmax, output_lengths, convert_layout, add16, cast_scale, copy, collate_pad, gvec, skipped, zero padding) are compared bit
for bit; NaN positions by NaN-ness.  fp32 arithmetic is compared with the float64 restatement over every element, against
atol + rtol |ref| with (rtol, atol) = SHARE[quantity] x the project's bar for that quantity (PROJECT, from tests/test_kernels_gpu.py).
SHARE is 4x the worst share measured on the MI355X over every check of the quantity in this file, and never above 1 (the measured values are
next to the constants).  Every check prints what it measured next to its bar, and next to what torch's own fp32 CPU op scores against the
same float64 where there is one; the table is in profiles/NOTEBOOK.md, section 15."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _head_ref as R  # noqa: E402

from oracle import convasr_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

INF, NAN = float('inf'), float('nan')
DTYPES = dict(f32 = torch.float32, bf16 = torch.bfloat16, f16 = torch.float16)
PAIRS = [('f32', 'f32'), ('f32', 'bf16'), ('bf16', 'f32'), ('bf16', 'bf16'), ('f32', 'f16'), ('f16', 'f32'), ('f16', 'f16')]  # the seven (source, destination) pairs the launchers accept

U32 = 2.0 ** -24  # unit roundoff of fp32
# (rtol, atol) each quantity may never exceed.  Where the project already has a bar for the quantity it is that one (tests/test_kernels_gpu.py:
# log_softmax, the two entropies, instnorm per output type, normalize_signal, and test_loss_head_matches_the_reference_expressions' 2e-6 / 1e-7
# for the loss head's means).  The two without one are derived from the number format and the kernel's chain of operations:
#   scale_rows: one rounding of the scale (gscale / gdiv), one of the product, and the input gscale is exact: 2 u, taken as 3 u; no absolute
#     term beyond fp32's underflow (the inputs are O(1))
#   instnorm_running: (1 - m) r + m mean_b(stat) where each statistic is a sum of T terms added in ceil(T / 64) + 64 steps (T <= 300: 69), then
#     B more additions, a division, two products and a sum: 80 u relative to the magnitudes involved (|x| up to ~10 for a result of ~1, hence
#     the same figure as absolute term)
PROJECT = dict(log_softmax = (1e-5, 1e-5), log_softmax_bwd = (1e-5, 1e-5), entropy = (1e-4, 1e-5), weighted_entropy = (2e-5, 1e-6), scale_rows = (3 * U32, 1e-30),
               loss_head = (2e-6, 1e-7), instnorm_f32 = (1e-5, 1e-5), instnorm_bf16 = (4e-3, 1e-5), instnorm_f16 = (6e-4, 1e-5), instnorm_running = (80 * U32, 80 * U32),
               normalize_signal = (3e-7, 1e-9))
# share of the bar above each quantity is held to = min(1, 4 x the worst share measured on the MI355X over every check of this file); the comment
# gives that measured worst share, and torch fp32 on the CPU against the same float64 where there is such an op
SHARE = dict(
	log_softmax = 1.0,          # 0.387 measured (C 65, logits x 30: the class at the maximum, where lse = m + log s is rounded at |m| ~ 100 before x - lse); torch 0.016 there, 0.091 at worst
	log_softmax_bwd = 0.53,     # 0.131 measured (C 257, 211 rows); torch 0.142
	entropy = 8.5e-3,           # 2.11e-3 measured (C 23 T 89); torch 1.6e-3
	weighted_entropy = 0.49,    # 0.122 measured (C 64, the mass on eps_id, eps 1e-2); torch 0.068
	scale_rows = 1.0,           # 0.604 measured = 1.81 u of the 3 u (both factors); torch 0.604, the same two roundings
	loss_head = 0.29,           # 0.071 measured (B 257); torch 0.059
	instnorm_f32 = 1.0,         # 0.680 measured on the 1 +- 2^-10 channel of test_instnorm_constant_channels (|mean| / std = 300); 0.181 at worst elsewhere (C 64 T 63), torch 0.107 there
	instnorm_bf16 = 1.0,        # 0.972 measured: the one rounding of the output, 2^-9 of 4e-3
	instnorm_f16 = 1.0,         # 0.805 measured: the one rounding of the output, 2^-12 of 6e-4
	instnorm_running = 0.083,   # 0.0208 measured (C 80 T 65, running_var after the third call)
	normalize_signal = 1.0,     # 0.482 measured (T 24581, multiplier 2.5); torch 0.396
)


def dev():
	return torch.device('cuda:0')


def gen(seed):
	return torch.Generator().manual_seed(seed)


def share_of(a, b, bar):
	"""worst err / (atol + rtol |ref|) over every element; positions where the reference is infinite must agree exactly"""
	a, b = a.detach().double().cpu(), b.detach().double().cpu()
	assert a.shape == b.shape, (a.shape, b.shape)
	inf = torch.isinf(b)
	assert torch.equal(a[inf], b[inf]), 'infinite entries differ'
	assert bool(torch.isfinite(a[~inf]).all()), 'non-finite result'
	if int((~inf).sum()) == 0:
		return 0.0
	return float(((a - b)[~inf].abs() / (bar[1] + bar[0] * b[~inf].abs())).max())


def close(key, got, ref, what, cpu32 = None, bar = None):
	"""got against the float64 ref at SHARE[key] of the project's bar (or an explicit, derived `bar`); cpu32: torch fp32 on the CPU, for the record"""
	proj = PROJECT[key] if bar is None else bar
	allowed = SHARE[key] if bar is None else 1.0
	s = share_of(got, ref, proj)
	note = '' if cpu32 is None else f', torch fp32 cpu {share_of(cpu32, ref, proj):.3e}'
	print(f'    HEAD {key} {what}: measured {s:.3e} of ({proj[0]:.1e}, {proj[1]:.1e}), bar {allowed:.3e}{note}')
	assert s <= allowed, f'{key} {what}: {s:.3e} of the bar ({proj[0]:.1e}, {proj[1]:.1e}), allowed {allowed:.3e}'


def bits(t):
	t = t.detach().cpu().contiguous()
	return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(got, exp, what):
	"""bit for bit; where the expected value is NaN the result must be a NaN (any payload)"""
	got, exp = got.detach().cpu(), exp.detach().cpu()
	assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
	if exp.is_floating_point():
		nan = torch.isnan(exp)
		assert torch.equal(torch.isnan(got), nan), f'{what}: NaN positions'
		got, exp = torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(exp), exp)
	bad = bits(got) != bits(exp)
	assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.flatten().nonzero()[0].item()}'


def cl(x, d, dtype = None):
	"""host (B, C, T) -> the kernels' channels-last device tensor, strides (T C, 1, C) whatever the sizes"""
	B, C, T = x.shape
	out = torch.empty(B, T, C, dtype = dtype or x.dtype, device = d).permute(0, 2, 1)
	out.copy_(x)
	return out


def rep(x, dt):
	return x.to(dt).float()


# ------------------------------------------------------------------------------------------------ log_softmax, argmax

ROWS = [(1, 1), (2, 1), (1, 3), (2, 2), (5, 1), (1, 211)]  # B x T = 1, 2, 3, 4, 5, 211 rows: part of a workgroup, exactly one, one and a part, 53


@pytest.mark.parametrize('scale', [3, 30])
@pytest.mark.parametrize('C', [1, 2, 38, 63, 64, 65, 129, 257])
def test_log_softmax_forward_backward_and_argmax(C, scale):
	"""one wave per row, lanes stride 64 over the classes, four rows per workgroup; at scale 30 the far classes underflow in exp"""
	from convasr_amd import ops
	d = dev()
	for B, T in ROWS:
		g_ = gen(1000 * C + 10 * B + T + scale)
		logits = torch.randn(B, C, T, generator = g_) * scale
		if C > 1 and T > 7:
			logits[0, C // 2, 7] = -INF  # one row with a single -inf logit: probability 0, log-probability -inf
		lp = ops.log_softmax(cl(logits, d))
		assert ops.is_cl(lp) and lp.shape == logits.shape
		close('log_softmax', lp, R.log_softmax(logits), f'C {C} rows {B * T}', cpu32 = F.log_softmax(logits, dim = 1))
		lp_h = lp.cpu()
		grad = torch.randn(B, C, T, generator = g_)
		dx = ops.log_softmax_bwd(cl(grad, d), lp)
		close('log_softmax_bwd', dx, R.log_softmax_bwd(grad, lp_h), f'C {C} rows {B * T}', cpu32 = grad - lp_h.exp() * grad.sum(dim = 1, keepdim = True))
		assert torch.equal(ops.log_softmax_bwd(grad.to(d), lp), dx), 'a torch-contiguous gradient goes through the layout kernel first'
		# argmax is exact on the values it is given, ties included (the lowest index): no element needs redrawing
		for src in (lp_h, logits):
			assert torch.equal(ops.argmax(cl(src, d)).cpu(), R.argmax(src)), f'argmax C {C} rows {B * T}'


def planted(C, plant, seed):
	"""(1, C, 9) log-probs: the planted row at rows 0, 3, 4, 8 (lanes of the first and the last wave of a workgroup, and a second workgroup), random finite rows between"""
	x = torch.randn(1, C, 9, generator = gen(seed)) * 3
	for r in (0, 3, 4, 8):
		if plant == 'all -inf':
			x[0, :, r] = -INF
		else:
			for c, v in plant:
				x[0, c, r] = v
	return x


ARGMAX_CASES = {
	'tie within a lane': (130, [(3, 9.0), (67, 9.0)]),
	'tie within a lane, three trips': (257, [(131, 9.0), (195, 9.0), (256, 8.0)]),
	'tie across lanes': (130, [(10, 9.0), (11, 9.0)]),
	'tie across the butterfly halves': (130, [(3, 9.0), (35, 9.0)]),
	'tie across the halves, higher index in the lower lane': (130, [(33, 9.0), (66, 9.0)]),
	'+inf tie': (130, [(40, INF), (100, INF)]),
	'all -inf': (130, 'all -inf'),
	'all -inf, one class': (1, 'all -inf'),
	'NaN at 0': (130, [(0, NAN)]),
	'NaN at 5': (130, [(5, NAN)]),
	'NaN at 37': (130, [(37, NAN)]),
	'NaN at 63': (130, [(63, NAN)]),
	'NaN at 64': (130, [(64, NAN)]),
	'NaN at 70': (130, [(70, NAN)]),
	'two NaNs': (130, [(70, NAN), (6, NAN)]),
	'two NaNs in one lane': (130, [(69, NAN), (5, NAN)]),
	'NaN at 5, finite maximum at 37': (38, [(5, NAN), (37, 50.0)]),
	'NaN and +inf': (130, [(129, NAN), (0, INF)]),
}


@pytest.mark.parametrize('name', list(ARGMAX_CASES))
def test_argmax_ties_infinities_and_nan(name):
	"""torch.argmax's rule: NaN above everything, the lowest index among equals; decoders call ops.argmax on GPU tensors and
	Tensor.argmax on CPU tensors, and the two must agree"""
	from convasr_amd import ops
	C, plant = ARGMAX_CASES[name]
	x = planted(C, plant, 17)
	ref = R.argmax(x)
	assert torch.equal(ref, x.argmax(dim = 1))
	got = ops.argmax(cl(x, dev())).cpu()
	assert torch.equal(got, ref), f'{name}: {got.tolist()} != {ref.tolist()}'


# ------------------------------------------------------------------------------------------------ entropies

# (C, T) with T C = 1, 1023, 1024, 1025, 2047, 2048, 2049, 3073, 38 x 211: around one and two trips of the 1024-thread, two-element walk
ENTROPY_SHAPES = [(1, 1), (33, 31), (32, 32), (41, 25), (23, 89), (64, 32), (683, 3), (7, 439), (38, 211)]


def log_probs(B, C, T, seed, scale = 3):
	"""normalised log-probs minus a little: the kernels take any values <= 0, and C = 1 would otherwise be all zeros"""
	g_ = gen(seed)
	return F.log_softmax(torch.randn(B, C, T, generator = g_) * scale, dim = 1) - 0.1 * torch.rand(B, C, T, generator = g_)


@pytest.mark.parametrize('C,T', ENTROPY_SHAPES)
def test_entropy(C, T):
	from convasr_amd import ops
	d = dev()
	lp = log_probs(6, C, T, C * 1000 + T)
	olen = torch.tensor([0, 1, T - 1, T, T + 5, (T + 1) // 2])  # a batch whose rows differ; T + 5: the sum stops at T, the divisor does not
	lpd = cl(lp, d)
	close('entropy', ops.entropy(lpd, olen.to(d)), R.entropy(lp, olen), f'C {C} T {T} olen {olen.tolist()}', cpu32 = O.entropy(lp, olen))
	close('entropy', ops.entropy(lpd), R.entropy(lp), f'C {C} T {T} no lengths', cpu32 = O.entropy(lp))
	close('entropy', ops.entropy(lp.to(d), olen.to(d), eps = 0.5), R.entropy(lp, olen, eps = 0.5), f'C {C} T {T} eps 0.5, torch-contiguous input')
	assert float(ops.entropy(lpd, olen.to(d))[0]) == 0.0


@pytest.mark.parametrize('C', [38, 64, 65, 129])
def test_weighted_mean_entropy(C):
	"""one wave per frame, 16 frames in flight, lane = class (stride 64)"""
	from convasr_amd import ops
	d = dev()
	T = 33
	olen = torch.tensor([0, 1, 15, 16, 17, 33])
	lp = log_probs(6, C, T, C)
	lpd = cl(lp, d)
	for eps_id in [-1, 0, 3, C - 1] + ([64] if C == 65 else [100] if C == 129 else []):
		for ol in (olen, None):
			close('weighted_entropy', ops.weighted_mean_entropy(lpd, None if ol is None else ol.to(d), eps_id = eps_id), R.weighted_mean_entropy(lp, ol, eps_id = eps_id),
			      f'C {C} eps_id {eps_id} olen {None if ol is None else ol.tolist()}', cpu32 = O.weighted_mean_entropy(lp, ol, eps_id = eps_id))
	assert float(ops.weighted_mean_entropy(lpd, olen.to(d))[0]) == 0.0
	# every frame puts almost all mass on eps_id: the weights 1 - p are ~4e-4, their sum over the frames is of the size of eps
	for eps_id in (C - 1, 3):
		logits = torch.randn(6, C, T, generator = gen(C + 7))
		logits[:, eps_id] += 12
		lq = F.log_softmax(logits, dim = 1)
		for ol in (olen, None):
			close('weighted_entropy', ops.weighted_mean_entropy(cl(lq, d), None if ol is None else ol.to(d), eps = 1e-2, eps_id = eps_id), R.weighted_mean_entropy(lq, ol, eps = 1e-2, eps_id = eps_id),
			      f'C {C} mass on eps_id {eps_id}, eps 1e-2', cpu32 = O.weighted_mean_entropy(lq, ol, eps = 1e-2, eps_id = eps_id))


# ------------------------------------------------------------------------------------------------ scale_rows, loss_head

@pytest.mark.parametrize('per_b', [1, 255, 256, 257, 64 * 256, 64 * 256 + 1, 3 * 64 * 256 + 7])
def test_scale_rows(per_b):
	"""256 elements per workgroup, at most 64 workgroups per row: a grid-stride loop from 64 x 256 + 1 elements on"""
	from convasr_amd import ops
	d = dev()
	for B in (1, 3):
		g_ = gen(per_b + B)
		grad = torch.randn(B, per_b, generator = g_)
		sc = torch.rand(B, generator = g_) + 0.5
		dv = torch.randint(1, 300, (B, 2), generator = g_)
		dvd = dv.to(d)[:, 0]  # a strided column
		assert B == 1 or dvd.stride(0) == 2
		for name, a, b in (('gscale', sc, None), ('gdiv', None, dv[:, 0]), ('both', sc, dv[:, 0])):
			out = ops.scale_rows(grad.to(d), None if a is None else a.to(d), None if b is None else dvd)
			s32 = (sc if a is not None else torch.ones(B)) / (dv[:, 0].float() if b is not None else torch.ones(B))
			close('scale_rows', out, R.scale_rows(grad, a, b), f'per_b {per_b} B {B} {name}', cpu32 = grad * s32.view(B, 1))
	if per_b == 257:  # a channels-last gradient: the strides are preserved, the rows are those of memory
		g_ = gen(2)
		grad, sc, dv = torch.randn(3, 5, 7, generator = g_), torch.rand(3, generator = g_) + 0.5, torch.randint(1, 300, (3, 2), generator = g_)
		gd = cl(grad, d)
		out = ops.scale_rows(gd, sc.to(d), dv.to(d)[:, 0])
		assert out.stride() == gd.stride() and ops.is_cl(out)
		close('scale_rows', out, R.scale_rows(grad, sc, dv[:, 0]), 'channels-last gradient')


@pytest.mark.parametrize('accum', [1, 4])
@pytest.mark.parametrize('B', [1, 2, 255, 256, 257, 600])
def test_loss_head(B, accum):
	"""one workgroup of 256 threads strides over the batch and adds in a tree; gvec is ((1 / accum) / B) * w * scale, exact in fp32"""
	from convasr_amd import ops
	import convasr_amd as ca
	d = dev()
	g_ = gen(B * 10 + accum)
	lv = torch.rand(B, generator = g_) * 5 + 0.1
	ylen2 = torch.randint(1, 200, (B, 2), generator = g_)
	ent = torch.rand(B, generator = g_)
	ylen, yd = ylen2[:, 0], ylen2.to(d)[:, 0]  # a strided column
	scaler = ca.train.LossScaler(d, init_scale = 4096.0)
	for what, kw, rkw in (('plain', dict(), dict()), ('entropy + metric_scale', dict(ent = ent.to(d), metric_scale = 0.25), dict(ent = ent, metric_scale = 0.25)),
	                      ('loss scaler', dict(ent = ent.to(d), loss_scaler = scaler.current), dict(ent = ent, loss_scale = 4096.0))):
		out3, gvec, skipped = ops.loss_head(lv.to(d), yd, accumulate_iterations = accum, **kw)
		r3, rg, rs = R.loss_head(lv, ylen, accum = accum, **rkw)
		cpu3 = torch.stack([(lv * ylen).mean() / accum, lv.mean() * rkw.get('metric_scale', 1.0), (ent.mean() if 'ent' in rkw else torch.zeros(())) * rkw.get('metric_scale', 1.0)])
		close('loss_head', out3, r3, f'B {B} accum {accum} {what}', cpu32 = cpu3)
		assert torch.equal(gvec.cpu(), rg), f'gvec {what}'
		assert bool(skipped) is rs is False
	out3, gvec, skipped = ops.loss_head(lv.to(d), yd, accumulate_iterations = accum, need_grad = False)
	assert gvec is None and not bool(skipped)
	close('loss_head', out3, R.loss_head(lv, ylen, accum = accum)[0], f'B {B} accum {accum} need_grad False')
	# skipped is 1 exactly when the mean loss is not finite
	for pos in sorted({0, B - 1, min(255, B - 1)}):
		for v in (INF, -INF, NAN):
			bad = lv.clone()
			bad[pos] = v
			out3, _, skipped = ops.loss_head(bad.to(d), yd, accumulate_iterations = accum)
			assert bool(skipped) is R.loss_head(bad, ylen, accum = accum)[2] is True and not math.isfinite(float(out3[1])), (pos, v)
	if B >= 2:
		bad = lv.clone()
		bad[0], bad[B - 1] = INF, -INF
		assert bool(ops.loss_head(bad.to(d), yd, accumulate_iterations = accum)[2]) is R.loss_head(bad, ylen, accum = accum)[2] is True


# ------------------------------------------------------------------------------------------------ output lengths

def near_integer_fractions(T, top):
	"""fractions whose fp32 product with T lies on an integer k <= top or within one ulp of it on either side, and 0 and 1"""
	k = torch.unique(torch.cat([torch.arange(0, min(top, 40) + 1), torch.linspace(0, top, 40).round().long()])).to(torch.float32)
	frac = k / T
	up, down = torch.nextafter(frac, torch.tensor(2.0)), torch.nextafter(frac, torch.tensor(-1.0)).clamp_min(0)
	return torch.cat([frac, up, down, torch.tensor([0.0, 1.0])])


@pytest.mark.parametrize('T', [1, 2, 753, 1501])
def test_output_lengths_near_integers(T):
	"""ceil(frac * T) with the product in fp32: exact, the reference's own expression"""
	from convasr_amd import ops
	d = dev()
	xlen = near_integer_fractions(T, T)
	ref = R.output_lengths(xlen, xlen.numel(), T)
	assert int(ref.min()) == 0 and int(ref.max()) >= T and len(set(ref.tolist())) >= min(T, 3)
	assert torch.equal(ops.output_lengths(xlen.to(d), xlen.numel(), T, d).cpu(), ref)
	assert torch.equal(ops.output_lengths(None, 5, T, d).cpu(), R.output_lengths(None, 5, T))
	# the same values through instnorm's mask (fractions that stay inside the T frames): frames from n on are exactly zero, those before it the normalised ones
	xl = near_integer_fractions(T, T - 1)
	xl = xl[R.output_lengths(xl, xl.numel(), T) <= T]
	x = torch.randn(xl.numel(), 2, T, generator = gen(T))
	y = ops.instnorm(cl(x, d), xl.to(d), 1e-5)
	ref = R.instnorm(x, xl, 1e-5)
	close('instnorm_f32', y, ref, f'T {T} mask of {xl.numel()} near-integer lengths')
	n = R.output_lengths(xl, xl.numel(), T)
	beyond = ~R.frame_mask(T, n).bool().unsqueeze(1).expand(-1, 2, -1)
	assert not bool(y.cpu()[beyond].any()), 'a frame at or beyond the valid length is not zero'
	if T > 2:
		nz = (y.cpu() != 0).any(dim = 1).sum(dim = 1)
		assert torch.equal(nz[n > 1], n[n > 1]), 'frames written'  # (n = 1: the one valid frame is its own mean)


# ------------------------------------------------------------------------------------------------ instance norm

def instnorm_input(B, C, T, dt, seed):
	g_ = gen(seed)
	return rep(torch.randn(B, C, T, generator = g_) * (torch.rand(1, C, 1, generator = g_) * 3 + 0.5) + torch.randn(1, C, 1, generator = g_) * 2, dt)


@pytest.mark.parametrize('T', [1, 63, 64, 65, 300])
@pytest.mark.parametrize('C', [1, 15, 16, 17, 64, 80])
def test_instnorm(C, T):
	"""16 channels x 64 time lanes per workgroup; the seven storage pairs; channels-last and torch-contiguous; masked (n = 0, 1, T and a fraction) and not"""
	from convasr_amd import ops
	d = dev()
	eps = 1e-5
	xlen = torch.tensor([0.0, 0.5 / T, 1.0, 0.61])
	assert R.output_lengths(xlen, 4, T).tolist()[:3] == [0, 1, T]
	for src, dst in PAIRS:
		sdt, ddt = DTYPES[src], DTYPES[dst]
		x = instnorm_input(4, C, T, sdt, C * 1000 + T)
		key = 'instnorm_' + dst
		cpu32 = lambda xl: None if src != 'f32' or dst != 'f32' else torch.nan_to_num(O.masked_instance_norm(x, None if xl is None else R.frame_mask(T, R.output_lengths(xl, 4, T)).bool(), eps), nan = 0.0)
		# channels-last in and out, one frame of time padding, masked
		y = ops.instnorm(cl(x, d, sdt), xlen.to(d), eps, out_dtype = ddt, pad_time_to = 2)
		Tp = T + T % 2
		assert y.shape == (4, C, Tp) and ops.is_cl(y) and y.dtype == ddt
		ref = R.instnorm(x, xlen, eps, T_out = Tp)
		close(key, y[:, :, :T], ref[:, :, :T], f'C {C} T {T} {src}->{dst} masked, channels-last', cpu32 = cpu32(xlen))
		assert not bool(y.cpu()[ref == 0].any()), 'masked frames and the padding frame must be exactly zero'
		assert not bool(y[0].any()) and (Tp == T or not bool(y[:, :, T:].any()))
		# torch-contiguous in and out (the legacy layout), no mask
		y = ops.instnorm(x.to(sdt).to(d), None, eps, out_dtype = ddt, channels_last = False)
		assert y.is_contiguous() and y.shape == (4, C, T)
		close(key, y, R.instnorm(x, None, eps), f'C {C} T {T} {src}->{dst} no mask, torch-contiguous', cpu32 = cpu32(None))
		# torch-contiguous in, channels-last out, masked
		y = ops.instnorm(x.to(sdt).to(d), xlen.to(d), eps, out_dtype = ddt)
		close(key, y, R.instnorm(x, xlen, eps), f'C {C} T {T} {src}->{dst} masked, mixed layouts')


def test_instnorm_two_pass_variance_far_from_zero_mean():
	"""per-channel mean 1e3, standard deviation 1: the two-pass variance holds where E[x^2] - E[x]^2 would not.  The bar is the condition of the
	problem, not a measurement: an error of u |mean| per step in the sum that gives the mean shifts x - mean by that, in units of std;
	chain = the additions of one lane (ceil(T / 64)) + the 64 lanes' sum + the division + the subtraction."""
	from convasr_amd import ops
	d = dev()
	B, C, T, mean, std, eps = 3, 17, 300, 1e3, 1.0, 1e-5
	x = mean * torch.tensor([1.0, -1.0]).repeat(9)[:C].view(1, C, 1) + std * torch.randn(B, C, T, generator = gen(3))
	bar = U32 * (1 + mean / std) * (math.ceil(T / 64) + 64 + 2)
	ref = R.instnorm(x, None, eps)
	assert 0.9 < float(ref.std()) < 1.1
	close('instnorm_f32', ops.instnorm(cl(x, d), None, eps), ref, f'mean 1e3 std 1 (bar {bar:.2e} from the condition)', cpu32 = O.masked_instance_norm(x, None, eps), bar = (bar, bar))
	xlen = torch.tensor([1.0, 0.5, 0.2])
	close('instnorm_f32', ops.instnorm(cl(x, d), xlen.to(d), eps), R.instnorm(x, xlen, eps), 'mean 1e3 std 1, masked', bar = (bar, bar))


def test_instnorm_constant_channels():
	"""variance 0 (constant channels) and variance 2^-20 (1 +- 2^-10, every sum exact in fp32): eps = 1e-5 decides the scale"""
	from convasr_amd import ops
	d = dev()
	B, C, T, eps = 2, 17, 65, 1e-5
	x = torch.full((B, C, T), 3.25)
	x[:, 1] = -7.0
	x[:, 2, ::2], x[:, 2, 1::2] = 1 + 2.0 ** -10, 1 - 2.0 ** -10
	x[:, 16] = 0.0
	for xlen in (None, torch.tensor([1.0, 0.5])):
		y = ops.instnorm(cl(x, d), None if xlen is None else xlen.to(d), eps)
		ref = R.instnorm(x, xlen, eps)
		close('instnorm_f32', y, ref, f'constant channels, xlen {xlen}')
		assert bool(torch.isfinite(y).all()) and not bool(y[:, [0, 1, 16]].any()) and 0.25 < float(ref[0, 2, 0]) < 0.31


@pytest.mark.parametrize('T', [1, 65, 300])
@pytest.mark.parametrize('C', [1, 17, 80])
def test_instnorm_running_statistics_and_fixed_statistics_eval(C, T):
	"""three training calls (momentum 0.1: batch mean of the instance means and of the unbiased variances, the biased one at T = 1, the counter
	counting), then eval mode on the running statistics with a frame of time padding"""
	from convasr_amd import ops
	d = dev()
	B, eps, mom = 3, 1e-5, 0.1
	g_ = gen(C * 100 + T)
	rm, rv, nbt = torch.randn(C, generator = g_), torch.rand(C, generator = g_) + 0.5, 0
	rmd, rvd, nbtd = rm.clone().to(d), rv.clone().to(d), torch.zeros(1, dtype = torch.int64, device = d)
	for call in range(3):
		x = instnorm_input(B, C, T, torch.float32, C * 100 + T + call + 1)
		y = ops.instnorm_running(cl(x, d), rmd, rvd, nbtd, mom, True, eps)
		ref, rm, rv, nbt = R.instnorm_running(x, rm, rv, nbt, mom, eps, True)
		close('instnorm_f32', y, ref, f'C {C} T {T} training call {call}')
		close('instnorm_running', rmd, rm, f'C {C} T {T} running_mean after call {call}')
		close('instnorm_running', rvd, rv, f'C {C} T {T} running_var after call {call}')
		assert int(nbtd) == nbt == call + 1
		rm, rv = rmd.cpu().clone(), rvd.cpu().clone()  # the next call starts from the fp32 values the kernel holds
	for src, dst in PAIRS:
		x = instnorm_input(B, C, T, DTYPES[src], 5)
		y = ops.instnorm_running(cl(x, d, DTYPES[src]), rmd, rvd, nbtd, mom, False, eps, out_dtype = DTYPES[dst], pad_time_to = 2)
		ref = R.instnorm_running(x, rm, rv, nbt, mom, eps, False, T_out = T + T % 2)[0]
		close('instnorm_' + dst, y, ref, f'C {C} T {T} {src}->{dst} eval on the running statistics')
		assert T % 2 == 0 or not bool(y[:, :, T:].any())
	assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv) and int(nbtd) == 3, 'eval mode writes nothing back'


# ------------------------------------------------------------------------------------------------ convert_layout

F16_SPECIALS = [-0.0, 0.0, 6e-8, 2.9e-8, 3.1e-8, 1e-7, 5.96e-8 * 1.5, 6.1e-5, 6.0e-5, 1e-40, 65504.0, 65519.9, 65520.0, 1e5, -7e4, 1 + 2.0 ** -11, 1 + 2.0 ** -10 + 2.0 ** -11, 3.3e38, -3.4e38, INF, -INF]


def layout_input(B, C, T, dt, seed):
	"""random values of the SOURCE type with the specials planted every 5th element: fp16 subnormals and their ties, fp16 / bf16 overflow, -0.0, infinities"""
	x = torch.randn(B * C * T, generator = gen(seed)) * 4
	sp = torch.tensor(F16_SPECIALS)
	idx = torch.arange(0, x.numel(), 5)
	x[idx] = sp[(idx // 5) % sp.numel()]
	return x.view(B, C, T).to(dt)


@pytest.mark.parametrize('src,dst', PAIRS)
def test_convert_layout(src, dst):
	"""64 x 64 tile through LDS: a pure permutation for equal types, exactly x.to(dtype) for a narrowing one, both directions, any source strides"""
	from convasr_amd import ops
	d = dev()
	sdt, ddt = DTYPES[src], DTYPES[dst]
	for C in (1, 63, 64, 65, 130):
		for T in (1, 63, 64, 65, 130):
			for B in (1, 3):
				x = layout_input(B, C, T, sdt, C * 131 + T + B)
				exp = R.convert_layout(x, ddt)
				to_cl = ops.convert(x.to(d), ddt, True)  # torch-contiguous -> channels-last
				assert to_cl.shape == x.shape and (to_cl.stride() == (T * C, 1, C)) and to_cl.dtype == ddt
				same_bits(to_cl, exp, f'{src}->{dst} to channels-last B {B} C {C} T {T}')
				back = ops.convert(cl(x, d), ddt, False)  # channels-last -> torch-contiguous
				assert back.is_contiguous()
				same_bits(back, exp, f'{src}->{dst} to torch-contiguous B {B} C {C} T {T}')
			# sources sliced along B, C and T out of a larger tensor: the first element is 1 + (T + 1) + (C + 1) (T + 1) elements in, not a multiple of 16 bytes
			big = layout_input(4, C + 1, T + 1, sdt, C + T)
			for what, sl in (('B', big[1:, :C, :T]), ('C', big[:3, 1:, :T]), ('T', big[:3, :C, 1:]), ('B, C and T', big[1:, 1:, 1:])):
				for big_d in (big.to(d), cl(big, d)):
					view = {'B': big_d[1:, :C, :T], 'C': big_d[:3, 1:, :T], 'T': big_d[:3, :C, 1:], 'B, C and T': big_d[1:, 1:, 1:]}[what]
					for to in (True, False):
						same_bits(ops.convert(view, ddt, to), R.convert_layout(sl, ddt), f'{src}->{dst} source sliced along {what}, C {C} T {T}')


# ------------------------------------------------------------------------------------------------ add16, cast_scale, copy

GRID_N = 8192 * 256 * 8  # elements one trip of the 8192-workgroup cap covers (8 per lane)
SIZES = [8, 16, 2040, 2048, GRID_N, GRID_N + 8]


def half_input(n, dt, seed, scale):
	"""random 16-bit values with subnormals, values whose sums / products overflow, infinities and a NaN planted"""
	x = (torch.randn(n, generator = gen(seed)) * scale).to(dt)
	tiny, big = (2.0 ** -24, 60000.0) if dt == torch.float16 else (2.0 ** -133, 3e38)
	sp = torch.tensor([tiny, -tiny, 3 * tiny, big, -big, INF, -INF, NAN, 0.0, -0.0, 1.0, 2.0 ** -11]).to(dt)
	idx = torch.arange(0, n, max(1, n // 4099) * 3 + 1)
	x[idx] = sp[torch.arange(idx.numel()) % sp.numel()]
	return x


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('half', ['bf16', 'f16'])
def test_add16(half, n):
	"""16 bytes per lane, at most 8192 workgroups: the last two sizes take a second grid-stride trip; bit-identical to the fp32 sum rounded once"""
	from convasr_amd import ops
	d, dt = dev(), DTYPES[half]
	a, b = half_input(n, dt, n, 100.0), half_input(n, dt, n + 1, 100.0).roll(5)
	exp = R.add16(a, b)
	ad, bd = a.to(d), b.to(d)
	same_bits(ops.add16(ad, bd), exp, f'add16 {half} n {n}')
	assert torch.equal(bits(ad), bits(a)) and torch.equal(bits(bd), bits(b)), 'inputs untouched'
	a2 = ad.clone()
	assert ops.add16(a2, bd, out = a2) is a2
	same_bits(a2, exp, f'add16 {half} n {n} in place, out == a')
	b2 = bd.clone()
	ops.add16(ad, b2, out = b2)
	same_bits(b2, exp, f'add16 {half} n {n} in place, out == b')


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('half', ['bf16', 'f16'])
def test_cast_scale(half, n):
	"""the two ends of a 16-bit gradient exchange: (x * scale) in fp32, rounded once into the destination"""
	from convasr_amd import _lib
	d, dt = dev(), DTYPES[half]
	s = _lib.stream_ptr()
	g_ = gen(n)
	x = torch.randn(n, generator = g_) * 50
	big = 3.4e38 if half == 'bf16' else 70000.0
	sp = torch.tensor([6e-8, 2.9e-8, -3.1e-8, 1e-40, -1e-40, 65504.0, 65519.9, 65520.0, big, -big, INF, -INF, NAN, -0.0, 1 + 2.0 ** -11, 1 + 2.0 ** -8 + 2.0 ** -9])
	idx = torch.arange(0, n, max(1, n // 4099) * 3 + 1)
	x[idx] = sp[torch.arange(idx.numel()) % sp.numel()]
	xd = x.to(d)
	for scale in (1.0, 0.125, 1.0 / 3.0, 1024.0):
		out = torch.full((n, ), 7.0, dtype = dt, device = d)
		_lib.call('convasr_cast_scale', _lib.ptr(xd), _lib.F32, _lib.ptr(out), _lib.dtype_code(dt), n, scale, s)
		same_bits(out, R.cast_scale(x, scale, dt), f'cast_scale f32->{half} n {n} scale {scale}')
	h = half_input(n, dt, n + 2, 100.0)
	hd = h.to(d)
	for scale in (1.0, 3.0, 2.0 ** -20):
		out = torch.full((n, ), 7.0, dtype = torch.float32, device = d)
		_lib.call('convasr_cast_scale', _lib.ptr(hd), _lib.dtype_code(dt), _lib.ptr(out), _lib.F32, n, scale, s)
		same_bits(out, R.cast_scale(h, scale, torch.float32), f'cast_scale {half}->f32 n {n} scale {scale}')


COPY_GRID = 4096 * 256 * 16  # bytes one trip of the 4096-workgroup cap covers on the 16-byte path


@pytest.mark.parametrize('nbytes', [0, 1, 15, 16, 17, 4096, COPY_GRID, COPY_GRID + 33])
def test_copy(nbytes):
	"""16 bytes per lane when source and destination are both 16-byte aligned (plus a byte tail), bytes otherwise; at most 4096 workgroups; the
	64 bytes on either side of the destination stay as they were"""
	from convasr_amd import _lib
	d = dev()
	src_h = torch.randint(0, 256, (nbytes + 16, ), generator = gen(nbytes + 1), dtype = torch.uint8)
	src_d = src_h.to(d)
	assert src_d.data_ptr() % 16 == 0
	guard = 64
	for so in (0, 1, 4, 16):
		for do in (0, 1, 4, 16):
			dst = torch.full((guard + 16 + nbytes + guard, ), 0xA5, dtype = torch.uint8, device = d)
			assert dst.data_ptr() % 16 == 0
			_lib.call('convasr_copy', src_d.data_ptr() + so, dst.data_ptr() + guard + do, nbytes, _lib.stream_ptr())
			exp = torch.full_like(dst, 0xA5, device = 'cpu')
			exp[guard + do:guard + do + nbytes] = R.copy(src_h[so:], nbytes)
			assert torch.equal(dst.cpu(), exp), f'copy of {nbytes} bytes, source offset {so}, destination offset {do}'


# ------------------------------------------------------------------------------------------------ collate_pad

@pytest.mark.parametrize('dtype', [torch.int16, torch.bfloat16, torch.float32, torch.int32, torch.int64])
@pytest.mark.parametrize('rows', [1, 64])
def test_collate_pad(rows, dtype):
	"""a ragged batch out of one packed buffer: the payload bit for bit, zeros behind it (element sizes 2, 4 and 8)"""
	from convasr_amd import _lib
	d = dev()
	for Tpad, lengths in ((300, [0, 1, 300, 17, 299]), (300, [300]), (300, [1]), (300, [0]), (2500, [2500, 0, 2049, 1, 255])):
		g_ = gen(Tpad + len(lengths) + rows)
		samples = [torch.randint(-30000, 30000, (rows, n), generator = g_).to(dtype) if not dtype.is_floating_point else torch.randn(rows, n, generator = g_).to(dtype) for n in lengths]
		packed = torch.cat([s.reshape(-1) for s in samples] + [torch.ones(1, dtype = dtype)])  # (one spare element: an all-empty batch still has a buffer)
		offsets = torch.tensor([0] + [s.numel() for s in samples], dtype = torch.int64).cumsum(0)[:-1]
		meta = torch.stack([offsets, torch.tensor(lengths, dtype = torch.int64)]).to(d)
		out = torch.empty(len(lengths), rows, Tpad, dtype = dtype, device = d)
		bits_view = out.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[dtype.itemsize])
		bits_view.fill_(0x5A5A)
		_lib.call('convasr_collate_pad', _lib.ptr(packed.to(d)), _lib.ptr(meta[0]), _lib.ptr(meta[1]), _lib.ptr(out), dtype.itemsize, len(lengths), rows, Tpad, _lib.stream_ptr())
		assert torch.equal(bits(out), bits(R.collate_pad(samples, rows, Tpad))), f'collate_pad {dtype} rows {rows} lengths {lengths}'


# ------------------------------------------------------------------------------------------------ normalize_signal, signal_absmax

@pytest.mark.parametrize('T', [1, 63, 64, 65, 4097, 3 * 8192 + 5])
def test_normalize_signal_and_absmax(T):
	"""per-row peak (16 bytes per lane on 16-byte aligned rows, elements otherwise; one atomic per workgroup, several workgroups per row from
	8193 samples on), then one scale_rows launch"""
	from convasr_amd import ops, _lib
	d = dev()
	g_ = gen(T)
	x = torch.rand(6, T, generator = g_) * 1.6 - 0.8
	x[1] = 0.0                      # an all-zero row
	x[2, 0] = 0.95                  # the peak at the first sample
	x[3, T - 1] = 0.97              # ... at the last
	x[4, T // 2] = -0.99            # a negative peak
	x16 = torch.randint(-20000, 20000, (6, T), generator = g_, dtype = torch.int16)
	x16[1] = 0
	x16[2, 0], x16[3, T - 1], x16[4, T // 2] = 32767, -32768, -32768
	for sig, name in ((x, 'fp32'), (x16, 'int16')):
		sd = sig.to(d)
		am = torch.empty(6, dtype = torch.float32, device = d)
		_lib.call('convasr_signal_absmax', _lib.ptr(sd), _lib.dtype_code(sig.dtype), 6, T, _lib.ptr(am), _lib.stream_ptr())
		assert torch.equal(am.cpu(), sig.float().abs().max(dim = -1).values), f'absmax {name} T {T}'  # exact: a maximum of magnitudes
		for m in (1.0, 2.5):
			out = ops.normalize_signal(sd, denom_multiplier = m)
			assert out.dtype == torch.float32 and out.shape == sig.shape
			close('normalize_signal', out, R.normalize_signal(sig, denom_multiplier = m), f'{name} T {T} multiplier {m}', cpu32 = O.normalize_signal(sig.float(), denom_multiplier = m))
			assert not bool(out[1].any())
