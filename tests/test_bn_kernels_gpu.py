"""The batch-norm / residual / activation kernels of convasr_amd/csrc/bn.hip on the MI355X against the float64 restatement
tests/_bn_ref.py (itself checked against torch.autograd in tests/test_bn_ref.py): every form of the forward, the two backward passes and
the finalize kernels, over a grid of channel counts and row counts chosen from row_walk_config / bn_bwd_config / RowWalk, for fp32, bf16
and fp16 storage, with xlen of 1, 0, one frame and None.

Inputs are exactly representable in the storage type, so the only errors are fp32 arithmetic and one rounding of the output.  Elements
whose float64 pre-activation lies within fp32 rounding of a gate boundary are redrawn BEFORE the comparison (draw_case), never excluded
after it; exact ties have bit-exact tests of their own (test_gate_boundaries_*).  Bars: the project's own for the same kind of quantity
(tests/test_kernels_gpu.py); every comparison is over every element; each check prints its measured maximum next to its bar."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = dict(f32 = torch.float32, bf16 = torch.bfloat16, f16 = torch.float16)
HALF = dict(bf16 = 4e-3, f16 = 6e-4)  # one output rounding (tests/test_kernels_gpu.py: HALF)
HALF_ATOL = 5e-5
DY_HALF = dict(bf16 = 1.2e-2, f16 = 1.5e-3)  # of max |dy| (test_dense_block_backward_sweep_from_gates_against_torch)
SEED, OFFSET = 1234, 77
ACTS = ['none', 'relu', 'hardtanh', 'leaky_relu']


def dev():
	return torch.device('cuda:0')


def rep(x, dt):
	"""the values of x that the storage type holds exactly, as fp32"""
	return x.to(dt).float()


def cl(t, dt, d):
	"""(B, T, C) host tensor -> the kernels' channels-last (B, C, T) device tensor"""
	return t.to(dt).to(d).contiguous().permute(0, 2, 1)


def rows(t):
	"""channels-last (B, C, T) device tensor -> (B, T, C) float64 on the host"""
	return t.permute(0, 2, 1).double().cpu()


def to(v, d):
	return None if v is None else v.to(d)


def report(what, err, bar):
	print(f'    {what}: {err:.3e} measured, bar {bar:.3e}')


def close(a, b, rtol, atol, what):
	a, b = a.detach().double().cpu(), b.detach().double().cpu()
	assert a.shape == b.shape, (what, a.shape, b.shape)
	assert bool(torch.isfinite(a).all()), what
	err, tol = (a - b).abs(), atol + rtol * b.abs()
	report(what + ' (worst err / tol)', float((err / tol).max()), 1.0)
	assert bool((err <= tol).all()), f'{what}: max abs err {float(err.max()):.3e}, worst excess {float((err - tol).max()):.3e}'


F32_EW = (8e-6, 8e-6)  # the project's bar for fp32 storage is rtol = atol = 1e-4 (test_bn_act_forward_backward); 2.0e-6 measured at worst over every z and g of this file: 4x that
F32_DY = (2.8e-5, 2.8e-6)  # the project's: 1e-3, 1e-4; 0.7 % of it measured at worst over every dy of this file: 4x that


def close_ew(a, b, dtn, what, f32_bar = F32_EW):
	"""elementwise outputs z, g: fp32 storage by fp32 arithmetic alone, 16-bit storage by one output rounding (0.97 / 0.81 of the bf16 / fp16 bar measured)"""
	close(a, b, *(f32_bar if dtn == 'f32' else (HALF[dtn], HALF_ATOL)), f'{what} [{dtn}]')


def close_dy(a, b, dtn, what):
	if dtn == 'f32':
		return close(a, b, *F32_DY, what + ' [f32]')  # (16-bit storage below: 0.30 of its bar measured)
	a, b = a.detach().double().cpu(), b.detach().double().cpu()
	err, bar = float((a - b).abs().max()), DY_HALF[dtn] * float(b.abs().max()) + HALF_ATOL
	report(f'{what} [{dtn}]', err, bar)
	assert bool(torch.isfinite(a).all()) and err <= bar, f'{what}: {err:.3e} > {bar:.3e}'


def close_sums(gpu_sg, gpu_sgx, sg, sgx, what):
	"""per-channel sums, dgamma, dbeta, rsums: the project's bar is 2e-5 * (max |sum g| + max |sum g xhat|) (test_dense_block_backward_sweep_from_gates_against_torch);
	4.0e-7 of that magnitude measured at worst over the three storage types and every case of this file, so the bar here is 4x that"""
	bar = 1.6e-6 * (float(sg.abs().max()) + float(sgx.abs().max())) + 1e-30
	for name, a, b in (('sum g', gpu_sg, sg), ('sum g xhat', gpu_sgx, sgx)):
		if a is None:
			continue
		a = a.detach().double().cpu()
		err = float((a - b).abs().max())
		report(f'{what} {name}', err, bar)
		assert bool(torch.isfinite(a).all()) and err <= bar, f'{what} {name}: {err:.3e} > {bar:.3e}'


def xlen_for(B, T, variant):
	"""variant 0: None; else utterance i takes entry i + variant - 1 of (all frames, none, one frame, two fractions)"""
	if variant == 0:
		return None
	pool = [1.0, 0.0, 0.5 / T, 0.61, 0.3]
	return torch.tensor([pool[(i + variant - 1) % len(pool)] for i in range(B)], dtype = torch.float32)


def unpack_gate(gate, B, T, C):
	"""(B * T * C / 8,) bytes -> (B, T, C) bool on the host: bit (element index & 7) of byte (element index >> 3)"""
	return ((gate.view(B, T, C // 8, 1) >> torch.arange(8, device = gate.device, dtype = torch.uint8)) & 1).reshape(B, T, C).bool().cpu()


def keep_scale(p):
	return 65536.0 / (65536 - round(p * 65536))


def keep_pattern(B, T, C, dt, p, d, seed = SEED, offset = OFFSET):
	"""The dropout keep tensor (0 / keep_scale, (B, T, C) float64) of the kernels' counter hash: one forward launch on ones, no activation."""
	from convasr_amd import ops, _lib
	if p == 0:
		return None
	# The hash is a function of the element index alone, so the launch is made on ONE utterance of B * T frames: no utterance edge for the row
	# walk to cross, nothing of the geometry under test in the reference.  The same launch on (B, T, C) must give the same pattern.
	k = rows(ops.bn_act(cl(torch.ones(1, B * T, C), dt, d), None, None, (_lib.ACT_NONE, 0.0, 0.0), dropout_p = p, seed = seed, offset = offset)).reshape(B, T, C)
	ks = float(torch.tensor(keep_scale(p), dtype = torch.float32).to(dt))  # (16-bit storage rounds the stored keep_scale; the kernels multiply by the fp32 one)
	assert bool(((k == 0) | (k == ks)).all())
	assert torch.equal(k, rows(ops.bn_act(cl(torch.ones(B, T, C), dt, d), None, None, (_lib.ACT_NONE, 0.0, 0.0), dropout_p = p, seed = seed, offset = offset))), 'keep pattern of (B, T, C) against (1, B T, C)'
	assert abs(float((k != 0).double().mean()) - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / k.numel()) + 1e-3, 'keep rate'
	return (k != 0).double() * float(torch.tensor(keep_scale(p), dtype = torch.float32))


class Case:
	pass


def draw_case(B, T, C, dt, nonlin, res_bn, affine, seed, redraw_share = 1e-4):
	"""res_bn: one bool per residual input (True: it comes with rscale / rshift and has a batch norm of its own in the backward).
	redraw_share None: no redraw (forward-only callers: z is continuous across a gate boundary, only the gate and g are not)."""
	gen = torch.Generator().manual_seed(seed)
	rn = lambda *s: torch.randn(*s, generator = gen)
	ru = lambda *s: torch.rand(*s, generator = gen)
	c = Case()
	c.y = rep(rn(B, T, C) * 8, dt)
	c.scale, c.shift = (ru(C) + 0.5, rn(C) * 4 + 4) if affine else (None, None)
	c.res = [rep(rn(B, T, C) * 2, dt) for _ in res_bn]
	c.rscale = [ru(C) + 0.5 if bn else None for bn in res_bn]
	c.rshift = [rn(C) if bn else None for bn in res_bn]
	c.mean, c.invstd, c.gamma = rn(C), ru(C) + 0.5, ru(C) + 0.5
	c.rmean = [rn(C) if bn else None for bn in res_bn]
	c.rinvstd = [ru(C) + 0.5 if bn else None for bn in res_bn]
	c.dz = rep(rn(B, T, C), dt)
	# no element within fp32 rounding of a gate boundary (the band is 40x the worst fp32 error of a four-term fused sum): redraw y there
	redrawn = 0
	for _ in range(20 if redraw_share is not None else 0):
		near = R.near_bound(c.y, c.scale, c.shift, c.res, c.rscale, c.rshift, nonlin)
		n = int(near.sum())
		if n == 0:
			break
		redrawn += n
		c.y[near] = rep(rn(n) * 8, dt)
	if redraw_share is not None:
		assert not bool(R.near_bound(c.y, c.scale, c.shift, c.res, c.rscale, c.rshift, nonlin).any())
		assert redrawn <= redraw_share * c.y.numel(), (redrawn, c.y.numel())
	return c


def run_case(B, T, C, dtn, act, res_bn, affine, p_drop, xvar, seed):
	"""Forward, both reduce forms (sums / coefficients), determinism, and the apply passes of one drawn case against the restatement."""
	from convasr_amd import ops
	d, dt, nonlin = dev(), DTYPES[dtn], R.NONLINS[act]
	a = ops.act_args(nonlin)
	n, n_res = B * T, len(res_bn)
	c = draw_case(B, T, C, dt, nonlin, res_bn, affine, seed)
	xlen = xlen_for(B, T, xvar)
	xd = to(xlen, d)
	keep = keep_pattern(B, T, C, dt, p_drop, d)
	drop = dict(dropout_p = p_drop, seed = SEED, offset = OFFSET)
	yd, dzd, resd = cl(c.y, dt, d), cl(c.dz, dt, d), [cl(r, dt, d) for r in c.res]
	scale, shift, mean, invstd, gamma = (to(v, d) for v in (c.scale, c.shift, c.mean, c.invstd, c.gamma))
	resargs = dict(res = resd, rscale = [to(v, d) for v in c.rscale], rshift = [to(v, d) for v in c.rshift]) if n_res else {}
	# ---- forward, with gate bits where the activation has a 0 / 1 derivative
	z_ref, pre = R.forward(c.y, c.scale, c.shift, c.res, c.rscale, c.rshift, nonlin, keep, xlen)
	g_ref, bits_ref = R.grad_pre(pre, nonlin, keep, xlen, c.dz)
	gate = torch.zeros(n * C // 8, dtype = torch.uint8, device = d) if act != 'leaky_relu' else None
	z = ops.bn_act(yd, scale, shift, a, xlen = xd, gate = gate, **resargs, **drop)
	close_ew(rows(z), z_ref, dtn, 'z')
	if gate is not None:
		assert torch.equal(unpack_gate(gate, B, T, C), bits_ref), 'gate bits'
		# the launch without gate bits is another instantiation of the kernel: held to the reference too, not to the bits of the first (in fp16 the
		# two differ by one rounding in ~1e-5 of the elements: hipcc fuses multiply and fp16 conversion into v_fma_mixlo_f16 in one and not the other)
		close_ew(rows(ops.bn_act(yd, scale, shift, a, xlen = xd, **resargs, **drop)), z_ref, dtn, 'z (launch without gate bits)')
	if xlen is not None:
		for b in range(B):
			if float(xlen[b]) == 0.0:
				assert not bool(z[b].any()) and not bool(g_ref[b].any())
	# ---- backward pass 1, re-derived: g + sums of the main batch norm and of the first two residuals that have one
	sg, sgx = R.bn_sums(g_ref, c.y, c.mean, c.invstd)
	rsum_idx = [r for r in range(min(n_res, 2)) if res_bn[r]]
	bwdargs = dict(resargs, rmean = [to(v, d) for v in c.rmean], rinvstd = [to(v, d) for v in c.rinvstd]) if n_res else {}
	outs = []
	for _ in range(2):
		sums = torch.full((2 * C, ), float('nan'), dtype = torch.float64, device = d)
		rsums = [torch.full((2 * C, ), float('nan'), dtype = torch.float64, device = d) if r in rsum_idx else None for r in range(n_res)]
		g = ops.bn_act_bwd_reduce(dzd, yd, scale, shift, mean, invstd, a, xlen = xd, sums = sums, **bwdargs, **(dict(rsums = rsums) if rsum_idx else {}), **drop)
		outs.append([g, sums] + [rsums[r] for r in rsum_idx])
	for u, v in zip(*outs):
		assert torch.equal(u, v), 'two launches of the reduce pass differ'
	g, sums = outs[0][:2]
	close_ew(rows(g), g_ref, dtn, 'g')
	close_sums(sums[:C], sums[C:], sg, sgx, 'main')
	for i, r in enumerate(rsum_idx):
		rsg, rsgx = R.bn_sums(g_ref, c.res[r], c.rmean[r], c.rinvstd[r])
		close_sums(outs[0][2 + i][:C], outs[0][2 + i][C:], rsg, rsgx, f'residual {r}')
	# ---- backward pass 1, coefficient form: no g, no sums; coef / dgamma / dbeta (accumulated onto what is there)
	A, Bc, D = R.bn_coef(sg, sgx, n, c.gamma, c.mean, c.invstd)
	coef_ref = torch.cat([A, Bc, D])
	forms = [('re-derived', None)] + ([('gated', gate)] if gate is not None and n_res == 0 else [])
	coefs = {}
	for name, gt in forms:
		for rep_ in range(2):
			coef, dgm, dbt = torch.full((3 * C, ), float('nan'), device = d), torch.full((C, ), 5.0, device = d), torch.full((C, ), -5.0, device = d)
			kw = dict(bwdargs, **drop) if gt is None else dict(drop, gate = gt)
			assert ops.bn_act_bwd_reduce(dzd, yd, scale, shift, mean, invstd, a, xlen = xd, write_g = False, gamma = gamma, coef = coef, dgamma = dgm, dbeta = dbt, accumulate = True, **kw) is None
			if rep_:
				assert torch.equal(coef, coefs[name][0]) and torch.equal(dgm, coefs[name][1]) and torch.equal(dbt, coefs[name][2]), f'two launches of the {name} coefficient pass differ'
			coefs[name] = (coef, dgm, dbt)
		close(coef, coef_ref, 1e-4, 1e-5, f'coef ({name})')
		close_sums(dbt.double() + 5.0, dgm.double() - 5.0, sg, sgx, f'dbeta / dgamma ({name}, accumulate)')
	if gate is not None and n_res == 0:  # the gated form with fp64 sums out instead of coefficients (bn_bwd_finalize_kernel: sets.dst[0] set)
		outs = []
		for _ in range(2):
			sums_g = torch.full((2 * C, ), float('nan'), dtype = torch.float64, device = d)
			assert ops.bn_act_bwd_reduce(dzd, yd, scale, shift, mean, invstd, a, xlen = xd, write_g = False, sums = sums_g, gate = gate, **drop) is None
			outs.append(sums_g)
		assert torch.equal(outs[0], outs[1]), 'two launches of the gated sums pass differ'
		close_sums(outs[0][:C], outs[0][C:], sg, sgx, 'main (gated, sums out)')
	# ---- backward pass 2
	gen = torch.Generator().manual_seed(seed + 1)
	cf = torch.randn(3 * C, generator = gen)
	cA, cB, cD = R.f64(cf[:C]), R.f64(cf[C:2 * C]), R.f64(cf[2 * C:])
	dy = ops.bn_act_bwd_apply(g, yd, cf.to(d), False)
	close_dy(rows(dy), cA * rows(g) + cB * R.f64(c.y) + cD, dtn, 'dy = A g + B y + D (g given)')
	if n_res == 0:  # (the apply pass re-derives g of a residual-free layer only)
		dy_ref = cA * g_ref + cB * R.f64(c.y) + cD
		dy = ops.bn_act_bwd_apply(dzd, yd, cf.to(d), True, scale, shift, a, xlen = xd, **drop)
		close_dy(rows(dy), dy_ref, dtn, 'dy (g re-derived from dz)')
		if gate is not None:
			dy = ops.bn_act_bwd_apply(dzd, yd, cf.to(d), True, scale, shift, a, xlen = xd, gate = gate, **drop)
			close_dy(rows(dy), dy_ref, dtn, 'dy (g from the stored gates)')
	dy_ref = R.bn_dy(rows(g), c.y, c.gamma, c.mean, c.invstd, sg, sgx)
	sums_ref = torch.cat([sg, sgx]).to(d)
	dgm, dbt = torch.full((C, ), 5.0, device = d), torch.full((C, ), -5.0, device = d)
	dy = ops.bn_bwd_apply(g, yd, gamma, mean, invstd, sums_ref, dgm, dbt, accumulate = True, inplace = False)
	assert dy.data_ptr() != g.data_ptr()
	close_dy(rows(dy), dy_ref, dtn, 'bn_bwd_apply, out of place')
	close(dgm - 5.0, sgx, 1e-5, 1e-5, 'bn_bwd_apply dgamma (accumulate)')
	close(dbt + 5.0, sg, 1e-5, 1e-5, 'bn_bwd_apply dbeta (accumulate)')
	g2 = g.clone(memory_format = torch.preserve_format)
	dy2 = ops.bn_bwd_apply(g2, yd, gamma, mean, invstd, sums_ref)
	assert dy2.data_ptr() == g2.data_ptr() and torch.equal(dy2, dy), 'bn_bwd_apply in place'


# ------------------------------------------------------------------------------------------------ geometry grid
# C: 8, 40: rlanes = 256 / 51 (more row-lanes than frames for small T; a 255-thread block).  200, 384, 640, 896: cgroups = 25 / 48 / 80 / 112
# (block sizes 250 / 240 / 240 / 224).  768, 1024: the benchmark widths (rlanes 2 / 1).  1032: cgroups 129, rlanes 1.  2560: gridDim.y = 2
# with a ragged second channel block.  8200: c8 = 1025 > 4 x 256, the cbase loop takes a second trip for one channel group.
# (B, T): (1, 1); (7, 3): T < rlanes, all rows in a thread's first step (C = 8, 40) or one utterance crossed per step; (200, 3) / (40, 3) / (60, 3)
# at C = 8 / 40 / 200 (rlanes 256 / 51 / 10): T < rlanes AND B T > rlanes, so a thread's second and later steps are live and each crosses
# several utterances (RowWalk::next's while loop; the only other case that needs it is (384, 7, 3), rlanes 5); (3, 57); (5, 611): several workgroups, a ragged
# last one, utterance edges inside a thread's stride; (24, 601) / (13, 950): more than 768 x rows_per_block rows, the capped backward grid.
GEOMETRY = [
	(8, 1, 1), (8, 7, 3), (8, 5, 611), (40, 7, 3), (40, 3, 57), (40, 5, 611), (200, 3, 57), (200, 5, 611), (384, 7, 3), (384, 5, 611), (640, 1, 1), (640, 3, 57),
	(896, 7, 3), (896, 5, 611), (768, 3, 57), (768, 24, 601), (1024, 5, 611), (1024, 13, 950), (1032, 1, 1), (1032, 3, 57), (2560, 7, 3), (2560, 3, 57), (8200, 3, 57), (8200, 7, 3),
	(8, 200, 3), (40, 40, 3), (200, 60, 3),
]
CAPPED = {(768, 24, 601): (20, 722), (1024, 13, 950): (18, 687)}  # -> (rows per block, blocks) of bn_bwd_config


def test_capped_grid_cases_take_the_capped_path():
	from convasr_amd import _lib
	lib = _lib.load()
	for (C, B, T), (rpb, blocks) in CAPPED.items():
		rlanes = 256 // min(C // 8, 256)
		got = lib.convasr_bn_bwd_workspace_bytes(B, T, C) // (3 * 2 * C * 4)
		assert got <= 768 and got != math.ceil(B * T / (8 * rlanes)) and got == blocks == math.ceil(B * T / rpb), (C, B, T, got)
	for C, B, T in GEOMETRY:
		if (C, B, T) not in CAPPED:
			rlanes = 256 // min(C // 8, 256)
			assert lib.convasr_bn_bwd_workspace_bytes(B, T, C) // (3 * 2 * C * 4) == math.ceil(B * T / (8 * rlanes))


@pytest.mark.parametrize('dtn', list(DTYPES))
@pytest.mark.parametrize('geom', GEOMETRY, ids = lambda g: 'C%d-B%d-T%d' % g)
def test_geometry_grid(geom, dtn):
	"""Every form on every geometry; the activation, the residual form, main scale / shift, dropout and xlen rotate with the case so that
	each (C, rows) pair meets different ones for the three storage types."""
	C, B, T = geom
	i = GEOMETRY.index(geom) + list(DTYPES).index(dtn)
	big = B * T * C > 4e6
	res_forms = [(), (True, False), (True, True), (False, True, False)] if not big else [(), (True, ), (False, True), (True, True)]
	run_case(B, T, C, dtn, ACTS[i % 4], res_forms[(i // 2) % 4], affine = i % 5 != 0, p_drop = 0.2 if i % 3 else 0.0, xvar = i % 4, seed = 100 + i)


@pytest.mark.parametrize('dtn', list(DTYPES))
@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('res_bn', [(), (True, True), (False, True, True)], ids = ['nores', 'res-bn-bn', 'res-plain-bn-bn'])
def test_every_activation_and_storage_type(act, dtn, res_bn):
	"""(5, 611, 384) of the issue's band count (60 % of the elements inside (0, 20)): both gate values well populated."""
	run_case(5, 611, 384, dtn, act, res_bn, affine = True, p_drop = 0.2, xvar = 1, seed = 7)
	run_case(7, 3, 40, dtn, act, res_bn, affine = True, p_drop = 0.0, xvar = 2, seed = 8)


# ------------------------------------------------------------------------------------------------ dropout keep pattern
def test_keep_pattern_values_storage_types_and_offsets():
	from convasr_amd import ops, _lib
	d = dev()
	for (B, T, C), p in (((5, 611, 384), 0.2), ((7, 3, 40), 0.5), ((3, 57, 8200), 0.2)):
		pats = {}
		for dtn, dt in DTYPES.items():
			k = rows(ops.bn_act(cl(torch.ones(B, T, C), dt, d), None, None, (_lib.ACT_NONE, 0.0, 0.0), dropout_p = p, seed = SEED, offset = OFFSET))
			pats[dtn] = k != 0
			if dtn == 'f32':
				want = float(torch.tensor(65536.0 / (65536 - round(p * 65536)), dtype = torch.float32))
				assert bool(((k == 0) | (k == want)).all()), 'every kept element is 65536 / (65536 - round(p * 65536)) exactly'
		assert torch.equal(pats['f32'], pats['bf16']) and torch.equal(pats['f32'], pats['f16'])
		rate = float(pats['f32'].double().mean())
		assert abs(rate - (1 - p)) < 4 * math.sqrt(p * (1 - p) / (B * T * C)) + 1e-3, rate
		other = keep_pattern(B, T, C, torch.float32, p, d, offset = OFFSET + 1)
		assert not torch.equal(other != 0, pats['f32'])
		assert torch.equal(keep_pattern(B, T, C, torch.float32, p, d) != 0, pats['f32'])


# ------------------------------------------------------------------------------------------------ forward: many residuals
@pytest.mark.parametrize('dtn', list(DTYPES))
@pytest.mark.parametrize('n_res', [1, 3, 12])
def test_forward_with_many_residuals(n_res, dtn):
	"""n_res 1 / 3 / 12 with scales on all, none, and alternating residuals; with and without the main scale / shift."""
	from convasr_amd import ops
	d, dt = dev(), DTYPES[dtn]
	B, T, C = 3, 57, 200
	for k, (act, pattern, affine) in enumerate([('hardtanh', 'all', True), ('relu', 'none', False), ('leaky_relu', 'mixed', True), ('none', 'mixed', False)]):
		res_bn = tuple(dict(all = True, none = False, mixed = r % 2 == 0)[pattern] for r in range(n_res))
		nonlin = R.NONLINS[act]
		c = draw_case(B, T, C, dt, nonlin, res_bn, affine, 300 + 10 * n_res + k, redraw_share = None)
		xlen = xlen_for(B, T, 1 + k % 3)
		p = 0.2 if k % 2 == 0 else 0.0
		keep = keep_pattern(B, T, C, dt, p, d)
		z_ref, _ = R.forward(c.y, c.scale, c.shift, c.res, c.rscale, c.rshift, nonlin, keep, xlen)
		rscale = [to(v, d) for v in c.rscale] if pattern != 'none' else ()
		rshift = [to(v, d) for v in c.rshift] if pattern != 'none' else ()
		z = ops.bn_act(cl(c.y, dt, d), to(c.scale, d), to(c.shift, d), ops.act_args(nonlin), xlen = to(xlen, d), res = [cl(r, dt, d) for r in c.res], rscale = rscale, rshift = rshift, dropout_p = p, seed = SEED, offset = OFFSET)
		close_ew(rows(z), z_ref, dtn, f'z, {n_res} residuals ({pattern})')


# ------------------------------------------------------------------------------------------------ residual sum sets
@pytest.mark.parametrize('dtn', list(DTYPES))
def test_reduce_residual_sum_sets_land_in_their_own_slots(dtn):
	"""rsums for residual 1 only, for none of three, for both with the main batch norm's sums left out; a third is refused."""
	from convasr_amd import ops, _lib
	d, dt = dev(), DTYPES[dtn]
	B, T, C = 5, 611, 200
	nonlin = R.NONLINS['hardtanh']
	a = ops.act_args(nonlin)
	c = draw_case(B, T, C, dt, nonlin, (True, True, True), True, 41)
	xlen = xlen_for(B, T, 1)
	keep = keep_pattern(B, T, C, dt, 0.2, d)
	_, pre = R.forward(c.y, c.scale, c.shift, c.res, c.rscale, c.rshift, nonlin, keep, xlen)
	g_ref, _ = R.grad_pre(pre, nonlin, keep, xlen, c.dz)
	dv = lambda v: to(v, d)
	common = dict(xlen = dv(xlen), res = [cl(r, dt, d) for r in c.res], rscale = [dv(v) for v in c.rscale], rshift = [dv(v) for v in c.rshift], rmean = [dv(v) for v in c.rmean], rinvstd = [dv(v) for v in c.rinvstd], dropout_p = 0.2, seed = SEED, offset = OFFSET)
	yd, dzd = cl(c.y, dt, d), cl(c.dz, dt, d)
	main = (dv(c.scale), dv(c.shift), dv(c.mean), dv(c.invstd))
	sg, sgx = R.bn_sums(g_ref, c.y, c.mean, c.invstd)
	fresh = lambda: torch.full((2 * C, ), float('nan'), dtype = torch.float64, device = d)
	for want in ((1, ), (), (0, 1)):
		sums, rsums = fresh(), [fresh() if r in want else None for r in range(3)]
		g = ops.bn_act_bwd_reduce(dzd, yd, *main, a, sums = sums, rsums = rsums, **common)
		close_ew(rows(g), g_ref, dtn, f'g, rsums {want}')
		close_sums(sums[:C], sums[C:], sg, sgx, f'main, rsums {want}')
		for r in want:
			rsg, rsgx = R.bn_sums(g_ref, c.res[r], c.rmean[r], c.rinvstd[r])
			close_sums(rsums[r][:C], rsums[r][C:], rsg, rsgx, f'residual {r}, rsums {want}')
	# no main batch norm (mean / invstd None): only the residual sets are written
	rsums = [fresh(), fresh(), None]
	g = ops.bn_act_bwd_reduce(dzd, yd, main[0], main[1], None, None, a, rsums = rsums, **common)
	close_ew(rows(g), g_ref, dtn, 'g, no main batch norm')
	for r in (0, 1):
		rsg, rsgx = R.bn_sums(g_ref, c.res[r], c.rmean[r], c.rinvstd[r])
		close_sums(rsums[r][:C], rsums[r][C:], rsg, rsgx, f'residual {r}, no main batch norm')
	# a third batch-normed residual is refused before anything is launched
	sums, rsums = fresh(), [fresh(), fresh(), fresh()]
	# (CONVASR_EUNSUPPORTED: ConvasrHipError carries the C side's message, not its code, so the refusal is told apart by its text)
	with pytest.raises(_lib.ConvasrHipError, match = 'beyond the first two'):
		ops.bn_act_bwd_reduce(dzd, yd, *main, a, sums = sums, rsums = rsums, **common)
	torch.cuda.synchronize()
	assert all(bool(torch.isnan(t).all()) for t in [sums] + rsums), 'a refused call wrote something'


@pytest.mark.parametrize('dtn', list(DTYPES))
@pytest.mark.parametrize('shape', [(5, 611, 384), (7, 3, 40), (24, 601, 768)], ids = lambda s: 'B%d-T%d-C%d' % s)
def test_reduce_alias_form_of_the_dense_block_backward(shape, dtn):
	"""The extra passes of a dense block's backward: dz and y are the SAME tensor (g), no scale, no mean, no activation, only residual sums."""
	from convasr_amd import ops, _lib
	d, dt = dev(), DTYPES[dtn]
	B, T, C = shape
	gen = torch.Generator().manual_seed(C + T)
	g_host = rep(torch.randn(B, T, C, generator = gen), dt)
	g_host[:, T // 2:] = 0  # (g of a masked batch: zero rows contribute nothing)
	res = [rep(torch.randn(B, T, C, generator = gen) * 2 + 1, dt) for _ in range(2)]
	rmean, rinvstd = [torch.randn(C, generator = gen) for _ in res], [torch.rand(C, generator = gen) + 0.5 for _ in res]
	gd = cl(g_host, dt, d)
	before = gd.clone(memory_format = torch.preserve_format)
	for batch in ((0, 1), (1, )):
		outs = []
		for _ in range(2):
			rsums = [torch.full((2 * C, ), float('nan'), dtype = torch.float64, device = d) for _ in batch]
			assert ops.bn_act_bwd_reduce(gd, gd, None, None, None, None, (_lib.ACT_NONE, 0.0, 0.0), res = [cl(res[r], dt, d) for r in batch], rscale = [None] * len(batch), rshift = [None] * len(batch),
				rmean = [rmean[r].to(d) for r in batch], rinvstd = [rinvstd[r].to(d) for r in batch], rsums = rsums, write_g = False) is None
			outs.append(rsums)
		assert torch.equal(gd, before), 'the alias form wrote to g'
		for i, r in enumerate(batch):
			assert torch.equal(outs[0][i], outs[1][i])
			rsg, rsgx = R.bn_sums(R.f64(g_host), res[r], rmean[r], rinvstd[r])
			close_sums(outs[0][i][:C], outs[0][i][C:], rsg, rsgx, f'alias form, residual {r} of {batch}')


# ------------------------------------------------------------------------------------------------ finalize kernels
def make_stats(y64, pieces, d):
	"""A ConvStats holding the (sum, sum of squares) partial rows of y64's rows cut into `pieces` contiguous pieces (built in float64)"""
	from convasr_amd import ops
	n, C = y64.shape
	edges = [round(i * n / pieces) for i in range(pieces + 1)]
	part = torch.stack([torch.stack([y64[a:b].sum(0), (y64[a:b] ** 2).sum(0)]) for a, b in zip(edges[:-1], edges[1:])])  # (pieces, 2, C)
	s = ops.ConvStats.__new__(ops.ConvStats)
	s.C, s.max_rows, s.rows, s.buf = C, pieces, pieces, part.reshape(-1).to(d)
	return s


@pytest.mark.parametrize('C', [8, 40, 200, 1024])
@pytest.mark.parametrize('pieces', [1, 63, 64, 65, 200])
def test_bn_finalize_partial_rows(C, pieces):
	from convasr_amd import ops
	d = dev()
	gen = torch.Generator().manual_seed(C + pieces)
	n, eps, momentum = 400, 1e-5, 0.1
	y = torch.randn(n, C, generator = gen, dtype = torch.float64) * (torch.rand(C, generator = gen, dtype = torch.float64) * 3 + 0.1) + torch.randn(C, generator = gen, dtype = torch.float64) * 2
	y[:, 3] = 2.5  # a constant channel: E[x^2] - m^2 is 0 (or rounds below it): the variance clamps at 0
	stats = make_stats(y, pieces, d)
	for with_affine in (True, False):
		gamma, beta = (torch.rand(C, generator = gen) + 0.5, torch.randn(C, generator = gen)) if with_affine else (None, None)
		rm, rv = torch.randn(C, generator = gen), torch.rand(C, generator = gen) + 0.5
		ref = R.finalize(y.sum(0), (y ** 2).sum(0), n, gamma, beta, rm, rv, momentum, eps)
		rm_d, rv_d, nbt = rm.to(d), rv.to(d), torch.tensor(41, dtype = torch.int64, device = d)
		out = ops.bn_finalize(stats, n, to(gamma, d), to(beta, d), rm_d, rv_d, momentum, eps, num_batches_tracked = nbt)
		assert int(nbt) == 42
		assert torch.equal(out, ops.bn_finalize(stats, n, to(gamma, d), to(beta, d), rm.to(d), rv.to(d), momentum, eps, num_batches_tracked = nbt)) and int(nbt) == 43
		for i, name in enumerate(('mean', 'invstd', 'scale', 'shift')):
			close(out[i], ref[name], 2e-6, 2e-6, f'bn_finalize {name}')  # fp32 roundings of a float64 result: a few 2^-24
		close(rm_d, ref['running_mean'], 2e-6, 1e-6, 'running_mean')
		close(rv_d, ref['running_var'], 2e-6, 1e-6, 'running_var')
		assert float(out[1][3]) == float(1.0 / torch.sqrt(torch.tensor(0.0, dtype = torch.float32) + torch.tensor(eps, dtype = torch.float32))), 'invstd of a constant channel is 1 / sqrt(eps) as fp32 evaluates it'
		assert float(out[0][3]) == 2.5


def test_bn_finalize_single_element_and_plain_totals():
	from convasr_amd import ops
	d = dev()
	C = 40
	y = torch.randn(1, C, dtype = torch.float64)
	totals = torch.cat([y[0], y[0] ** 2]).to(d)  # the (2 C,) fp64 form of the stats argument
	rm, rv = torch.zeros(C, device = d), torch.ones(C, device = d)
	out = ops.bn_finalize(totals, 1, None, None, rm, rv, 0.1, 1e-5)
	ref = R.finalize(y[0], y[0] ** 2, 1, None, None, torch.zeros(C), torch.ones(C), 0.1, 1e-5)
	for i, name in enumerate(('mean', 'invstd', 'scale', 'shift')):
		close(out[i], ref[name], 2e-6, 2e-6, f'bn_finalize n = 1 {name}')
	close(rv, ref['running_var'], 2e-6, 1e-6, 'running_var, n = 1 (no division by n - 1)')
	close(rm, ref['running_mean'], 2e-6, 1e-6, 'running_mean, n = 1')


def test_grouped_finalize_kernels_equal_single_calls_bit_for_bit():
	from convasr_amd import ops
	d = dev()
	K, C, n, pieces = 13, 200, 400, 65
	gen = torch.Generator().manual_seed(5)
	rn = lambda *s: torch.randn(*s, generator = gen)
	ys = [torch.randn(n, C, generator = gen, dtype = torch.float64) * (k + 1) + k for k in range(K)]
	stats = [make_stats(y, pieces, d) for y in ys]
	gammas, betas = [(torch.rand(C, generator = gen) + 0.5).to(d) if k % 3 else None for k in range(K)], [rn(C).to(d) if k % 3 else None for k in range(K)]
	rms, rvs = [rn(C) for _ in range(K)], [torch.rand(C, generator = gen) + 0.5 for _ in range(K)]
	momenta, epss = [0.1 + 0.01 * k for k in range(K)], [1e-5 * (k + 1) for k in range(K)]
	rm1, rv1, nbt1 = [t.to(d) for t in rms], [t.to(d) for t in rvs], [torch.tensor(k, dtype = torch.int64, device = d) for k in range(K)]
	rm2, rv2, nbt2 = [t.to(d) for t in rms], [t.to(d) for t in rvs], [torch.tensor(k, dtype = torch.int64, device = d) for k in range(K)]
	grouped = ops.bn_finalize_grouped(stats, n, gammas, betas, rm1, rv1, momenta, epss, nbt1)
	for k in range(K):
		single = ops.bn_finalize(stats[k], n, gammas[k], betas[k], rm2[k], rv2[k], momenta[k], epss[k], num_batches_tracked = nbt2[k])
		assert torch.equal(grouped[k], single) and torch.equal(rm1[k], rm2[k]) and torch.equal(rv1[k], rv2[k]) and int(nbt1[k]) == int(nbt2[k]) == k + 1, k
		ref = R.finalize(ys[k].sum(0), (ys[k] ** 2).sum(0), n, gammas[k], betas[k], rms[k], rvs[k], momenta[k], epss[k])
		close(single[1], ref['invstd'], 2e-6, 2e-6, f'invstd of batch norm {k}')
	# backward: (2 C,) fp64 totals each
	sums = [torch.randn(2 * C, generator = gen, dtype = torch.float64).to(d) * 50 for _ in range(K)]
	means, invstds = [rn(C).to(d) for _ in range(K)], [(torch.rand(C, generator = gen) + 0.5).to(d) for _ in range(K)]
	acc = [k % 2 for k in range(K)]
	mk = lambda: ([torch.full((3 * C, ), float('nan'), device = d) for _ in range(K)], [torch.full((C, ), 5.0, device = d) for _ in range(K)], [torch.full((C, ), -5.0, device = d) for _ in range(K)])
	(c1, dg1, db1), (c2, dg2, db2) = mk(), mk()
	ops.bn_bwd_finalize_grouped(sums, gammas, means, invstds, n, c1, dg1, db1, acc)
	for k in range(K):
		ops.bn_bwd_finalize(sums[k], gammas[k], means[k], invstds[k], n, coef = c2[k], dgamma = dg2[k], dbeta = db2[k], accumulate = bool(acc[k]))
		assert torch.equal(c1[k], c2[k]) and torch.equal(dg1[k], dg2[k]) and torch.equal(db1[k], db2[k]), k
		A, Bc, D = R.bn_coef(sums[k][:C].cpu(), sums[k][C:].cpu(), n, gammas[k], means[k], invstds[k])
		close(c2[k], torch.cat([A, Bc, D]), 1e-4, 1e-5, f'coef of batch norm {k}')
		close(dg2[k] - (5.0 if acc[k] else 0.0), sums[k][C:], 1e-6, 1e-5, f'dgamma of batch norm {k}')
		close(db2[k] + (5.0 if acc[k] else 0.0), sums[k][:C], 1e-6, 1e-5, f'dbeta of batch norm {k}')


@pytest.mark.parametrize('C', [8, 40, 200])
@pytest.mark.parametrize('pieces', [1, 63, 64, 65, 200])
def test_bn_bwd_finalize_from_partial_rows_and_reduce_rows(C, pieces):
	from convasr_amd import ops, _lib
	d = dev()
	gen = torch.Generator().manual_seed(C * 7 + pieces)
	part = torch.randn(pieces, 2, C, generator = gen, dtype = torch.float64) * 10
	s = ops.ConvStats.__new__(ops.ConvStats)
	s.C, s.max_rows, s.rows, s.buf = C, pieces, pieces, part.reshape(-1).to(d)
	tot = part.sum(0)
	close(s.totals(), tot.reshape(-1), 1e-14, 1e-12, 'reduce_rows')
	assert torch.equal(s.totals(), s.totals())
	n = 1000
	gamma, mean, invstd = torch.rand(C, generator = gen) + 0.5, torch.randn(C, generator = gen), torch.rand(C, generator = gen) + 0.5
	coef, dgm, dbt = torch.empty(3 * C, device = d), torch.empty(C, device = d), torch.empty(C, device = d)
	ops.bn_bwd_finalize(s, gamma.to(d), mean.to(d), invstd.to(d), n, coef = coef, dgamma = dgm, dbeta = dbt)
	close(coef, torch.cat(R.bn_coef(tot[0], tot[1], n, gamma, mean, invstd)), 1e-4, 1e-5, 'coef from partial rows')
	close(dgm, tot[1], 1e-6, 1e-5, 'dgamma from partial rows')
	close(dbt, tot[0], 1e-6, 1e-5, 'dbeta from partial rows')


def test_bn_eval_scale_shift():
	from convasr_amd import ops
	d = dev()
	for C in (8, 40, 257, 1024):
		gen = torch.Generator().manual_seed(C)
		gamma, beta, rm, rv = torch.rand(C, generator = gen) + 0.5, torch.randn(C, generator = gen), torch.randn(C, generator = gen), torch.rand(C, generator = gen) * 4
		for gm, bt in ((gamma, beta), (None, None)):
			sc, sh = R.eval_scale_shift(gm, bt, rm, rv, 1e-5)
			out = ops.bn_eval_scale_shift(to(gm, d), to(bt, d), rm.to(d), rv.to(d), 1e-5)
			close(out[0], sc, 2e-6, 0.0, 'eval scale')
			close(out[1], sh, 2e-6, 2e-6, 'eval shift')


# ------------------------------------------------------------------------------------------------ boundary semantics
def torch_act_and_grad(pre, nonlin, dz):
	"""what F.relu / F.hardtanh / F.leaky_relu and their autograd give in float64 at these pre-activations"""
	p = pre.double().clone().requires_grad_(True)
	z = R.activation(p, nonlin)
	(g, ) = torch.autograd.grad(z, p, dz.double())
	return z.detach(), g


SPECIAL = [0.0, -0.0, 20.0, float('inf'), -float('inf'), 1.0, -1.0, 19.0, 21.0, 2.0 ** -126, -2.0 ** -126, 20.0 - 2.0 ** -4, 20.0 + 2.0 ** -3, 5.0, -5.0, 0.5]


@pytest.mark.parametrize('dtn', list(DTYPES))
@pytest.mark.parametrize('act', ['relu', 'hardtanh', 'leaky_relu'])
@pytest.mark.parametrize('how', ['plain', 'scaled', 'residual'])
def test_gate_boundaries_match_torch_bit_for_bit(act, dtn, how):
	"""Pre-activations of exactly 0, -0, 20, +-inf (and their neighbours), exact in fp32: z, the gate bit and g equal torch's forward and
	autograd (strict gate: gradient 0 at both ends of hardtanh and at relu's 0, the slope at leaky-relu's 0; at +inf relu and leaky-relu pass
	the gradient like at any positive value).  plain: pre = y; scaled: pre = 2 y + 4 (y chosen so that pre hits the values); residual: pre =
	y + res with one residual."""
	from convasr_amd import ops
	d, dt, nonlin = dev(), DTYPES[dtn], R.NONLINS[act]
	a = ops.act_args(nonlin)
	B, T, C = 2, 3, 16
	pre = torch.tensor(SPECIAL, dtype = torch.float32).repeat(B * T).reshape(B, T, C)
	pre = rep(pre, dt)  # (a value the storage type does not hold moves to a neighbour or becomes another exact tie: 2^-126 is 0 in fp16)
	scale = shift = None
	res = []
	if how == 'plain':
		y = pre
	elif how == 'scaled':
		y = rep((pre - 4.0) / 2.0, dt)
		scale, shift = torch.full((C, ), 2.0), torch.full((C, ), 4.0)
		pre = y * 2.0 + 4.0  # exact in fp32 (and what fmaf gives)
	else:
		res = [rep(torch.tensor([3.0, -3.0, 1.0, 0.0] * 4).expand(B, T, C).clone(), dt)]
		y = rep(pre - res[0], dt)
		pre = y + res[0]
	assert bool((pre.double() == R.pre_activation(y, scale, shift, res).double()).all() | torch.isnan(pre).any())
	dz = rep(torch.randn(B, T, C) + 3.0, dt)
	z_ref, g_ref = torch_act_and_grad(pre, nonlin, dz)
	resargs = dict(res = [cl(r, dt, d) for r in res]) if res else {}
	gate = torch.zeros(B * T * C // 8, dtype = torch.uint8, device = d) if act != 'leaky_relu' else None
	z = rows(ops.bn_act(cl(y, dt, d), to(scale, d), to(shift, d), a, gate = gate, **resargs))
	# leaky-relu multiplies by the slope as fp32 holds it: where it does, equality with float64 is to one rounding, everywhere else to the bit
	everywhere = torch.full(pre.shape, act != 'leaky_relu')
	for name, got, ref, exact in (('z', z, z_ref, everywhere | (pre >= 0) | torch.isinf(pre)), ('g', None, g_ref, everywhere | (pre > 0))):
		if got is None:
			got = g = rows(ops.bn_act_bwd_reduce(cl(dz, dt, d), cl(y, dt, d), to(scale, d), to(shift, d), None, None, a, **resargs))
		assert exact.dtype == torch.bool
		assert torch.equal(got[exact], ref.to(dt).double()[exact]), (name, got[0, 0], ref[0, 0])
		if not bool(exact.all()):
			close_ew(got[~exact], ref[~exact], dtn, name + ' (scaled by the slope)')
	if gate is not None:
		assert torch.equal(unpack_gate(gate, B, T, C), g_ref != 0), 'gate bits'
		if not res:
			cf = torch.cat([torch.ones(C), torch.zeros(2 * C)]).to(d)  # dy = g
			y0 = torch.where(torch.isinf(y), torch.zeros_like(y), y)  # (B y + D with B = 0 must not make inf * 0; the gated pass never looks at y's value)
			dy = rows(ops.bn_act_bwd_apply(cl(dz, dt, d), cl(y0, dt, d), cf, True, gate = gate))
			assert torch.equal(dy, g_ref.to(dt).double()), 'g from the stored gates'


@pytest.mark.parametrize('dtn', list(DTYPES))
@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('p_drop', [0.0, 0.5])
def test_nan_pre_activation_propagates_like_torch(act, dtn, p_drop):
	"""A NaN pre-activation gives NaN out of every activation (F.relu / F.hardtanh / F.leaky_relu all propagate it): the loss turns non-finite and
	the step is skipped, instead of the NaN being swallowed as 0.  Backward rule (common.h, act_grad): the gradient is zeroed (leaky-relu: scaled)
	only where pre <= lo or pre >= hi COMPARES true, so a NaN pre-activation passes the gradient unchanged and its gate bit is 1 -- in the
	re-derived AND in the gated backward passes.  With dropout: z = NaN x keep is NaN whether the element is kept or not; a dropped element
	has g = 0 and gate bit 0 like any other dropped element.  First form: the NaN is in y, no scale; second: it is in a residual input (y finite,
	so that the gated passes, which read y but never the pre-activation, have finite sums and dy to compare)."""
	from convasr_amd import ops
	d, dt, nonlin = dev(), DTYPES[dtn], R.NONLINS[act]
	a = ops.act_args(nonlin)
	B, T, C = 2, 5, 40
	gen = torch.Generator().manual_seed(9)
	keep = keep_pattern(B, T, C, dt, p_drop, d)
	drop = dict(dropout_p = p_drop, seed = SEED, offset = OFFSET)
	nan_at = torch.rand(B, T, C, generator = gen) < 0.04
	assert int(nan_at.sum()) >= 8 and (keep is None or (bool((keep[nan_at] == 0).any()) and bool((keep[nan_at] != 0).any())))
	dz = rep(torch.randn(B, T, C, generator = gen) + 3.0, dt)
	for form in ('y', 'residual'):
		y = rep(torch.randn(B, T, C, generator = gen) * 8, dt)
		scale, shift, res = None, None, []
		if form == 'y':
			y[nan_at] = float('nan')
		else:
			scale, shift, res = torch.rand(C, generator = gen) + 0.5, torch.randn(C, generator = gen), [rep(torch.randn(B, T, C, generator = gen), dt)]
			res[0][nan_at] = float('nan')
		pre = R.pre_activation(y, scale, shift, res)
		kp = torch.ones(B, T, C, dtype = torch.float64) if keep is None else keep
		z_ref, g_ref = torch_act_and_grad(pre, nonlin, dz)
		z_ref, g_ref = z_ref * kp, g_ref * kp
		assert bool(torch.isnan(z_ref[nan_at]).all()) and not bool(torch.isnan(z_ref[~nan_at]).any())
		resargs = dict(res = [cl(r, dt, d) for r in res]) if res else {}
		gate = torch.zeros(B * T * C // 8, dtype = torch.uint8, device = d) if act != 'leaky_relu' else None
		yd, dzd = cl(y, dt, d), cl(dz, dt, d)
		z = rows(ops.bn_act(yd, to(scale, d), to(shift, d), a, gate = gate, **resargs, **drop))
		assert torch.equal(torch.isnan(z), nan_at), 'NaN pre-activations, and only they, give NaN'
		close_ew(z[~nan_at], z_ref[~nan_at], dtn, 'z beside the NaNs')
		g = rows(ops.bn_act_bwd_reduce(dzd, yd, to(scale, d), to(shift, d), None, None, a, **resargs, **drop))
		# torch gives no one rule there: relu passes the gradient, leaky-relu scales it by the slope, and hardtanh passes it in ATen's scalar path
		# but zeroes it in the vectorised one (torch 2.10 CPU: 3.0 for a 5-element tensor, 0.0 for a 64-element one).  The kernels' rule is one
		# for every kind: a NaN compares with no bound, the gradient passes unchanged.
		assert not bool(torch.isnan(g_ref).any())
		g_ref[nan_at] = (dz.double() * kp)[nan_at]
		close_ew(g, g_ref, dtn, 'g')
		assert torch.equal(g[nan_at] != 0, kp[nan_at] != 0), 'the gradient at a NaN pre-activation is zero only where dropout dropped the element'
		if gate is None:
			continue
		assert torch.equal(unpack_gate(gate, B, T, C), g_ref != 0), 'gate bits'
		if form == 'residual':  # the gated backward passes on those bits (they take no residual inputs: the bits carry all that the pre-activation decided)
			mean, invstd = torch.randn(C, generator = gen), torch.rand(C, generator = gen) + 0.5
			sums = torch.full((2 * C, ), float('nan'), dtype = torch.float64, device = d)
			assert ops.bn_act_bwd_reduce(dzd, yd, to(scale, d), to(shift, d), mean.to(d), invstd.to(d), a, write_g = False, sums = sums, gate = gate, **drop) is None
			sg, sgx = R.bn_sums(g_ref, y, mean, invstd)
			close_sums(sums[:C], sums[C:], sg, sgx, 'gated reduce over NaN pre-activations')
			cf = torch.randn(3 * C, generator = gen)
			dy = rows(ops.bn_act_bwd_apply(dzd, yd, cf.to(d), True, to(scale, d), to(shift, d), a, gate = gate, **drop))
			close_dy(dy, R.f64(cf[:C]) * g_ref + R.f64(cf[C:2 * C]) * R.f64(y) + R.f64(cf[2 * C:]), dtn, 'gated apply over NaN pre-activations')


@pytest.mark.parametrize('dtn', list(DTYPES))
@pytest.mark.parametrize('act', ['relu', 'hardtanh', 'leaky_relu'])
def test_nan_input_frame_propagates_through_the_conv_epilogue_activation(act, dtn):
	from convasr_amd import ops, _lib
	d, dt, nonlin = dev(), DTYPES[dtn], R.NONLINS[act]
	torch.manual_seed(4)
	B, Cin, Cout, T, K = 2, 64, 128, 300, 5
	x, w = rep(torch.randn(B, Cin, T), dt), rep(torch.randn(Cout, Cin, K) / 18, dt)
	x[1, :, 140] = float('nan')  # one frame: reaches output frames 138 .. 142 of utterance 1
	scale, shift = torch.rand(Cout) + 0.5, torch.randn(Cout)
	ref = R.activation(F.conv1d(x.double(), w.double(), padding = K // 2) * scale.double()[None, :, None] + shift.double()[None, :, None], nonlin)
	want_nan = torch.zeros(B, Cout, T, dtype = torch.bool)
	want_nan[1, :, 138:143] = True
	assert torch.equal(torch.isnan(ref), want_nan)
	wp = ops.pack_weight(w.to(d), dt, _lib.PACK_FWD)
	y = ops.conv1d(ops.as_cl(x.to(d), dt), wp, Cout, K, 1, 1, K // 2, scale = scale.to(d), shift = shift.to(d), act = ops.act_args(nonlin)).double().cpu()
	assert torch.equal(torch.isnan(y), want_nan), 'the fused activation of the conv epilogue swallowed (or spread) a NaN'
	close_ew(y[~want_nan], ref[~want_nan], dtn, 'conv epilogue beside the NaN frames', f32_bar = (1e-4, 2e-5))  # (test_conv1d_forward's fp32 bar: a 320-term fp32 dot product)
