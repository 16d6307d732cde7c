"""The float64 restatement tests/_bn_ref.py against torch.autograd through F.batch_norm -> + residual batch norms -> activation ->
dropout keep -> frame mask, all in float64 on the CPU.  This is what makes the reference of tests/test_bn_kernels_gpu.py trustworthy."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bn_ref as R  # noqa: E402

from oracle import convasr_oracle as O  # noqa: E402

EPS, MOMENTUM = 1e-5, 0.1


def same(a, b, what):
	"""1e-12 relative to the largest magnitude of the quantity (outputs that are differences have elements near 0)"""
	a, b = a.detach().double(), b.detach().double()
	assert a.shape == b.shape, (what, a.shape, b.shape)
	err, bar = float((a - b).abs().max()), 1e-12 * max(float(b.abs().max()), 1e-30)
	assert err <= bar, f'{what}: max abs err {err:.3e} > {bar:.3e}'


@pytest.mark.parametrize('n_res', [0, 2])
@pytest.mark.parametrize('act', ['none', 'relu', 'hardtanh', 'leaky_relu'])
@pytest.mark.parametrize('masked', [False, True])
def test_restatement_equals_autograd_through_batch_norm(n_res, act, masked):
	nonlin = R.NONLINS[act]
	torch.manual_seed(11 + n_res)
	B, T, C = 4, 37, 24
	n = B * T
	dd = dict(dtype = torch.float64)
	ys = [(torch.randn(B, T, C, **dd) * 8 + torch.randn(C, **dd)).requires_grad_(True) for _ in range(1 + n_res)]
	gammas = [(torch.rand(C, **dd) + 0.5).requires_grad_(True) for _ in ys]
	betas = [(torch.randn(C, **dd) * 4 + 4).requires_grad_(True) for _ in ys]
	xlen = torch.tensor([1.0, 0.0, 0.5 / T, 0.61]) if masked else None
	keep = (torch.rand(B, T, C) >= 0.2).double() * 1.25
	dz = torch.randn(B, T, C, **dd)
	# torch: (B, C, T) batch norms, summed, activated, dropped, masked
	rms, rvs = [torch.randn(C, **dd) for _ in ys], [torch.rand(C, **dd) + 0.5 for _ in ys]
	rms0, rvs0 = [t.clone() for t in rms], [t.clone() for t in rvs]
	pre_t = sum(F.batch_norm(y.permute(0, 2, 1), rm, rv, gm, bt, True, MOMENTUM, EPS) for y, rm, rv, gm, bt in zip(ys, rms, rvs, gammas, betas)).permute(0, 2, 1)
	mask = O.temporal_mask(T, O.compute_output_lengths(T, xlen, B)).double().unsqueeze(-1)
	z_t = R.activation(pre_t, nonlin) * keep * mask
	z_t.backward(dz)
	# the restatement: finalize from plain sums ...
	fins = []
	for y, gm, bt, rm0, rv0, rm, rv in zip(ys, gammas, betas, rms0, rvs0, rms, rvs):
		yd = y.detach()
		fin = R.finalize(yd.sum(dim = (0, 1)), (yd ** 2).sum(dim = (0, 1)), n, gm, bt, rm0, rv0, MOMENTUM, EPS)
		same(fin['mean'], yd.mean(dim = (0, 1)), 'mean')
		same(fin['var'], yd.var(dim = (0, 1), unbiased = False), 'biased variance')
		same(fin['running_mean'], rm, 'running_mean')
		same(fin['running_var'], rv, 'running_var')
		fins.append(fin)
	# ... forward ...
	z, pre = R.forward(ys[0], fins[0]['scale'], fins[0]['shift'], ys[1:], [f['scale'] for f in fins[1:]], [f['shift'] for f in fins[1:]], nonlin, keep, xlen)
	same(pre, pre_t, 'pre-activation')
	same(z, z_t, 'z')
	# ... backward
	g, bits = R.grad_pre(pre, nonlin, keep, xlen, dz)
	assert bool((bits == (g != 0)).all()) or act == 'leaky_relu'  # (dz has no exact zeros)
	if masked:
		assert not bool(g[1].any()) and not bool(z[1].any()) and not bool(g[2, 1:].any()) and bool(g[2, 0].any())  # xlen 0: no valid frame; 0.5 / T: one
	for y, gm, bt, fin in zip(ys, gammas, betas, fins):
		sg, sgx = R.bn_sums(g, y, fin['mean'], fin['invstd'])
		same(sgx, gm.grad, 'dgamma = sum g xhat')
		same(sg, bt.grad, 'dbeta = sum g')
		dy = R.bn_dy(g, y, gm, fin['mean'], fin['invstd'])
		same(dy, y.grad, 'dy')
		A, Bc, D = R.bn_coef(sg, sgx, n, gm, fin['mean'], fin['invstd'])
		same(A * g + Bc * y.detach() + D, y.grad, 'dy from the coefficient triple')


def test_finalize_edges_and_eval_scale_shift():
	dd = dict(dtype = torch.float64)
	torch.manual_seed(3)
	C = 8
	# n = 1: variance 0, running variance takes the biased estimate (no division by n - 1)
	y = torch.randn(1, C, **dd)
	fin = R.finalize(y.sum(0), (y ** 2).sum(0), 1, None, None, torch.zeros(C, **dd), torch.ones(C, **dd), MOMENTUM, EPS)
	same(fin['mean'], y[0], 'mean, n = 1')
	assert bool((fin['var'].abs() < 1e-12).all()) and bool((fin['var'] >= 0).all())
	same(fin['running_var'], torch.full((C, ), 1 - MOMENTUM, **dd) + MOMENTUM * fin['var'], 'running_var, n = 1')
	same(fin['scale'], fin['invstd'], 'scale without gamma')
	same(fin['shift'], -fin['mean'] * fin['invstd'], 'shift without beta')
	# a negative E[x^2] - m^2 (rounding of the caller's sums) clamps at 0
	fin = R.finalize(torch.full((C, ), 30.0, **dd), torch.full((C, ), 89.999999, **dd), 10, None, None, None, None, MOMENTUM, EPS)
	assert bool((fin['var'] == 0).all())
	same(fin['invstd'], torch.full((C, ), EPS ** -0.5, **dd), 'invstd at variance 0')
	# eval mode against F.batch_norm(training = False)
	x = torch.randn(5, C, 9, **dd)
	gm, bt, rm, rv = torch.rand(C, **dd) + 0.5, torch.randn(C, **dd), torch.randn(C, **dd), torch.rand(C, **dd) + 0.5
	sc, sh = R.eval_scale_shift(gm, bt, rm, rv, EPS)
	same(x * sc[None, :, None] + sh[None, :, None], F.batch_norm(x, rm, rv, gm, bt, False, MOMENTUM, EPS), 'eval scale / shift')


def test_near_bound_finds_exactly_the_band():
	dd = dict(dtype = torch.float64)
	y = torch.tensor([[[0.0, 1e-7, 1e-3, 20.0, 20.0 - 1e-5, 19.0, 20.0 + 3e-4, 5.0]]], **dd)
	near = R.near_bound(y, None, None, (), (), (), R.NONLINS['hardtanh'])
	assert near.flatten().tolist() == [True, False, False, True, True, False, False, False]
	assert R.near_bound(y, None, None, (), (), (), R.NONLINS['relu']).flatten().tolist() == [True, False, False, False, False, False, False, False]
	assert not bool(R.near_bound(y, None, None, (), (), (), None).any())
	# the band scales with the magnitude of the addends, not with the (cancelled) pre-activation
	y2, res = torch.full((1, 1, 8), 1000.0, **dd), [torch.full((1, 1, 8), -1000.0 + 1e-3, **dd)]
	assert bool(R.near_bound(y2, None, None, res, (), (), R.NONLINS['relu']).all())
