"""tests/_wgrad_ref.py held to float64 autograd, its case tables held to the edges they claim, and the weight-gradient entry points' refusals.
No GPU: the plan queries (ops.wgrad_plan, ops.wgrad1x1_grouped_plan) launch nothing, and the refusals are argument checks that run before any
launch, on pointers that are never dereferenced."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wgrad_ref as R  # noqa: E402


# ---- the restatement

def _autograd(x, dy, K, stride, dil, pad):
	"""float64 autograd of F.conv1d; dy may have fewer frames than the conv yields (the missing ones get a zero gradient)"""
	w = torch.zeros(dy.shape[1], x.shape[1], K, dtype = torch.float64, requires_grad = True)
	b = torch.zeros(dy.shape[1], dtype = torch.float64, requires_grad = True)
	y = F.conv1d(x.double(), w, b, stride = stride, padding = pad, dilation = dil)
	g = torch.zeros_like(y)
	g[:, :, :dy.shape[2]] = dy.double()
	y.backward(g)
	return w.grad, b.grad


@pytest.mark.parametrize('shape', [
	# (B, Cin, Cout, Tout, K, stride, dil, pad, trunc)
	(2, 5, 7, 13, 3, 1, 1, 1, 0), (3, 4, 6, 11, 5, 2, 1, 2, 0), (2, 3, 5, 9, 4, 1, 3, 4, 0), (2, 6, 4, 17, 3, 1, 2, 0, 0), (2, 5, 3, 12, 3, 1, 2, 4, 0),
	(1, 7, 2, 10, 5, 2, 2, 9, 0), (3, 9, 8, 6, 1, 1, 1, 0, 0), (2, 4, 4, 8, 1, 2, 1, 0, 0), (2, 5, 6, 10, 4, 1, 1, 2, 1), (2, 5, 6, 10, 6, 2, 1, 3, 1)])
def test_restatement_equals_float64_autograd(shape):
	B, Cin, Cout, Tout, K, stride, dil, pad, trunc = shape
	Tin = R.tin_of(Tout + trunc, K, stride, dil, pad)
	g = torch.Generator().manual_seed(sum(shape))
	x, dy = torch.randn(B, Cin, Tin, generator = g, dtype = torch.float64), torch.randn(B, Cout, Tout, generator = g, dtype = torch.float64)
	dw, db, absdot = R.wgrad(x, dy, K, stride, dil, pad)
	rw, rb = _autograd(x, dy, K, stride, dil, pad)
	assert float((dw - rw).abs().max()) <= 1e-12 * float(rw.abs().max()) and float((db - rb).abs().max()) <= 1e-12 * float(rb.abs().max())
	aw, _ = _autograd(x.abs(), dy.abs(), K, stride, dil, pad)
	assert float((absdot - aw).abs().max()) <= 1e-12 * float(aw.abs().max()) and bool((absdot >= dw.abs() - 1e-12).all())
	# the fp32 chain is the same sum: on integers it is exact, on random data within the standard bound of a chain of B Tout terms
	xi, yi = R.integer_operands((B, Cin, Tin, Cout, Tout), 3)
	assert torch.equal(torch.from_numpy(R.chain32(xi, yi, K, stride, dil, pad)).double(), R.wgrad(xi, yi, K, stride, dil, pad)[0][:R.CORNER, :R.CORNER])
	c = torch.from_numpy(R.chain32(x.float(), dy.float(), K, stride, dil, pad)).double()
	d64, _, a64 = R.wgrad(x.float(), dy.float(), K, stride, dil, pad)
	assert bool(((c - d64[:R.CORNER, :R.CORNER]).abs() <= 2 * (B * Tout + 1) * R.U32 * a64[:R.CORNER, :R.CORNER] + R.TINY).all())
	assert torch.equal(torch.from_numpy(R.chain32_rows(yi.permute(0, 2, 1).reshape(-1, Cout))).double(), yi.double().sum(dim = (0, 2))[:R.CORNER])


@pytest.mark.parametrize('K,pad', [(11, 5), (13, 6), (4, 2), (5, 0), (3, 1), (1, 0), (6, 3), (4, 1), (2, 0), (7, 4)])
def test_unfolded_gradient_of_the_folded_view_is_the_stride_2_gradient(K, pad):
	"""exactly, on integer data, for pad even and odd and K even and odd; the folded taps outside [0, K) are dropped"""
	B, Cin, Cout, Tin = 2, 3, 4, 26
	Kf, Pf, s0 = R.fold2(K, pad)
	assert Pf == -(-pad // 2) and s0 == 2 * Pf - pad and Kf == (K - 1 + s0) // 2 + 1
	Tout = (Tin + 2 * pad - (K - 1) - 1) // 2 + 1
	assert Tout <= Tin // 2 + 2 * Pf - Kf + 1  # the folded conv yields at least as many frames: the fold asks for the first Tout of them
	x, dy = R.integer_operands((B, Cin, Tin, Cout, Tout), K * 16 + pad)
	ref, _, _ = R.wgrad(x, dy, K, 2, 1, pad)
	dwf, _, _ = R.wgrad(R.fold_view(x), dy, Kf, 1, 1, Pf)
	assert dwf.shape == (Cout, 2 * Cin, Kf)
	assert torch.equal(R.unfold(dwf, K, pad), ref)
	assert torch.equal(ref, _autograd(x, dy, K, 2, 1, pad)[0])


# ---- the tables reach the edges they claim

def _plan(c, name):
	from convasr_amd import ops, _lib
	lib = _lib.load()
	prev = lib.convasr_debug_set_conv_v2(c.v2)
	try:
		return ops.wgrad_plan(R.DTYPES[name], c.B, c.Cin, c.Cout, R.tin(c), c.Tout, c.K, c.stride, c.dil)
	finally:
		lib.convasr_debug_set_conv_v2(prev)


@pytest.mark.parametrize('table', ['LDS_DMA', 'GENERAL'])
def test_every_case_reaches_the_edge_it_claims(table):
	"""asked of the library's own plan (the code wgrad_impl launches from): a shape that stops reaching its edge after the cost model is
	retuned fails here, before any GPU run"""
	cases = getattr(R, table)
	assert len({c.name for c in cases}) == len(cases)
	for c in cases:
		assert R.tin(c) > 0 and c.B * c.Tout <= 400000, c.name  # (integer sums stay below 2^24)
		for name, claimed in c.edges.items():
			got = R.edges_of(c, name, _plan(c, name))
			print(f'    {table} {c.name} {name}: {got}')
			assert 'route' in claimed, c.name
			for k, v in claimed.items():
				assert got.get(k) == v, (table, c.name, name, k, v, got)


def test_tables_cover_the_listed_edges():
	from convasr_amd import ops  # noqa: F401
	reach = lambda cases, name, key: {R.edges_of(c, name, _plan(c, name)).get(key) for c in cases if name in c.edges and c.edges[name]['route'] == _plan(c, name)['route']}
	lds = [c for c in R.LDS_DMA if c.edges['bf16']['route'] == 'lds_dma']
	assert {1, 2, 3, 4, 5, 8, 12} <= reach(lds, 'bf16', 'cps') and {5, 12} <= reach(lds, 'f16', 'cps')
	assert {1, 2, 3, 4} <= reach(lds, 'bf16', 'last_taps') and set(range(32, 41)) <= reach(lds, 'bf16', 'pieces')
	assert {c.name for c in R.STARRED} >= {'one_chunk', 'taps3', 'taps4+3', 'pieces40_envelope_edge', 'ring5_last2', 'ring12_workload'} and set(R.SAME_BITS) <= {c.name for c in lds}
	for name in R.ALL:
		assert max(reach(R.GENERAL, name, 'cps')) >= 5, name
		assert {R.TT, R.TF, R.FT, R.FF} <= reach(R.GENERAL, name, 'align') and {5, 12} <= reach(R.GENERAL, name, 'xi'), name
		assert 12 in reach(R.GENERAL, name, 'xi_used') and {5, 6} <= reach(R.GENERAL, name, 'xi_used'), name
		assert {1, 2, 3, 4} <= reach(R.GENERAL, name, 'last_taps'), name


def test_plan_query_follows_the_switch_and_the_pitches():
	from convasr_amd import ops, _lib
	lib = _lib.load()
	bf = torch.bfloat16
	assert ops.wgrad_plan(bf, 2, 128, 128, 300, 300, 3, 1, 1)['route'] == 'lds_dma' and ops.wgrad_plan(torch.float32, 2, 128, 128, 300, 300, 3, 1, 1)['route'] == 'general'
	assert ops.wgrad_plan(bf, 2, 128, 128, 599, 300, 3, 2, 1)['route'] == 'general' and ops.wgrad_plan(bf, 2, 128, 136, 300, 300, 3, 1, 1)['route'] == 'general'
	prev = lib.convasr_debug_set_conv_v2(0)
	try:
		assert ops.wgrad_plan(bf, 2, 128, 128, 300, 300, 3, 1, 1)['route'] == 'general'
		assert ops.wgrad_plan(bf, 2, 128, 128, 300, 300, 3, 1, 1, x_ld = 384)['route'] == 'refused'
	finally:
		lib.convasr_debug_set_conv_v2(prev)
	# a pitch: the LDS-DMA kernel or nothing -- the answer of convasr_conv1d_wgrad_ld_supported
	for Cin, Cout, K, dil, x_ld, dy_ld in [(128, 128, 3, 1, 384, 128), (128, 256, 6, 1, 384, 768), (64, 128, 3, 1, 192, 128), (128, 128, 4, 11, 384, 128), (128, 128, 3, 1, 388, 128)]:
		route = ops.wgrad_plan(bf, 2, Cin, Cout, 300, 300, K, 1, dil, x_ld = x_ld, dy_ld = dy_ld)['route']
		assert route == ('lds_dma' if lib.convasr_conv1d_wgrad_ld_supported(_lib.BF16, 2, Cin, Cout, 300, 300, K, dil, x_ld, dy_ld) else 'refused'), (Cin, Cout, K, dil, x_ld, dy_ld)
	assert ops.wgrad_plan(bf, 2, 128, 128, 300, 300, 3, 1, 1, x_ld = 384) == dict(ops.wgrad_plan(bf, 2, 128, 128, 300, 300, 3, 1, 1), route = 'lds_dma')  # (a pitch of 0 = dense)
	assert ops.wgrad_plan(bf, 2, 128, 128, 300, 300, 3, 1, 1, dy_ld = 384)['route'] == 'lds_dma' and ops.wgrad_plan(bf, 2, 128, 128, 300, 300, 3, 1, 1, dy_ld = 64)['route'] == 'refused'
	assert ops.wgrad_plan(bf, 2, 128, 128, 300, 300, 65, 1, 1)['route'] == 'refused' and ops.wgrad_plan(torch.float32, 2, 128, 128, 300, 300, 3, 1, 1, x_ld = 384)['route'] == 'refused'
	# the workspace the entry point is given holds the plan's slabs
	for c in R.LDS_DMA + R.GENERAL:
		for name in c.edges:
			p = _plan(c, name)
			assert lib.convasr_conv1d_wgrad_workspace_bytes(c.B, c.Cin, c.Cout, R.tin(c), c.Tout, c.K, c.stride, c.dil) >= p['splits'] * c.K * c.Cout * c.Cin * 4, (c.name, name)


def test_grouped_plan_query():
	from convasr_amd import ops, _lib
	lib = _lib.load()
	seen = set()
	for (B, T), probs, claimed in R.GROUPED:
		cins, couts = [p[0] for p in probs], [p[1] for p in probs]
		for dt in (torch.bfloat16, torch.float16):
			got = ops.wgrad1x1_grouped_plan(dt, cins, couts, B, T)
			print(f'    GROUPED {(B, T)} x {len(probs)}: {got}')
			assert got == claimed, ((B, T), probs, got)
			splits, cps = got
			assert (splits - 1) * cps < B * -(-T // 64) <= splits * cps
			assert lib.convasr_wgrad1x1_grouped_workspace_bytes(len(probs), ops._int_array(cins), ops._int_array(couts), B, T) == splits * sum(a * b for a, b in probs) * 4
		seen.add(len(probs))
	assert {1, 2, 5, R.GROUPED_MAX} <= seen and (32, 12) in [c for _, _, c in R.GROUPED]
	assert ops.wgrad1x1_grouped_plan(torch.bfloat16, [128] * 13, [128] * 13, 2, 300) is None and ops.wgrad1x1_grouped_plan(torch.bfloat16, [192], [128], 2, 300) is None
	assert ops.wgrad1x1_grouped_plan(torch.float32, [128], [128], 2, 300) is None


# ---- the refusals

def test_weight_gradient_entry_points_refuse_before_any_launch():
	"""every refusal is a negative code and a message that names the entry point; the pointers are never dereferenced"""
	from convasr_amd import ops, _lib
	lib = _lib.load()
	p = ctypes.c_void_p(4096)
	bf, f32 = _lib.BF16, _lib.F32
	refused = lambda rc, name: rc < 0 and name in lib.convasr_last_error()
	wgrad = lambda dt, B, Cin, Cout, Tin, Tout, K, stride, dil, pad, layout = _lib.W_REFERENCE: lib.convasr_conv1d_wgrad(p, p, p, None, p, dt, B, Cin, Cout, Tin, Tout, K, stride, dil, pad, 0, layout, None)
	assert refused(wgrad(bf, 1, 128, 128, 64, 64, 65, 1, 1, 32), b'conv1d_wgrad: K 65')
	assert refused(wgrad(f32, 1, 35, 35, 64, 64, 3, 1, 1, 1, _lib.W_KMAJOR), b'conv1d_wgrad: K-major')
	# a tile that is too large for the general kernel (one dilation step past R.GENERAL's x_rows_limit cases)
	assert refused(wgrad(bf, 1, 16, 16, R.tin_of(40, 4, 2, 22, 33), 40, 4, 2, 22, 33), b'conv1d_wgrad: tile too large')
	assert refused(wgrad(_lib.F16, 1, 16, 16, R.tin_of(40, 4, 2, 22, 33), 40, 4, 2, 22, 33), b'conv1d_wgrad: tile too large')
	assert refused(wgrad(f32, 1, 16, 16, R.tin_of(40, 4, 2, 12, 18), 40, 4, 2, 12, 18), b'conv1d_wgrad: tile too large')
	for dt, dil in ((torch.bfloat16, 22), (torch.float32, 12)):
		assert ops.wgrad_plan(dt, 1, 16, 16, R.tin_of(40, 4, 2, dil, dil * 3 // 2), 40, 4, 2, dil)['route'] == 'refused'
	# pitches outside the LDS-DMA envelope on _ld: fp32, not multiples of 8, below the channel count, channel counts the kernel does not take, too wide a window
	ld = lambda dt, Cin, Cout, K, dil, x_ld, dy_ld: lib.convasr_conv1d_wgrad_ld(p, x_ld, p, dy_ld, p, p, dt, 2, Cin, Cout, 300, 300, K, dil, 0, 0, _lib.W_REFERENCE, None)
	for bad in ((f32, 128, 128, 3, 1, 384, 128), (bf, 128, 128, 3, 1, 388, 128), (bf, 128, 128, 3, 1, 384, 132), (bf, 128, 128, 3, 1, 120, 128), (bf, 128, 128, 3, 1, 384, 64),
	            (bf, 64, 128, 3, 1, 192, 128), (bf, 128, 136, 3, 1, 384, 408), (bf, 128, 128, 4, 11, 384, 128), (bf, 128, 128, 65, 1, 384, 128)):
		assert refused(ld(*bad), b'conv1d_wgrad'), bad
	for bad in ((bf, 128, 128, 3, 1, 388, 128), (bf, 64, 128, 3, 1, 192, 128), (bf, 128, 128, 4, 11, 384, 128)):
		assert refused(ld(*bad), b'conv1d_wgrad_ld'), bad
	# the grouped one-tap launch: 13 problems, a channel count of 192, fp32
	grouped = lambda n, cins, couts, dt = bf: lib.convasr_wgrad1x1_grouped(n, (ctypes.c_void_p * 16)(*[4096] * 16), (ctypes.c_void_p * 16)(*[4096] * 16), (ctypes.c_void_p * 16)(*[4096] * 16), None,
	                                                                           ops._int_array(cins), ops._int_array(couts), None, p, dt, 2, 300, None)
	assert refused(grouped(13, [128] * 13, [128] * 13), b'wgrad1x1_grouped')
	assert refused(grouped(2, [128, 192], [128, 128]), b'wgrad1x1_grouped: problem 1')
	assert refused(grouped(1, [128], [192]), b'wgrad1x1_grouped') and refused(grouped(1, [128], [128], f32), b'wgrad1x1_grouped')
	assert lib.convasr_wgrad1x1_grouped_workspace_bytes(13, ops._int_array([128] * 13), ops._int_array([128] * 13), 2, 300) < 0
