"""tests/_conv_ref.py held to float64 F.conv1d and autograd, its planner held to the library's route query, its case tables held to the edges
they claim, and the forward conv's refusals.  No GPU: convasr_conv1d_fwd_route launches nothing, and the refusals are argument checks that
run before any launch, on pointers that are never dereferenced."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_ref as R  # noqa: E402

EVERY = [(t, c.name) for t, cases in R.TABLES.items() for c in cases]


# ---- the restatements

@pytest.mark.parametrize('shape', [
	# (B, Cin, Cout, Tin, K, stride, dil, pad, trunc)
	(2, 5, 7, 13, 3, 1, 1, 1, 0), (3, 4, 6, 23, 5, 2, 1, 2, 0), (2, 3, 5, 19, 4, 1, 3, 4, 0), (2, 6, 4, 17, 3, 1, 2, 0, 0), (2, 5, 3, 12, 3, 1, 2, 4, 0),
	(1, 7, 2, 21, 5, 2, 2, 9, 0), (3, 9, 8, 6, 1, 1, 1, 0, 0), (2, 4, 4, 8, 1, 2, 1, 0, 0), (2, 5, 6, 10, 4, 1, 1, 2, 1), (2, 5, 6, 20, 6, 2, 1, 3, 1)])
def test_restatements_equal_float64_torch(shape):
	B, Cin, Cout, Tin, K, stride, dil, pad, trunc = shape
	Tout = R.out_len(Tin, K, stride, dil, pad) - trunc
	g = torch.Generator().manual_seed(sum(shape))
	x, w, b = torch.randn(B, Cin, Tin, generator = g, dtype = torch.float64), torch.randn(Cout, Cin, K, generator = g, dtype = torch.float64), torch.randn(Cout, generator = g, dtype = torch.float64)
	ref = F.conv1d(x, w, b, stride = stride, padding = pad, dilation = dil)[:, :, :Tout]
	y = R.conv(x, w, b, stride, dil, pad, Tout)
	assert y.shape == ref.shape and float((y - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
	a = R.absdot(x, w, b, stride, dil, pad, Tout)
	assert float((a - (F.conv1d(x.abs(), w.abs(), b.abs(), stride = stride, padding = pad, dilation = dil)[:, :, :Tout])).abs().max()) <= 1e-12 * float(a.max()) and bool((a >= y.abs() - 1e-12).all())
	if stride == 1:  # the input gradient of the frames the conv was asked for
		xr = x.clone().requires_grad_(True)
		dy = torch.randn(B, Cout, Tout, generator = g, dtype = torch.float64)
		F.conv1d(xr, w, None, padding = pad, dilation = dil)[:, :, :Tout].backward(dy)
		dx = R.dgrad(dy, w, dil, pad, Tin)
		assert float((dx - xr.grad).abs().max()) <= 1e-12 * float(xr.grad.abs().max())
		# ... which is the forward restatement on dy with the taps flipped, the channels swapped and pad' = dil (K - 1) - pad: what the kernels run
		assert float((dx - R.conv(dy, w.flip(2).permute(1, 0, 2), None, 1, dil, dil * (K - 1) - pad, Tin)).abs().max()) <= 1e-12 * float(dx.abs().max())
	# the fp32 chain is the same sum: exact on integers, within the standard bound of a chain of Cin K + 1 terms on random data
	xi, wi = torch.randint(-1, 7, (B, Cin, Tin), generator = g).float(), torch.randint(-3, 4, (Cout, Cin, K), generator = g).float()
	assert torch.equal(torch.from_numpy(R.chain32(xi, wi, b.round(), stride, dil, pad, Tout)).double(), R.conv(xi, wi, b.round(), stride, dil, pad, Tout)[:, :R.CORNER])
	c = torch.from_numpy(R.chain32(x.float(), w.float(), b.float(), stride, dil, pad, Tout)).double()
	y32, a32 = R.conv(x.float(), w.float(), b.float(), stride, dil, pad, Tout), R.absdot(x.float(), w.float(), b.float(), stride, dil, pad, Tout)
	assert bool(((c - y32[:, :R.CORNER]).abs() <= 2 * (Cin * K + 1) * R.U32 * a32[:, :R.CORNER] + R.TINY).all())


def test_epilogue_statistics_and_length_mask():
	g = torch.Generator().manual_seed(7)
	raw = torch.randn(3, 5, 11, generator = g, dtype = torch.float64) * 8
	scale, shift, xlen = torch.randn(5, generator = g), torch.randn(5, generator = g), torch.tensor([1.0, 0.61, 0.3])
	assert R.valid_len(xlen, 11).tolist() == [11, 7, 4] and R.valid_len(torch.tensor([0.7]), 300).tolist() == [int(torch.ceil(torch.tensor(0.7) * 300))]
	mask = (torch.arange(11).view(1, 1, -1) < torch.tensor([11, 7, 4]).view(-1, 1, 1)).double()
	ref = F.hardtanh(raw * scale.double().view(1, -1, 1) + shift.double().view(1, -1, 1), 0.0, 20.0) * mask
	assert torch.equal(R.epilogue(raw, scale, shift, ('hardtanh', 0.0, 20.0), xlen), ref)
	assert torch.equal(R.epilogue(raw, None, None, 'relu', None), F.relu(raw)) and torch.equal(R.epilogue(raw, None, None, None, None), raw)
	masked = R.epilogue(-raw.abs() - 1, None, None, None, xlen)[1, :, 7:]
	assert bool((masked == 0).all()) and not bool(torch.signbit(masked).any())  # +0 exactly
	s1, s2 = R.stats(raw)
	assert torch.allclose(s1, raw.permute(1, 0, 2).reshape(5, -1).sum(1), rtol = 1e-14) and torch.allclose(s2, (raw ** 2).permute(1, 0, 2).reshape(5, -1).sum(1), rtol = 1e-14)


@pytest.mark.parametrize('name', R.HALVES)
def test_round16_is_round_to_nearest_even_into_the_storage_type(name):
	dt = R.DTYPES[name]
	g = torch.Generator().manual_seed(3)
	v = torch.cat([torch.randn(4096, generator = g) * 10.0 ** torch.randint(-42, 6, (4096, ), generator = g).float(), torch.arange(-2048, 2049).float() * 0.25, torch.tensor([0.0, 60000.0, 65519.0, 65520.0, -70000.0, 3e38])])
	want = v.to(dt).double()  # (one rounding: fp32 -> the storage type)
	got = R.round16(v.double(), name)
	assert torch.equal(got, want), (v[got != want][:4], got[got != want][:4], want[got != want][:4])
	# a float64 value fp32 would round first: just above a tie of the storage type
	tie = 1.0 + R.U16[name]
	assert float(R.round16(torch.tensor([tie + 2.0 ** -40, tie, 1 + 3 * R.U16[name]], dtype = torch.float64), name)[0]) == 1.0 + 2 * R.U16[name]
	assert R.round16(torch.tensor([tie, 1 + 3 * R.U16[name]], dtype = torch.float64), name).tolist() == [1.0, 1.0 + 4 * R.U16[name]]


# ---- the planner is the library's dispatcher, and the tables reach the edges they claim

def _route(c, name, bits = None, v2 = None, dgrad = False):
	from convasr_amd import ops, _lib
	lib = _lib.load()
	v2 = (c.v2 if name != 'f32' else 1) if v2 is None else v2
	prev = lib.convasr_debug_set_conv_v2(v2 | ((c.bits if bits is None else bits) << 8))
	try:
		dt, yd = R.DTYPES[name], R.DTYPES['f32' if c.out == 'f32' else name]
		if dgrad:
			return ops.conv_route(dt, yd, c.B, c.Cout, c.Cin, R.tout(c) + c.trunc, c.T, c.K, 1, c.dil, c.dil * (c.K - 1) - c.pad)
		e = c.epi
		return ops.conv_route(dt, yd, c.B, c.Cin, c.Cout, c.T, R.tout(c), c.K, c.stride, c.dil, c.pad, scale = e['scale'], act = _lib.ACT_NONE if e['act'] is None else _lib.ACT_RELU if e['act'] == 'relu' else _lib.ACT_HARDTANH,
		                      xlen = e['xlen'] is not None, stats = e['stats'])
	finally:
		lib.convasr_debug_set_conv_v2(prev)


@pytest.mark.parametrize('table,case_name', EVERY + [('-', R.SPLITK_FALLBACK.name), ('-', R.REFUSED.name)])
def test_planner_is_the_route_query_and_the_case_reaches_its_edge(table, case_name):
	"""asked of the code conv1d_run launches from: a shape that stops reaching its instantiation after the dispatcher is retuned fails here,
	before any GPU run"""
	c = R.by_name(case_name)
	assert R.tout(c) > 0
	for name in c.dtypes:
		got = _route(c, name)
		print(f'    {table} {c.name} {name}: {got}')
		assert got == R.plan_of(c, name), (c.name, name, got, R.plan_of(c, name))
		for k, v in c.edges.items():
			assert got.get(k) == v, (c.name, name, k, v, got)
		# the other settings the GPU file runs the case under
		for bits in (R.QUARTERS_BITS if c.name == 'quarters' else ()) + ((c.bits | R.FLIP_STAGES, c.bits | R.NO_1X1) if table == 'ONE_TAP' else ()):
			assert _route(c, name, bits = bits) == R.plan_of(c, name, bits = bits), (c.name, name, bits)
		for v2 in (0, 1):
			assert _route(c, name, v2 = v2) == R.plan_of(c, name, v2 = v2), (c.name, name, v2)
		if R.has_dgrad(c):
			for v2 in (0, 1):
				assert _route(c, name, v2 = v2, dgrad = True) == R.plan_of(c, name, v2 = v2, dgrad = True), (c.name, name, 'dgrad', v2)
			assert _route(c, name, dgrad = True)['route'] != 'refused'


def test_tables_cover_the_listed_edges():
	plans = {(c.name, n): R.plan_of(c, n) for cases in R.TABLES.values() for c in cases for n in c.dtypes}
	lds = [p for p in plans.values() if p['route'] == 'lds_dma']
	assert {0, 1, 2} <= {p['tail128'] for p in lds} and {128, 256} <= {p['tile_rows'] for p in lds} and {2, 4} <= {p['narrow_parts'] for p in lds if p['full_tiles'] < p['total_tiles']}
	assert any(p['full_tiles'] == 0 for p in lds) and any(0 < p['full_tiles'] < p['total_tiles'] for p in lds) and max(p['lds_bytes'] for p in lds) == 160 * 1024
	assert any(p['m_tiles_per_b'] * p['B'] % 16 and p['n_tiles'] % 2 and p['n_tiles'] > 1 for p in lds)  # tile_coords: a ragged m block, an n group of width 1
	for n in R.ALL:
		gen = [p for (_, m), p in plans.items() if m == n and p['route'] == 'general']
		assert {5, 9, 16} <= {p['xi'] for p in gen if p['aligned_x']} and any(not p['aligned_x'] for p in gen), n
	for n in R.HALVES:
		assert {1, 2} <= {p['stages'] for (_, m), p in plans.items() if m == n and p['route'] == 'one_tap'}
	# dgrad runs reach both 16-bit kernels too
	assert {'lds_dma', 'general'} <= {R.plan_of(c, 'bf16', dgrad = True)['route'] for c in R.LDS_DMA if R.has_dgrad(c)}
	# a chip of another size moves the thresholds the cases sit on: the planner takes n_cu, the tables assume 256
	c = R.by_name('quarters')
	assert R.plan_of(c, 'bf16', n_cu = 304)['full_tiles'] == 264 and R.plan_of(R.by_name('all_short_halves'), 'bf16', n_cu = 4)['tile_rows'] == 256


def test_split_k_plans():
	from convasr_amd import _lib
	lib = _lib.load()
	nb = ctypes.c_int64(0)
	for c in R.SPLITK + [R.SPLITK_FALLBACK]:
		for name in c.dtypes:
			splits, cps = R.splitk_plan(name, c.B, c.Cin, c.Cout, R.tout(c))
			assert lib.convasr_conv1d_fwd_splitk_plan(_lib.dtype_code(R.DTYPES[name]), c.B, c.Cin, c.Cout, R.tout(c), c.K, ctypes.byref(nb)) == splits >= 2 and nb.value == splits * c.B * R.tout(c) * c.Cout * 4
			if c is not R.SPLITK_FALLBACK:
				n_cib = c.Cin // 64 if name in R.HALVES else -(-c.Cin // 32)
				assert dict(splits = splits, cps = cps, last = n_cib - (splits - 1) * cps) == c.edges, (c.name, splits, cps)
	# the finding: the split-K plan sees neither K's halo nor the dilation -- it splits a geometry whose 256-row tile the LDS-DMA kernel refuses
	# ((K - 1) dil = 66 > 64), while the unsplit dispatch serves it on 128-row tiles; convasr_conv1d_fwd_splitk falls back to that launch
	c = R.SPLITK_FALLBACK
	assert (c.K - 1) * c.dil > 64 and R.plan_of(c, 'bf16', bits = R.NO_SHORT)['route'] == 'general' and _route(c, 'bf16', bits = R.NO_SHORT)['route'] == 'general'
	assert _route(c, 'bf16')['route'] == 'lds_dma' and _route(c, 'bf16')['tile_rows'] == 128


# ---- the integer operands stay exact

@pytest.mark.parametrize('table,case_name', EVERY + [('SPLITK', c.name) for c in R.SPLITK])
def test_integer_operands_stay_below_the_exactness_limits(table, case_name):
	"""asserted from the reference itself: every partial sum is at most absdot < 2^24 in magnitude (so every fp32 accumulator, in any order, is
	exact), every 16-bit result is below 60000 (f16 stays finite), and each (tile, column) sum of squares of a case with statistics is below
	2^24 (so are the fp32 per-lane chains inside it) -- forward and, for stride-1 cases, as an input gradient"""
	c = R.by_name(case_name)
	o = R.integer_operands(c)
	ref = R.reference(c, o)
	assert float(ref['absdot'].max()) < 2 ** 24 and float(ref['raw'].abs().max()) < 60000 and float(ref['y'].abs().max()) < 60000, (float(ref['absdot'].max()), float(ref['raw'].abs().max()))
	assert c.epi['stats'] or float(ref['raw'].abs().max()) > 256  # ... and past what bf16 holds exactly (the statistics' limit keeps the cases with statistics smaller)
	if o['scale'] is not None:  # raw * 2^-k + shift is exact in fp32: |raw| < 2^21 and three fractional bits
		assert bool((torch.log2(o['scale']) == torch.log2(o['scale']).round()).all()) and float(o['scale'].min()) >= 0.125 and float(ref['raw'].abs().max()) < 2 ** 20
	if c.epi['stats']:
		for name in c.dtypes:
			p = R.plan_of(c, name)
			sq = (ref['raw'] ** 2).permute(1, 0, 2).reshape(c.Cout, p['B'], p['T'])
			worst = max(float(sq[:, :, t0:t0 + p['tile_rows']].sum(dim = 2).max()) for t0 in range(0, p['T'], p['tile_rows']))
			assert worst < 2 ** 24, (c.name, name, worst)
	if R.has_dgrad(c):
		dy = R.integer_dy(c)
		dx, adx = R.dgrad(dy, o['w'], c.dil, c.pad, c.T), R.dgrad(dy.abs(), o['w'].abs(), c.dil, c.pad, c.T)
		assert float(adx.max()) < 2 ** 24 and float(dx.abs().max()) < 60000


# ---- ops.conv1d's timer label follows the dispatcher

@pytest.mark.parametrize('table,case_name', EVERY)
def test_timer_label_predicates_agree_with_the_route_query(table, case_name):
	"""ops.conv1d books a launch under the LDS-DMA family / the one-tap family for the bench's per-kernel timer: its two predicates against
	the route the library reports, for every case, both switch states"""
	from convasr_amd import ops, _lib
	lib = _lib.load()
	c = R.by_name(case_name)
	e = c.epi
	act = (_lib.ACT_NONE if e['act'] is None else _lib.ACT_RELU if e['act'] == 'relu' else _lib.ACT_HARDTANH, 0.0, 20.0)
	for name in c.dtypes:
		for v2 in (0, 1):
			prev = lib.convasr_debug_set_conv_v2(v2 | (c.bits << 8))
			try:
				dt, yd = R.DTYPES[name], R.DTYPES['f32' if c.out == 'f32' else name]
				v2s, one_tap = ops._conv_label_route(dt, yd, c.B, c.Cin, c.Cout, c.T, R.tout(c), c.K, c.stride, c.dil, c.pad, e['scale'], act, e['xlen'] is not None, e['stats'])
			finally:
				lib.convasr_debug_set_conv_v2(prev)
			route = R.plan_of(c, name, v2 = v2)['route']
			assert (v2s, one_tap) == (route in ('lds_dma', 'one_tap'), route == 'one_tap'), (c.name, name, v2, route, v2s, one_tap)


# ---- the refusals

def test_forward_conv_refuses_before_any_launch():
	"""every refusal is a negative code and a message that names the entry point, from the query and from the call alike; the pointers are never
	dereferenced"""
	from convasr_amd import ops, _lib
	lib = _lib.load()
	p = ctypes.c_void_p(4096)
	rows = ctypes.c_int(-7)
	fwd = lambda xd, yd, B, Cin, Cout, Tin, Tout, K, stride, dil, pad, scale = None, shift = None: lib.convasr_conv1d_fwd(p, p, p, xd, yd, B, Cin, Cout, Tin, Tout, K, stride, dil, pad, None, None, scale, shift, _lib.ACT_NONE, 0.0, 0.0, None, ctypes.byref(rows), None)
	refused = lambda rc, code, text: rc == code and text in lib.convasr_last_error()
	c = R.REFUSED
	prev = lib.convasr_debug_set_conv_v2(0)
	try:
		for name in c.dtypes:  # x_rows 290 > 288 with rows that are no multiple of 16 bytes: the unaligned kernel has no XI = 16 form
			code = _lib.dtype_code(R.DTYPES[name])
			assert c.Cin * (4 if name == 'f32' else 2) % 16 != 0
			got = _route(c, name)
			assert got == dict(route = 'refused', error = R.EUNSUPPORTED) == R.plan_of(c, name) and b'halo too large (x_rows 290)' in lib.convasr_last_error()
			assert refused(fwd(code, code, c.B, c.Cin, c.Cout, c.T, R.tout(c), c.K, c.stride, c.dil, c.pad), R.EUNSUPPORTED, b'conv1d: halo too large (x_rows 290)') and rows.value == -7
			# one tap fewer is served (x_rows 288)
			assert ops.conv_route(R.DTYPES[name], R.DTYPES[name], c.B, c.Cin, c.Cout, c.T, R.out_len(c.T, c.K - 1, 2, 1, c.pad), c.K - 1, 2, 1, c.pad)['x_rows'] == 288
	finally:
		lib.convasr_debug_set_conv_v2(prev)
	bf, f32 = _lib.BF16, _lib.F32
	assert refused(fwd(bf, bf, 2, 64, 64, 100, 101, 3, 1, 1, 1), R.EINVAL, b'conv1d_fwd: Tout 101 inconsistent')
	assert refused(fwd(bf, bf, 0, 64, 64, 100, 100, 3, 1, 1, 1), R.EINVAL, b'conv1d_fwd: bad arguments') and refused(fwd(bf, bf, 2, 64, 64, 100, 100, 3, 0, 1, 1), R.EINVAL, b'conv1d_fwd: bad arguments')
	assert refused(fwd(bf, bf, 2, 64, 64, 100, 100, 3, 1, 1, 1, scale = p), R.EINVAL, b'conv1d_fwd: scale and shift go together')
	assert refused(fwd(_lib.dtype_code(torch.int16), f32, 2, 64, 64, 100, 100, 3, 1, 1, 1), R.EINVAL, b'conv1d_fwd: x dtype')
	assert refused(fwd(f32, bf, 2, 64, 64, 100, 100, 3, 1, 1, 1), R.EUNSUPPORTED, b'conv1d_fwd: dtype 0 -> 1') and refused(fwd(bf, _lib.F16, 2, 96, 64, 100, 100, 3, 1, 1, 1), R.EUNSUPPORTED, b'conv1d_fwd: dtype 1 -> 3')
	assert refused(fwd(f32, f32, 1, 64, 64, 4000, 4000 - 1200, 3, 1, 600, 0), R.EINVAL, b'conv1d_fwd: tile needs')  # a halo of 1200 rows: 2 x 1328 x 128 B of LDS
	assert lib.convasr_conv1d_fwd(None, p, p, bf, bf, 2, 64, 64, 100, 100, 3, 1, 1, 1, None, None, None, None, 0, 0.0, 0.0, None, None, None) == R.EINVAL
	assert lib.convasr_conv1d_fwd(p, p, p, bf, bf, 2, 64, 64, 100, 100, 3, 1, 1, 1, None, p, None, None, 0, 0.0, 0.0, None, None, None) == R.EINVAL and b'stats needs stats_rows' in lib.convasr_last_error()
	# the query answers the same codes
	assert ops.conv_route(torch.bfloat16, torch.bfloat16, 2, 64, 64, 100, 101, 3, 1, 1, 1) == dict(route = 'refused', error = R.EINVAL)
	assert ops.conv_route(torch.float32, torch.bfloat16, 2, 64, 64, 100, 100, 3, 1, 1, 1) == dict(route = 'refused', error = R.EUNSUPPORTED)
	assert R.plan('f32', 'bf16', 2, 64, 64, 100, 100, 3, 1, 1, 1)['error'] == R.EUNSUPPORTED and R.plan('bf16', 'bf16', 2, 64, 64, 100, 101, 3, 1, 1, 1)['error'] == R.EINVAL
	# split-K: a split count that is not the plan's, an output type the kernel does not have
	sk = lambda xd, yd, splits, Cout = 128: lib.convasr_conv1d_fwd_splitk(p, p, p, xd, yd, 1, 256, Cout, 300, 300, 3, 1, 1, None, None, None, 0, 0.0, 0.0, None, splits, p, None)
	assert refused(sk(bf, bf, 3), R.EINVAL, b"conv1d_fwd_splitk: splits 3 is not this geometry's plan") and refused(sk(bf, _lib.F16, 4), R.EINVAL, b'conv1d_fwd_splitk: bad arguments') and refused(sk(bf, bf, 4, Cout = 132), R.EINVAL, b'conv1d_fwd_splitk: bad arguments')
