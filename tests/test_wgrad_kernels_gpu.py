"""Every dense weight-gradient route on the MI355X against the float64 restatement tests/_wgrad_ref.py, at the edges its tables name:
convasr_conv1d_wgrad (the general kernel csrc/conv.hip conv1d_wgrad_kernel in fp32 / bf16 / f16, the LDS-DMA kernel csrc/wgrad_v2.hip in
bf16 / f16), convasr_conv1d_wgrad_ld, convasr_wgrad1x1_grouped, the three combines, the bias gradient (colsum_kernel + colsum_final_kernel,
as dbias and as convasr_colsum) and convasr_fold2_unfold_wgrad behind the folded stride-1 launch.  tests/test_wgrad_ref.py holds the
restatement to float64 autograd and every case to the edge it claims (ring depth, last split, tap group, DMA pieces, alignment, XI), on the CPU.

Protocol of every launch: dw and dbias are views into the middle of a larger buffer of a sentinel, NaN before a plain launch and integers /
random fp32 before an accumulating one; the bytes around the views must be untouched afterwards; the cached 'wgrad' workspace is filled
with 0xFF bytes first, so a slab entry that is summed but never written shows as NaN; a second launch gives the same bits (no float atomics).

Three checks:
 (a) integer operands from -1 ... 6, bit for bit: every product and partial sum is an integer below 36 B Tout < 2^24, so every summation
     order is exact in fp32 and the result must EQUAL the float64 sum (start + sum when accumulating).  A partial rounded to 16 bits, a
     dropped or doubled frame, a frame read from the neighbouring utterance shows as a small integer, printed with its (co, ci, k).
 (b) random operands rounded to the storage type, element-wise: |got - ref| <= 2 n u absdot + 2^-126 with n = B Tout + splits, u = 2^-24,
     absdot = sum |dy| |x|: the standard bound gamma_(n-1) sum |a_i b_i| of ANY summation order of exactly representable products, doubled for
     the matrix pipe's internal adds (whose rounding the ISA does not promise to be nearest-even) and the rounded products of fp32 operands.
     An accumulating launch has one more term, its start.  Nothing in it is measured.
 (c) random operands, norm-wise on the 32 x 32 corner: ||got - ref||_F <= FACTOR ||chain32 - ref||_F, chain32 = the same sum in ONE fp32
     accumulator per element, frame after frame (the least accurate order a plain fp32 kernel could use).  FACTOR = 4 is not measured: it
     allows for the pipe's rounding mode and for short chains, where both errors are a few ulp; the bias gradient's is 8 (see FACTOR).
     Every case prints both norms (WGRAD lines); the table is in profiles/NOTEBOOK.md, section 19.

No test of this file found a wrong result in the kernels: the one change to the library is the plan query the tables are held to."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wgrad_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float('nan')
SENTINEL = -12345.0
GUARD = 64  # floats of sentinel on either side of a view (16-byte aligned views: the tap-major combine moves float4s)
# (c): 4 for every route, not measured.  The bias gradient's is raised to 8, the next power of two that holds, after 4.12 was measured on one
# case (140 rows of f16, 32 columns: the chain is off by one ulp in ONE column, 2.4e-7, the kernel by one ulp in several -- its four waves carry
# four 35-row chains that meet in three more fp32 adds at the full sum's magnitude, where the chain's last adds happened to be exact); every other
# ratio measured is at most 1.3 (profiles/NOTEBOOK.md, section 19)
FACTOR = dict(general = 4.0, lds_dma = 4.0, grouped = 4.0, dbias = 8.0)
LAYOUTS = ('reference', 'tap_major')


def dev():
	return torch.device('cuda:0')


def cl(t, dtype):
	"""logical (B, C, T) fp32 values -> channels-last tensor of the storage type on the device (memory [B][T][C])"""
	B, C, T = t.shape
	out = torch.empty(B, T, C, dtype = dtype, device = dev()).permute(0, 2, 1)
	out.copy_(t)
	return out


class Arena:
	"""a (Cout, Cin, K) gradient (or a (C,) bias gradient) as a view into the middle of a buffer of SENTINEL"""

	def __init__(self, shape, layout = 'reference', start = None):
		n = 1
		for s in shape:
			n *= s
		self.n = n
		self.buf = torch.full((GUARD + n + GUARD, ), SENTINEL, device = dev())
		flat = self.buf[GUARD:GUARD + n]
		if layout == 'tap_major':
			Cout, Cin, K = shape
			self.view = flat.view(K, Cout, Cin).permute(1, 2, 0)
		else:
			self.view = flat.view(*shape)
		if start is None:
			flat.fill_(NAN)
		else:
			self.view.copy_(start.to(dev()))

	def intact(self):
		g = self.buf.cpu()
		return bool((g[:GUARD] == SENTINEL).all()) and bool((g[GUARD + self.n:] == SENTINEL).all())

	def result(self, what):
		assert self.intact(), f'{what}: the bytes around the view were written'
		return self.view.detach().cpu().double()


def exact(got, ref, what):
	"""(a)"""
	if torch.equal(got, ref):
		return
	bad = (got != ref)
	idx = tuple(bad.nonzero()[0].tolist())
	raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements wrong, the first at {idx} ((co, ci, k) of a dw): got - ref = {float(got[idx] - ref[idx])} (got {float(got[idx])})')


def bounded(got, ref, absdot, n, what):
	"""(b)"""
	assert bool(torch.isfinite(got).all()), f'{what}: non-finite result'
	excess = (got - ref).abs() - (2 * n * R.U32 * absdot + R.TINY)
	assert float(excess.max()) <= 0, f'{what}: |got - ref| exceeds 2 n u absdot + tiny (n = {n}) by {float(excess.max()):.3e} at {tuple((excess == excess.max()).nonzero()[0].tolist())}'


def corner_norms(got, ref, chain, route, tag):
	"""(c): got, ref already cut to what chain covers"""
	bar = FACTOR[route]
	tag = f'{route} {tag}'
	e_gpu, e_chain = float((got - ref).norm()), float((torch.from_numpy(chain).double().reshape(ref.shape) - ref).norm())
	ratio = e_gpu / e_chain if e_chain > 0 else (0.0 if e_gpu == 0 else float('inf'))
	print(f'    WGRAD {tag}: gpu {e_gpu:.3e} chain32 {e_chain:.3e} ratio {ratio:.3f} (bar {bar:g})')
	assert e_gpu <= bar * e_chain, f'{tag}: ||got - ref|| = {e_gpu:.3e} > {bar:g} x ||chain32 - ref|| = {e_chain:.3e}'


def poison(nbytes, tag = 'wgrad'):
	from convasr_amd import ops
	ws = ops.workspace(nbytes, dev(), tag)
	ws[:max(int(nbytes), 16)].fill_(0xFF)
	return ws


def wgrad_workspace(c):
	from convasr_amd import _lib
	return poison(_lib.load().convasr_conv1d_wgrad_workspace_bytes(c.B, c.Cin, c.Cout, R.tin(c), c.Tout, c.K, c.stride, c.dil))


class switch:
	"""convasr_debug_set_conv_v2(state) for the block, the previous state restored behind it"""

	def __init__(self, state):
		self.state = state

	def __enter__(self):
		from convasr_amd import _lib
		self.prev = _lib.load().convasr_debug_set_conv_v2(self.state)

	def __exit__(self, *exc):
		from convasr_amd import _lib
		_lib.load().convasr_debug_set_conv_v2(self.prev)


TABLES = dict(lds = R.LDS_DMA, gen = R.GENERAL)
BY_NAME = {(t, c.name): c for t, cases in TABLES.items() for c in cases}


def shape5(c):
	return (c.B, c.Cin, R.tin(c), c.Cout, c.Tout)


@functools.lru_cache(maxsize = None)
def integer_case(table, cname):
	"""(x, dy, dw, dbias) of a case on integer data (the same for every dtype: the integers are exact in all three), computed once"""
	c = BY_NAME[table, cname]
	x, dy = R.integer_operands(shape5(c), len(cname) + c.Tout)
	dw, db, _ = R.wgrad(x, dy, c.K, c.stride, c.dil, c.pad)
	assert float(dw.abs().max()) < 2 ** 24 - 2 ** 21 and float(db.abs().max()) < 2 ** 24 - 2 ** 21
	return x, dy, dw, db


@functools.lru_cache(maxsize = None)
def random_case(table, cname, name):
	"""(x, dy, dw, dbias, absdot, chain32, chain32 of dbias) on randn rounded to the storage type, computed once and left unchanged"""
	c = BY_NAME[table, cname]
	x, dy = R.random_operands(shape5(c), len(cname) + c.Tout + 1, R.DTYPES[name])
	dw, db, absdot = R.wgrad(x, dy, c.K, c.stride, c.dil, c.pad)
	return x, dy, dw, db, absdot, R.chain32(x, dy, c.K, c.stride, c.dil, c.pad), R.chain32_rows(dy.permute(0, 2, 1).reshape(-1, c.Cout))


def launch(c, xg, dyg, layout, start_w = None, start_b = None):
	"""one ops.conv1d_wgrad launch into fresh arenas; (dw arena, dbias arena)"""
	from convasr_amd import ops
	dw, db = Arena((c.Cout, c.Cin, c.K), layout, start_w), Arena((c.Cout, ), 'reference', start_b)
	wgrad_workspace(c)
	ops.conv1d_wgrad(xg, dyg, c.Cout, c.K, c.stride, c.dil, c.pad, dw.view, dbias = db.view, accumulate = start_w is not None)
	return dw, db


def run_case(table, c, name):
	"""checks (a), (b), (c) of one case in one dtype, both gradient layouts, plain and accumulating"""
	from convasr_amd import ops
	dt = R.DTYPES[name]
	plan = ops.wgrad_plan(dt, c.B, c.Cin, c.Cout, R.tin(c), c.Tout, c.K, c.stride, c.dil)
	assert plan['route'] == c.edges[name]['route'], (c.name, plan)
	n = c.B * c.Tout + plan['splits']
	g = torch.Generator().manual_seed(c.Tout)
	layouts = LAYOUTS if (c.Cout * c.Cin) % 4 == 0 else LAYOUTS[:1]
	# (a)
	x, dy, dw_ref, db_ref = integer_case(table, c.name)
	xg, dyg = cl(x, dt), cl(dy, dt)
	for layout in layouts:
		what = f'{c.name} {name} {layout} integers'
		dw, db = launch(c, xg, dyg, layout)
		first_w, first_b = dw.result(what), db.result(what)
		exact(first_w, dw_ref, what + ' dw')
		exact(first_b, db_ref, what + ' dbias')
		dw, db = launch(c, xg, dyg, layout)
		assert torch.equal(dw.result(what), first_w) and torch.equal(db.result(what), first_b), what + ': a second launch differs'
		sw, sb = torch.randint(-2 ** 20, 2 ** 20, dw_ref.shape, generator = g).float(), torch.randint(-2 ** 20, 2 ** 20, db_ref.shape, generator = g).float()
		dw, db = launch(c, xg, dyg, layout, sw, sb)
		exact(dw.result(what), sw.double() + dw_ref, what + ' dw accumulate')
		exact(db.result(what), sb.double() + db_ref, what + ' dbias accumulate')
	# (b), (c)
	x, dy, dw_ref, db_ref, absdot, chain, chain_b = random_case(table, c.name, name)
	xg, dyg = cl(x, dt), cl(dy, dt)
	absdot_b = dy.double().abs().sum(dim = (0, 2))
	for layout in layouts:
		what = f'{c.name} {name} {layout} random'
		dw, db = launch(c, xg, dyg, layout)
		first_w, first_b = dw.result(what), db.result(what)
		bounded(first_w, dw_ref, absdot, n, what + ' dw')
		bounded(first_b, db_ref, absdot_b, c.B * c.Tout + 1, what + ' dbias')
		if layout == layouts[0]:
			corner_norms(first_w[:R.CORNER, :R.CORNER], dw_ref[:R.CORNER, :R.CORNER], chain, plan['route'], f'{name} {c.name} dw')
			corner_norms(first_b[:R.CORNER], db_ref[:R.CORNER], chain_b, 'dbias', f'{name} {c.name}')
		else:
			assert torch.equal(first_w, prev_w), what + ': the two layouts differ (the same slabs, the same order of summation)'
		prev_w = first_w
		dw, db = launch(c, xg, dyg, layout)
		assert torch.equal(dw.result(what), first_w) and torch.equal(db.result(what), first_b), what + ': a second launch differs'
		sw, sb = torch.randn(dw_ref.shape, generator = g), torch.randn(db_ref.shape, generator = g)
		dw, db = launch(c, xg, dyg, layout, sw, sb)
		bounded(dw.result(what), sw.double() + dw_ref, absdot + sw.double().abs(), n + 1, what + ' dw accumulate')
		bounded(db.result(what), sb.double() + db_ref, absdot_b + sb.double().abs(), c.B * c.Tout + 2, what + ' dbias accumulate')


def _params(table):
	return [pytest.param(c.name, name, id = f'{c.name}-{name}') for c in TABLES[table] for name in c.edges]


@pytest.mark.parametrize('cname,name', _params('lds'))
def test_lds_dma_kernel(cname, name):
	"""csrc/wgrad_v2.hip at every tap-group instantiation, every DMA piece count of its envelope (and one step past it, where the general
	kernel takes over), ring depths 1 ... 12 chunks per split with short last splits, every kind of padding, a truncated Tout and the
	tap-major combine's capped grid."""
	c = BY_NAME['lds', cname]
	with switch(c.v2):
		run_case('lds', c, name)


@pytest.mark.parametrize('cname,name', _params('gen'))
def test_general_kernel(cname, name):
	"""csrc/conv.hip conv1d_wgrad_kernel in fp32, bf16 and f16: one frame, the four alignment instantiations, the XI = 5 / 12 boundary, the
	widest tap window it takes, ragged tiles, K = 64, up to 15 chunks per split, a truncated Tout."""
	c = BY_NAME['gen', cname]
	with switch(c.v2):
		run_case('gen', c, name)


@pytest.mark.parametrize('cname', R.SAME_BITS)
def test_both_kernels_give_the_same_bits_on_integer_data(cname):
	from convasr_amd import ops
	c = BY_NAME['lds', cname]
	x, dy, dw_ref, db_ref = integer_case('lds', cname)
	for name in c.edges:
		dt = R.DTYPES[name]
		xg, dyg = cl(x, dt), cl(dy, dt)
		got = {}
		for state in (1, 0):
			with switch(state):
				assert ops.wgrad_plan(dt, c.B, c.Cin, c.Cout, R.tin(c), c.Tout, c.K, c.stride, c.dil)['route'] == ('lds_dma' if state else 'general')
				dw, db = launch(c, xg, dyg, 'reference')
				got[state] = dw.result(cname)
		exact(got[0], dw_ref, f'{cname} {name} switch off')
		assert torch.equal(got[0], got[1])


# ---- the in-place plane read

def plane_tensor(t, dtype):
	"""logical (B, C, T) values as plane 0 of a [B][T][3][C] tensor whose planes 1 and 2 are NaN, returned as the (B, 3 C, T) channels-last tensor"""
	B, C, T = t.shape
	m = torch.full((B, T, 3, C), NAN, dtype = dtype, device = dev())
	m[:, :, 0, :] = t.permute(0, 2, 1).to(dtype).to(dev())
	return m.view(B, T, 3 * C).permute(0, 2, 1)


@pytest.mark.parametrize('cname', [c.name for c in R.STARRED])
@pytest.mark.parametrize('name', R.HALVES)
def test_in_place_plane_read(cname, name):
	"""ops.conv1d_wgrad_hi (x read as plane 0 of a plane tensor, frames 3 Cin elements apart) and convasr_conv1d_wgrad_ld with dy a plane too
	(dy_ld = 3 Cout): the NaN planes next to the operands must never be read.  (a) on integers, (b) on random data, and the bits of the dense launch."""
	from convasr_amd import ops, _lib
	c = BY_NAME['lds', cname]
	dt = R.DTYPES[name]
	Tin = R.tin(c)
	assert ops.wgrad_plan(dt, c.B, c.Cin, c.Cout, Tin, c.Tout, c.K, 1, c.dil, x_ld = 3 * c.Cin, dy_ld = 3 * c.Cout)['route'] == 'lds_dma'
	plan = ops.wgrad_plan(dt, c.B, c.Cin, c.Cout, Tin, c.Tout, c.K, 1, c.dil, x_ld = 3 * c.Cin)
	assert plan['route'] == 'lds_dma' and plan == ops.wgrad_plan(dt, c.B, c.Cin, c.Cout, Tin, c.Tout, c.K, 1, c.dil)
	g = torch.Generator().manual_seed(7)

	def ld(x3, dy3, dw, accumulate, layout):
		ws = wgrad_workspace(c)
		_lib.call('convasr_conv1d_wgrad_ld', x3.data_ptr(), 3 * c.Cin, dy3.data_ptr(), 3 * c.Cout, dw.view.data_ptr(), ws.data_ptr(), _lib.dtype_code(dt), c.B, c.Cin, c.Cout, Tin, c.Tout, c.K, c.dil, c.pad,
		          int(accumulate), _lib.W_KMAJOR if layout == 'tap_major' else _lib.W_REFERENCE, _lib.stream_ptr())

	x, dy, dw_ref, _ = integer_case('lds', cname)
	x3, dy3, dyg = plane_tensor(x, dt), plane_tensor(dy, dt), cl(dy, dt)
	for layout in LAYOUTS:
		what = f'{cname} {name} {layout} plane'
		dw = Arena(dw_ref.shape, layout)
		wgrad_workspace(c)
		ops.conv1d_wgrad_hi(x3, dyg, c.Cout, c.K, c.dil, c.pad, dw.view)
		exact(dw.result(what), dw_ref, what)
		sw = torch.randint(-2 ** 20, 2 ** 20, dw_ref.shape, generator = g).float()
		dw = Arena(dw_ref.shape, layout, sw)
		wgrad_workspace(c)
		ops.conv1d_wgrad_hi(x3, dyg, c.Cout, c.K, c.dil, c.pad, dw.view, accumulate = True)
		exact(dw.result(what), sw.double() + dw_ref, what + ' accumulate')
		dw = Arena(dw_ref.shape, layout)
		ld(x3, dy3, dw, False, layout)
		exact(dw.result(what), dw_ref, what + ', dy a plane too')
		dw = Arena(dw_ref.shape, layout, sw)
		ld(x3, dy3, dw, True, layout)
		exact(dw.result(what), sw.double() + dw_ref, what + ', dy a plane too, accumulate')
	x, dy, dw_ref, _, absdot, _, _ = random_case('lds', cname, name)
	x3, dy3 = plane_tensor(x, dt), plane_tensor(dy, dt)
	dense, _ = launch(c, cl(x, dt), cl(dy, dt), 'reference')
	for fn in (lambda dw: ops.conv1d_wgrad_hi(x3, cl(dy, dt), c.Cout, c.K, c.dil, c.pad, dw.view), lambda dw: ld(x3, dy3, dw, False, 'reference')):
		dw = Arena(dw_ref.shape)
		wgrad_workspace(c)
		fn(dw)
		got = dw.result(cname)
		bounded(got, dw_ref, absdot, c.B * c.Tout + plan['splits'], f'{cname} {name} plane random')
		assert torch.equal(got, dense.result(cname)), 'the in-place read and the dense launch differ'


@pytest.mark.parametrize('name', R.HALVES)
def test_plane_outside_the_envelope_is_copied_out(name):
	from convasr_amd import ops, _lib
	dt = R.DTYPES[name]
	c = R.case('plane_cin64', (2, 64, 128, 150, 3, 1, 1), {})
	assert _lib.load().convasr_conv1d_wgrad_ld_supported(_lib.dtype_code(dt), c.B, c.Cin, c.Cout, R.tin(c), c.Tout, c.K, c.dil, 3 * c.Cin, c.Cout) == 0
	x, dy = R.integer_operands(shape5(c), 11)
	dw_ref, _, _ = R.wgrad(x, dy, c.K, 1, c.dil, c.pad)
	x3, dyg = plane_tensor(x, dt), cl(dy, dt)
	for layout in LAYOUTS:
		dw = Arena(dw_ref.shape, layout)
		wgrad_workspace(c)
		ops.conv1d_wgrad_hi(x3, dyg, c.Cout, c.K, c.dil, c.pad, dw.view)
		exact(dw.result(layout), dw_ref, f'dense-copy path {name} {layout}')


# ---- the reference-layout combine

@pytest.mark.parametrize('name', ['f32', 'bf16'])
def test_reference_layout_combine_blocks(name):
	"""wgrad_reduce_kernel: 64-column blocks of Cin (24, 64, 65, 129: less than one, one, one and a column, two and a column) and its
	k += 4 loop (K = 1, 3, 4, 5, 64), through the C entry point so that one tap keeps the reference layout"""
	from convasr_amd import _lib
	dt = R.DTYPES[name]
	g = torch.Generator().manual_seed(5)
	for Cin in R.REDUCE_CIN:
		for K in R.REDUCE_K:
			c = R.case(f'reduce_{Cin}_{K}', (2, Cin, 6, 37, K, 1, 1), {})
			x, dy = R.integer_operands(shape5(c), Cin + K)
			dw_ref, _, _ = R.wgrad(x, dy, K, 1, 1, c.pad)
			xg, dyg = cl(x, dt), cl(dy, dt)
			for start in (None, torch.randint(-2 ** 20, 2 ** 20, dw_ref.shape, generator = g).float()):
				dw = Arena(dw_ref.shape, 'reference', start)
				ws = wgrad_workspace(c)
				_lib.call('convasr_conv1d_wgrad', xg.data_ptr(), dyg.data_ptr(), dw.view.data_ptr(), None, ws.data_ptr(), _lib.dtype_code(dt), c.B, Cin, c.Cout, R.tin(c), c.Tout, K, 1, 1, c.pad,
				          int(start is not None), _lib.W_REFERENCE, _lib.stream_ptr())
				exact(dw.result(c.name), dw_ref if start is None else start.double() + dw_ref, f'{c.name} {name} accumulate {start is not None}')


# ---- the bias gradient

@functools.lru_cache(maxsize = None)
def bias_data(rows, C, name):
	g = torch.Generator().manual_seed(rows + C)
	yi = torch.randint(-1, 7, (1, C, rows), generator = g).float()
	yr = torch.randn(1, C, rows, generator = g).to(R.DTYPES[name]).float()
	return yi, yi.double().sum(dim = (0, 2)), yr, yr.double().sum(dim = (0, 2)), yr.double().abs().sum(dim = (0, 2)), R.chain32_rows(yr[0].t())


@pytest.mark.parametrize('rows', R.BIAS_ROWS)
@pytest.mark.parametrize('name', R.ALL)
def test_bias_gradient(rows, name):
	"""colsum_kernel (256 rows per block, four waves of row-strided sums) + colsum_final_kernel (partial rows over 16 row-lanes: 4097 rows make the
	17th partial row, 70001 rows 274) as ops.colsum and as the dbias of the entry point, C = 1 ... 200 (one channel, a ragged block, one
	block, one and a channel, four blocks), with and without accumulate: (a), (b), (c)"""
	from convasr_amd import ops, _lib
	dt = R.DTYPES[name]
	lib = _lib.load()
	g = torch.Generator().manual_seed(rows)
	Cin = 8
	x8 = torch.zeros(1, 8, rows, dtype = dt, device = dev()).permute(0, 2, 1).contiguous().permute(0, 2, 1)
	pooled = dict(colsum = [], dbias = [])  # (c) over the columns of every C together: one column or a few are no norm to speak of
	for C in R.BIAS_C:
		yi, ref_i, yr, ref_r, abs_r, chain = bias_data(rows, C, name)

		def colsum(y, out, accumulate):
			poison(lib.convasr_colsum_workspace_bytes(rows, C), 'colsum')
			ops.colsum(y, out.view, accumulate = accumulate)

		def dbias(y, out, accumulate):
			c = R.case('dbias', (1, Cin, C, rows, 1, 1, 1), {})
			ws = wgrad_workspace(c)
			dw = Arena((C, Cin, 1), start = torch.zeros(C, Cin, 1) if accumulate else None)  # (x is zero: the weight gradient is 0, and 0 + 0)
			_lib.call('convasr_conv1d_wgrad', x8.data_ptr(), y.data_ptr(), dw.view.data_ptr(), out.view.data_ptr(), ws.data_ptr(), _lib.dtype_code(dt), 1, Cin, C, rows, rows, 1, 1, 1, 0, int(accumulate), _lib.W_REFERENCE, _lib.stream_ptr())
			assert dw.intact() and bool((dw.view == 0).all())

		for path, fn in (('colsum', colsum), ('dbias', dbias)):
			what = f'{path} {name} rows {rows} C {C}'
			yg = cl(yi, dt)
			out = Arena((C, ))
			fn(yg, out, False)
			exact(out.result(what), ref_i, what + ' integers')
			si = torch.randint(-2 ** 20, 2 ** 20, (C, ), generator = g).float()
			out = Arena((C, ), start = si)
			fn(yg, out, True)
			exact(out.result(what), si.double() + ref_i, what + ' integers accumulate')
			yg = cl(yr, dt)
			out = Arena((C, ))
			fn(yg, out, False)
			first = out.result(what)
			bounded(first, ref_r, abs_r, rows + 1, what + ' random')
			pooled[path].append((first[:R.CORNER], ref_r[:R.CORNER], torch.from_numpy(chain)))
			out = Arena((C, ))
			fn(yg, out, False)
			assert torch.equal(out.result(what), first), what + ': a second launch differs'
			sr = torch.randn(C, generator = g)
			out = Arena((C, ), start = sr)
			fn(yg, out, True)
			bounded(out.result(what), sr.double() + ref_r, abs_r + sr.double().abs(), rows + 2, what + ' random accumulate')
	for path, parts in pooled.items():
		corner_norms(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]).numpy(), 'dbias', f'{path} {name} rows {rows}')


# ---- the grouped one-tap launch

@pytest.mark.parametrize('index', range(len(R.GROUPED)))
@pytest.mark.parametrize('name', R.HALVES)
def test_grouped_one_tap_launch(index, name):
	"""ops.wgrad1x1_grouped: 1, 2, 5 and 12 problems of mixed channel counts over the same frames, accumulate mixed per problem, a bias
	gradient to zero for some problems and none for the others (NaN before, exactly 0.0 after; the others untouched); each problem against
	its own float64 reference by (a), (b), (c)"""
	from convasr_amd import ops, _lib
	dt = R.DTYPES[name]
	(B, T), probs, (splits, cps) = R.GROUPED[index]
	n = len(probs)
	cins, couts = [p[0] for p in probs], [p[1] for p in probs]
	assert ops.wgrad1x1_grouped_plan(dt, cins, couts, B, T) == (splits, cps)
	nbytes = _lib.load().convasr_wgrad1x1_grouped_workspace_bytes(n, ops._int_array(cins), ops._int_array(couts), B, T)
	g = torch.Generator().manual_seed(index)
	acc = [i % 2 for i in range(n)]
	for kind in ('integers', 'random'):
		data = [R.integer_operands((B, ci, T, co, T), 31 * index + i) if kind == 'integers' else R.random_operands((B, ci, T, co, T), 31 * index + i, dt) for i, (ci, co) in enumerate(probs)]
		refs = [R.wgrad(x, dy, 1, 1, 1, 0) for x, dy in data]
		xs, dys = [cl(x, dt) for x, _ in data], [cl(dy, dt) for _, dy in data]
		starts = [(torch.randint(-2 ** 20, 2 ** 20, r[0].shape, generator = g).float() if kind == 'integers' else torch.randn(r[0].shape, generator = g)) if a else None for r, a in zip(refs, acc)]
		first = None
		for attempt in range(2):
			dws = [Arena(r[0].shape, 'reference', s) for r, s in zip(refs, starts)]
			zeros = [Arena((co, )) if i % 3 == 0 else None for i, co in enumerate(couts)]
			poison(nbytes)
			assert ops.wgrad1x1_grouped(xs, dys, [d.view for d in dws], zeros = [z.view if z is not None else None for z in zeros], accumulate = acc)
			got = [d.result(f'grouped problem {i}') for i, d in enumerate(dws)]
			for i, z in enumerate(zeros):
				if z is not None:
					r = z.result(f'zeros {i}')
					assert torch.equal(r, torch.zeros_like(r)) and not bool(torch.signbit(r).any()), f'zeros {i}'
			if first is not None:
				assert all(torch.equal(a, b) for a, b in zip(first, got)), 'a second launch differs'
			first = got
		for i, ((dw_ref, _, absdot), s) in enumerate(zip(refs, starts)):
			what = f'grouped {name} frames {(B, T)} problem {i} of {n} {probs[i]} {kind}'
			if kind == 'integers':
				exact(got[i], dw_ref if s is None else s.double() + dw_ref, what)
			else:
				bounded(got[i], dw_ref if s is None else s.double() + dw_ref, absdot if s is None else absdot + s.double().abs(), B * T + splits + (s is not None), what)
				if s is None:
					x, dy = data[i]
					corner_norms(got[i][:R.CORNER, :R.CORNER], dw_ref[:R.CORNER, :R.CORNER], R.chain32(x, dy, 1, 1, 1, 0), 'grouped', f'{name} {(B, T)} x {n} problem {i}')


# ---- the stride-2 fold

@pytest.mark.parametrize('geometry', R.FOLD, ids = lambda g: 'x'.join(map(str, g)))
@pytest.mark.parametrize('name', R.HALVES)
def test_stride2_fold(geometry, name):
	"""the folded stride-1 launch on the (B, 2 Cin, T / 2) view with (K', P') and the stride-2 conv's own Tout (one frame fewer than the folded
	geometry yields where pad is odd), then convasr_fold2_unfold_wgrad: the float64 stride-2 gradient bit for bit on integers, both dw
	layouts, with and without accumulate; the folded taps outside [0, K) do not leak in"""
	from convasr_amd import ops
	dt = R.DTYPES[name]
	Cout, Cin, K, pad = geometry
	B, Tin = R.FOLD_B, R.FOLD_TIN
	Kf, Pf = ops.fold2_geometry(K, pad)
	assert (Kf, Pf) == R.fold2(K, pad)[:2]
	Tout = (Tin + 2 * pad - (K - 1) - 1) // 2 + 1
	folded_full = Tin // 2 + 2 * Pf - Kf + 1
	assert Tout <= folded_full and (folded_full - Tout == 1) == (pad % 2 == 1)
	x, dy = R.integer_operands((B, Cin, Tin, Cout, Tout), K + pad)
	dw_ref, _, _ = R.wgrad(x, dy, K, 2, 1, pad)
	dwf_ref, _, _ = R.wgrad(R.fold_view(x), dy, Kf, 1, 1, Pf)
	xg, dyg = cl(x, dt), cl(dy, dt)
	xv = xg.as_strided((B, 2 * Cin, Tin // 2), (Tin * Cin, 1, 2 * Cin))
	fc = R.case('folded', (B, 2 * Cin, Cout, Tout, Kf, 1, 1), {}, pad = Pf, trunc = folded_full - Tout)
	assert R.tin(fc) == Tin // 2
	g = torch.Generator().manual_seed(K)
	dwf = Arena((Cout, 2 * Cin, Kf), 'tap_major')
	wgrad_workspace(fc)
	ops.conv1d_wgrad(xv, dyg, Cout, Kf, 1, 1, Pf, dwf.view)
	exact(dwf.result('folded'), dwf_ref, f'folded launch {geometry} {name}')
	dwf_mem = dwf.buf[GUARD:GUARD + dwf.n].view(Kf, Cout, 2 * Cin)
	for layout in LAYOUTS:
		for start in (None, torch.randint(-2 ** 20, 2 ** 20, dw_ref.shape, generator = g).float()):
			dw = Arena(dw_ref.shape, layout, start)
			ops.fold2_unfold_wgrad(dwf_mem, dw.view, pad, accumulate = start is not None)
			exact(dw.result('unfold'), dw_ref if start is None else start.double() + dw_ref, f'unfold {geometry} {name} {layout} accumulate {start is not None}')
	assert dwf.intact() and torch.equal(dwf.result('folded'), dwf_ref)
