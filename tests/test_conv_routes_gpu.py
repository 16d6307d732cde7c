"""Every forward / dgrad conv route against float64 at its edges: the register-staged kernel (csrc/conv.hip), the LDS-DMA kernel
(csrc/conv_v2s.hip) and the one-tap kernel (csrc/conv1x1.hip), at the shapes tests/_conv_ref.py's tables hold to the instantiation they claim
(tests/test_conv_ref.py asks the library's own route query), the split-K launches, and the weight packers.

Protocol of every launch (launch() below): x, the packed weights and y are views into the middle of larger buffers; the guards around x
and w hold NaN (a read the buffer descriptor should have zeroed shows up as NaN in the output), y is NaN before the launch (a tile that is
never written shows up) and the guards around it hold a sentinel that must be intact afterwards; the statistics rows and the split-K
workspace start as 0xFF bytes; the rows the launch reports are the route query's; a second launch gives the same bits.

Three checks, as in tests/test_wgrad_kernels_gpu.py:
  (a) integer operands, bit for bit: fp32 outputs and the statistics equal the float64 result, 16-bit outputs equal round16 of it, frames at
      or past valid_len are +0.  A failure prints the first wrong (b, t, co) and the difference: a small integer there is a dropped tap or a
      neighbour's frame.
  (b) random operands, element-wise, against the derived bar of _conv_ref.bound / stats_bound (nothing measured).
  (c) random operands, fp32-output launches (fp32, the wide head, split-K): on the corner of the first 32 output channels
      ||got - ref||_F <= FACTOR ||chain32 - ref||_F; every case prints a CONV line (profiles/NOTEBOOK.md, section 20).

Findings.  test_split_k_request_outside_the_lds_dma_envelope_is_served_by_the_unsplit_launch pins the one defect read from the dispatcher:
convasr_conv1d_fwd_splitk_plan splits a geometry whose halo the LDS-DMA kernel cannot hold at 256-row tiles ((K - 1) dil > 64), and
convasr_conv1d_fwd_splitk then failed with CONVASR_EUNSUPPORTED where the unsplit call serves the request; it now runs the unsplit launch
with the caller's epilogue.  Apart from that the tests below found nothing wrong in the kernels."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# Check (c)'s bar, not a measured number: the weight-gradient suite's 4.  chain32 is the least accurate order a plain fp32 kernel could
# use, so a kernel that keeps fp32 accumulators stays below 1; 4 leaves room for a chain that happens to round luckily.
FACTOR = 4.0
GUARD = 4096      # elements on either side of every operand
SENTINEL = -7.0   # exact in every storage type


def dev():
	return torch.device('cuda:0')


def _ids(cases):
	return [f'{c.name}-{n}' for c in cases for n in c.dtypes]


def _pairs(cases):
	return [(c, n) for c in cases for n in c.dtypes]


# ---- the launch protocol

def _guarded(values, dtype, fill):
	"""a flat device buffer [guard | values | guard] and the view of its middle, shaped like `values` (a CPU tensor, or a shape to leave NaN)"""
	shape = tuple(values.shape) if isinstance(values, torch.Tensor) else tuple(values)
	n = 1
	for s in shape:
		n *= s
	buf = torch.full((2 * GUARD + n, ), fill, dtype = dtype, device = dev())
	mid = buf[GUARD:GUARD + n].view(shape)
	if isinstance(values, torch.Tensor):
		mid.copy_(values.to(dtype))
	else:
		mid.fill_(float('nan'))
	return buf, mid


def _guards_intact(buf, n):
	return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def _cl(t):
	"""logical (B, C, T) -> the kernels' channels-last memory (B, T, C)"""
	return t.permute(0, 2, 1).contiguous()


def _act(act):
	from convasr_amd import _lib
	return (_lib.ACT_NONE, 0.0, 0.0) if act is None else (_lib.ACT_RELU, 0.0, 0.0) if act == 'relu' else (_lib.ACT_HARDTANH, float(act[1]), float(act[2]))


def _f32(t):
	return None if t is None else t.float().to(dev())


def launch(name, out_name, x, packed, geom, epi = None, act = None, want_stats = False, bits = 0, v2 = 1, splits = 0):
	"""One conv launch under the protocol.  x: logical (B, Cin, Tin) CPU tensor of storage-type values; packed: the packed weight (device);
	geom = (B, Cin, Cout, Tin, Tout, K, stride, dil, pad); epi: dict(bias, scale, shift, xlen) of CPU tensors or None; splits > 0: through
	convasr_conv1d_fwd_splitk.  Returns dict(y = logical (B, Cout, Tout) CPU tensor of the output type, stats = (sum, sumsq) float64 or None, route)."""
	from convasr_amd import ops, _lib
	lib = _lib.load()
	B, Cin, Cout, Tin, Tout, K, stride, dil, pad = geom
	dt, odt = R.DTYPES[name], R.DTYPES[out_name]
	epi = epi or {}
	bias, scale, shift, xlen = (_f32(epi.get(k)) for k in ('bias', 'scale', 'shift', 'xlen'))
	a = _act(act)
	p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
	prev = lib.convasr_debug_set_conv_v2(v2 | (bits << 8))
	try:
		route = ops.conv_route(dt, odt, B, Cin, Cout, Tin, Tout, K, stride, dil, pad, scale = scale is not None, act = a[0], xlen = xlen is not None, stats = want_stats)
		assert route['route'] != 'refused', (geom, route)
		_, xg = _guarded(_cl(x), dt, float('nan'))
		_, wg = _guarded(packed.cpu().float(), dt, float('nan'))
		n_y = B * Tout * Cout
		max_rows = lib.convasr_conv_stats_max_rows(B, Tout)
		outs = []
		for attempt in range(2):
			ybuf, yg = _guarded((B, Tout, Cout), odt, SENTINEL)
			sbuf = torch.full((max(max_rows, 1) * 2 * Cout * 8, ), 255, dtype = torch.uint8, device = dev()).view(torch.float64) if want_stats else None
			rows = ctypes.c_int(-1)
			if splits:
				ws = torch.full((splits * n_y * 4 + 256, ), 255, dtype = torch.uint8, device = dev())
				_lib.call('convasr_conv1d_fwd_splitk', p(xg), p(wg), p(yg), _lib.dtype_code(dt), _lib.dtype_code(odt), B, Cin, Cout, Tin, Tout, K, dil, pad, p(bias), p(scale), p(shift), a[0], a[1], a[2], p(xlen), splits, p(ws), _lib.stream_ptr())
			else:
				_lib.call('convasr_conv1d_fwd', p(xg), p(wg), p(yg), _lib.dtype_code(dt), _lib.dtype_code(odt), B, Cin, Cout, Tin, Tout, K, stride, dil, pad, p(bias), p(sbuf), p(scale), p(shift), a[0], a[1], a[2], p(xlen), ctypes.byref(rows) if want_stats else None, _lib.stream_ptr())
			torch.cuda.synchronize()
			assert _guards_intact(ybuf, n_y), ('a write outside y', geom)
			st = None
			if want_stats:
				assert rows.value == route['stats_rows'] and 0 < rows.value <= max_rows, (rows.value, route)
				part = sbuf[:rows.value * 2 * Cout].view(rows.value, 2, Cout).cpu()
				assert bool(torch.isfinite(part).all()), ('a statistics row of the reported count was not written', geom)
				assert bool((sbuf[rows.value * 2 * Cout:].view(torch.int64) == -1).all()), ('a statistics row past the reported count was written', geom)
				st = part.sum(dim = 0)
			outs.append((yg.cpu(), st))
		(y, st), (y2, st2) = outs
		assert torch.equal(y.view(torch.int32 if odt == torch.float32 else torch.int16), y2.view(torch.int32 if odt == torch.float32 else torch.int16)), ('two launches differ', geom)
		assert st is None or torch.equal(st, st2)
		return dict(y = y.permute(0, 2, 1), stats = None if st is None else (st[0], st[1]), route = route)
	finally:
		lib.convasr_debug_set_conv_v2(prev)


@functools.lru_cache(maxsize = None)
def _packed(case_name, name, kind, mode):
	"""the packed forward (mode 0) / dgrad (mode 1) copy of a case's integer or random weights"""
	from convasr_amd import ops, _lib
	return ops.pack_weight(_operands(case_name, 'f32' if kind == 'int' else name, kind)['w'].to(dev()), R.DTYPES[name], _lib.PACK_DGRAD if mode else _lib.PACK_FWD)


@functools.lru_cache(maxsize = None)
def _operands(case_name, name, kind):
	c = R.by_name(case_name)
	if kind == 'int':
		return R.integer_operands(c)
	return R.random_operands(c, name, bias_sigmas = R.ONE_TAP_BIAS_SIGMAS if c in R.ONE_TAP else 0.0)


@functools.lru_cache(maxsize = None)
def _reference(case_name, name, kind):
	"""computed once per (case, operand kind; the integer operands are the same in every dtype), shared by the tests, never changed"""
	return R.reference(R.by_name(case_name), _operands(case_name, name, kind))


def _geom(c):
	return (c.B, c.Cin, c.Cout, c.T, R.tout(c), c.K, c.stride, c.dil, c.pad)


def _out_name(c, name):
	return 'f32' if c.out == 'f32' else name


def forward(c, name, kind, bits = None, v2 = None, splits = 0):
	o = _operands(c.name, 'f32' if kind == 'int' else name, kind)
	return launch(name, _out_name(c, name), o['x'], _packed(c.name, name, kind, 0), _geom(c), o, c.epi['act'], c.epi['stats'] and not splits,
	              c.bits if bits is None else bits, (c.v2 if name != 'f32' else 1) if v2 is None else v2, splits)


# ---- the three checks

def first_wrong(got, want, what):
	"""bit-for-bit equality of two logical (B, C, T) float64 tensors, with the first wrong (b, t, co) and the difference in the message"""
	bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
	if bool(bad.any()):
		b, co, t = (int(v) for v in bad.nonzero()[0])
		raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements wrong; first at (b {b}, t {t}, co {co}): got {float(got[b, co, t])!r}, float64 says {float(want[b, co, t])!r}, difference {float(got[b, co, t] - want[b, co, t])!r}')


def check_integers(c, name, got, ref, xlen, what):
	"""(a)"""
	out_name = got['y'].dtype
	assert not bool(torch.isnan(got['y']).any()), (what, 'an element of y was never written, or a guard was read', int(torch.isnan(got['y']).sum()))
	want = ref['y'] if out_name == torch.float32 else R.round16(ref['y'], 'bf16' if out_name == torch.bfloat16 else 'f16')
	first_wrong(got['y'].double(), want, what)
	if xlen is not None:  # frames at or past valid_len: +0 exactly
		dead = ~R.live_mask(xlen, got['y'].shape[2]).expand_as(got['y'])
		bits = got['y'].contiguous().view(torch.int32 if out_name == torch.float32 else torch.int16)
		assert bool(dead.any()) and bool((bits[dead] == 0).all()), (what, 'a masked frame is not +0')
	if got['stats'] is not None:
		s1, s2 = R.stats(ref['raw'])
		assert torch.equal(got['stats'][0], s1) and torch.equal(got['stats'][1], s2), (what, 'statistics', float((got['stats'][0] - s1).abs().max()), float((got['stats'][1] - s2).abs().max()))


def check_random(c, name, got, o, ref, what, splits = 0, chain = None):
	"""(b), and (c) for an fp32 output (chain: the thunk that computes chain32 of the corner)"""
	out_name = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16'}[got['y'].dtype]
	assert not bool(torch.isnan(got['y']).any()), (what, 'an element of y was never written, or a guard was read')
	err, bar = (got['y'].double() - ref['y']).abs(), R.bound(c, name, out_name, o, ref, splits)
	worst = float((err / bar).max())
	print(f'    {what}: worst |got - ref| / bar {worst:.3f}')
	assert bool((err <= bar).all()), (what, worst)
	if got['stats'] is not None:
		(s1, s2), (b1, b2) = R.stats(ref['raw']), R.stats_bound(c, got['route']['route'], ref)
		e1, e2 = (got['stats'][0] - s1).abs(), (got['stats'][1] - s2).abs()
		print(f'    {what}: statistics worst error / bar {float((e1 / b1).max()):.3f} (sum), {float((e2 / b2).max()):.3f} (sum of squares)')
		assert bool((e1 <= b1).all()) and bool((e2 <= b2).all()), (what, float((e1 / b1).max()), float((e2 / b2).max()))
	if out_name == 'f32' and chain is not None:
		assert c.epi['act'] is None or splits, what  # (the corner is compared before any activation clips it; the split-K cases compare the epilogue's value)
		k = min(R.CORNER, got['y'].shape[1])
		want = ref['y'][:, :k]
		e_got, e_chain = float((got['y'][:, :k].double() - want).norm()), float((torch.from_numpy(chain()).double() - want).norm())
		print(f'CONV {what}: ||got - ref||_F {e_got:.3e}  ||chain32 - ref||_F {e_chain:.3e}  ratio {e_got / e_chain:.3f}')
		assert e_got <= FACTOR * e_chain, (what, e_got, e_chain)


def _chain(c, o):
	return lambda: R.chain32(o['x'], o['w'], o['bias'], c.stride, c.dil, c.pad, R.tout(c))


FORWARD = R.LDS_DMA + R.GENERAL + R.ONE_TAP


@pytest.mark.parametrize('c,name', _pairs(FORWARD), ids = _ids(FORWARD))
def test_forward_on_integer_operands_is_exact(c, name):
	o, ref = _operands(c.name, 'f32', 'int'), _reference(c.name, 'f32', 'int')
	got = forward(c, name, 'int')
	assert got['route'] == R.plan_of(c, name) and all(got['route'][k] == v for k, v in c.edges.items()), got['route']
	check_integers(c, name, got, ref, o['xlen'], f'{c.name} {name} forward')


@pytest.mark.parametrize('c,name', _pairs(FORWARD), ids = _ids(FORWARD))
def test_forward_on_random_operands_is_within_the_derived_bound(c, name):
	o, ref = _operands(c.name, name, 'rand'), _reference(c.name, name, 'rand')
	got = forward(c, name, 'rand')
	plain = c.epi['act'] is None and not c.epi['scale'] and c.epi['xlen'] is None
	check_random(c, name, got, o, ref, f'{c.name} {name} forward', chain = _chain(c, o) if plain else None)
	if _out_name(c, name) == 'f32' and not plain:  # (c) before any activation clips the corner: the same launch with the bias alone
		cp, op = c._replace(epi = dict(R.PLAIN, bias = True)), dict(o, scale = None, shift = None, xlen = None)
		got = launch(name, 'f32', o['x'], _packed(c.name, name, 'rand', 0), _geom(c), op, None, False, c.bits, c.v2 if name != 'f32' else 1)
		check_random(cp, name, got, op, R.reference(cp, op), f'{c.name} {name} forward, bias alone', chain = _chain(c, o))


DGRAD = [c for c in FORWARD if R.has_dgrad(c)]


@pytest.mark.parametrize('c,name', _pairs(DGRAD), ids = _ids(DGRAD))
def test_dgrad_is_exact_on_integers_and_within_the_bound_on_random_operands(c, name):
	"""the same kernels on dy: ops.pack_weight(..., PACK_DGRAD), channels swapped, pad' = dil (K - 1) - pad, against the float64 dgrad"""
	d = R.case(c.name + ' as dgrad', (c.B, c.Cout, c.Cin, R.tout(c) + c.trunc, c.K, 1, c.dil), {}, pad = c.dil * (c.K - 1) - c.pad, ints = c.ints)
	geom = (c.B, c.Cout, c.Cin, R.tout(c) + c.trunc, c.T, c.K, 1, c.dil, d.pad)
	assert R.tout(d) == c.T
	v2 = c.v2 if name != 'f32' else 1
	for kind in ('int', 'rand'):
		w = _operands(c.name, 'f32' if kind == 'int' else name, kind)['w']
		dy = R.integer_dy(c) if kind == 'int' else R.random_dy(c, name)
		got = launch(name, _out_name(c, name), dy, _packed(c.name, name, kind, 1), geom, bits = c.bits, v2 = v2)
		assert got['route'] == R.plan_of(c, name, dgrad = True)
		wd = w.flip(2).permute(1, 0, 2).contiguous()  # the dgrad as a forward conv, for absdot and the chain
		ref = dict(raw = R.dgrad(dy, w, c.dil, c.pad, c.T), absdot = R.conv(dy.abs(), wd.abs(), None, 1, c.dil, d.pad, c.T))
		ref['y'] = ref['raw']
		what = f'{c.name} {name} dgrad ({got["route"]["route"]})'
		if kind == 'int':
			check_integers(d, name, got, ref, None, what)
		else:
			check_random(d, name, got, dict(scale = None), ref, what, chain = lambda: R.chain32(dy, wd, None, 1, c.dil, d.pad, c.T))


# ---- launches that must give the same bits

def _same(a, b):
	return torch.equal(a['y'].contiguous().view(torch.int16), b['y'].contiguous().view(torch.int16))


@pytest.mark.parametrize('name', R.HALVES)
def test_tile_shapes_of_the_lds_dma_kernel_give_the_same_bits(name):
	"""the 128-row tail tile against a padded 256-row one; a flattened K = 1 batch against per-utterance tiles; quarter tiles against halves
	and against full tiles -- on random operands, where a different k order would show"""
	for a, b in R.SAME_BITS:
		ga, gb = forward(R.by_name(a), name, 'rand'), forward(R.by_name(b), name, 'rand')
		assert ga['route'] != gb['route'] and _same(ga, gb), (a, b)
	q = R.by_name('quarters')
	g0 = forward(q, name, 'rand')
	for bits in R.QUARTERS_BITS:
		g = forward(q, name, 'rand', bits = bits)
		assert g['route'] != g0['route'] and g['route'] == R.plan_of(q, name, bits = bits) and _same(g0, g), bits


@pytest.mark.parametrize('c,name', _pairs(R.ONE_TAP), ids = _ids(R.ONE_TAP))
def test_one_tap_kernel_stage_forms_and_the_lds_dma_kernel_give_the_same_bits(c, name):
	o, ref = _operands(c.name, name, 'rand'), _reference(c.name, name, 'rand')
	g0 = forward(c, name, 'rand')
	flipped = forward(c, name, 'rand', bits = c.bits | R.FLIP_STAGES)
	assert flipped['route']['stages'] == 3 - g0['route']['stages'] and _same(g0, flipped) and torch.equal(g0['stats'][0], flipped['stats'][0]) and torch.equal(g0['stats'][1], flipped['stats'][1])
	v2s = forward(c, name, 'rand', bits = c.bits | R.NO_1X1)
	assert v2s['route']['route'] == 'lds_dma' and _same(g0, v2s)
	check_random(c, name, v2s, o, ref, f'{c.name} {name} forward, the LDS-DMA kernel on the same data')  # (its statistics: within the chain bound)


# ---- split-K

@pytest.mark.parametrize('c,name', _pairs(R.SPLITK), ids = _ids(R.SPLITK))
def test_split_k_launches_with_a_short_last_split(c, name):
	from convasr_amd import _lib
	splits, cps = R.splitk_plan(name, c.B, c.Cin, c.Cout, R.tout(c))
	assert dict(splits = splits, cps = cps, last = (c.Cin // 64 if name in R.HALVES else -(-c.Cin // 32)) - (splits - 1) * cps) == c.edges
	assert _lib.load().convasr_conv1d_fwd_splitk_plan(_lib.dtype_code(R.DTYPES[name]), c.B, c.Cin, c.Cout, R.tout(c), c.K, None) == splits
	for out in (('f32', ) if name == 'f32' else ('f32', 'same')):
		cc = c._replace(out = out)
		o, ref = _operands(c.name, 'f32', 'int'), _reference(c.name, 'f32', 'int')
		check_integers(cc, name, forward(cc, name, 'int', splits = splits), ref, o['xlen'], f'{c.name} {name} -> {out}, {splits} splits')
		o, ref = _operands(c.name, name, 'rand'), _reference(c.name, name, 'rand')
		plain = cc._replace(epi = dict(R.PLAIN, bias = True))  # (c) before any activation clips the corner: bias alone
		if out == 'f32':
			op = dict(o, scale = None, shift = None, xlen = None)
			check_random(plain, name, launch(name, 'f32', o['x'], _packed(c.name, name, 'rand', 0), _geom(c), op, None, False, c.bits, 1, splits), op, R.reference(plain, op), f'{c.name} {name} -> f32, {splits} splits, bias alone', splits, _chain(c, o))
		check_random(cc, name, forward(cc, name, 'rand', splits = splits), o, ref, f'{c.name} {name} -> {out}, {splits} splits', splits)


def test_split_k_request_outside_the_lds_dma_envelope_is_served_by_the_unsplit_launch():
	"""(1, 128, 128, 300, K 23, dil 3) in bf16: the plan splits it (it sees neither K's halo nor the dilation), the LDS-DMA kernel refuses the
	256-row tile a split launch forces ((K - 1) dil = 66 > 64), and ops.conv1d(..., splitk = True) raised CONVASR_EUNSUPPORTED for a request
	the unsplit call serves.  It must return the unsplit call's values -- and the float64 ones."""
	from convasr_amd import ops, _lib
	c = R.SPLITK_FALLBACK
	name = 'bf16'
	dt = R.DTYPES[name]
	o, ref = _operands(c.name, name, 'rand'), _reference(c.name, name, 'rand')
	splits, _ = R.splitk_plan(name, c.B, c.Cin, c.Cout, R.tout(c))
	assert splits >= 2 and R.plan_of(c, name, bits = R.NO_SHORT)['route'] == 'general' and R.plan_of(c, name)['route'] == 'lds_dma'
	d = dev()
	x, wp = ops.as_cl(o['x'].to(d), dt), _packed(c.name, name, 'rand', 0)
	kw = dict(bias = o['bias'].to(d), scale = o['scale'].to(d), shift = o['shift'].to(d), act = _act(c.epi['act']), xlen = o['xlen'].to(d))
	for out_dt in (dt, torch.float32):
		a = ops.conv1d(x, wp, c.Cout, c.K, 1, c.dil, c.pad, out_dtype = out_dt, splitk = True, **kw)
		b = ops.conv1d(x, wp, c.Cout, c.K, 1, c.dil, c.pad, out_dtype = out_dt, **kw)
		assert a.dtype == out_dt and torch.equal(a, b)
		got = dict(y = a.cpu(), stats = None)
		check_random(c, name, got, o, ref, f'{c.name} {name} -> {out_dt}')
	# under the protocol, through the entry point itself
	check_random(c, name, forward(c, name, 'rand', splits = splits), o, ref, f'{c.name} {name}, convasr_conv1d_fwd_splitk')
	check_integers(c, name, forward(c, name, 'int', splits = splits), _reference(c.name, 'f32', 'int'), _operands(c.name, 'f32', 'int')['xlen'], f'{c.name} {name}, integers')


# ---- the refusal leaves the output alone

@pytest.mark.parametrize('name', R.ALL)
def test_refused_launch_touches_nothing(name):
	from convasr_amd import _lib
	lib = _lib.load()
	c = R.REFUSED
	dt = R.DTYPES[name]
	_, xg = _guarded(torch.zeros(c.B, c.T, c.Cin), dt, float('nan'))
	_, wg = _guarded(torch.zeros(c.K, 128, c.Cin), dt, float('nan'))
	ybuf, yg = _guarded((c.B, R.tout(c), c.Cout), dt, SENTINEL)
	prev = lib.convasr_debug_set_conv_v2(0)
	try:
		p = lambda t: ctypes.c_void_p(t.data_ptr())
		rc = lib.convasr_conv1d_fwd(p(xg), p(wg), p(yg), _lib.dtype_code(dt), _lib.dtype_code(dt), c.B, c.Cin, c.Cout, c.T, R.tout(c), c.K, c.stride, c.dil, c.pad, None, None, None, None, 0, 0.0, 0.0, None, None, _lib.stream_ptr())
	finally:
		lib.convasr_debug_set_conv_v2(prev)
	torch.cuda.synchronize()
	assert rc == R.EUNSUPPORTED and b'halo too large' in lib.convasr_last_error()
	assert bool(torch.isnan(yg).all()) and _guards_intact(ybuf, yg.numel())


# ---- the grouped one-tap launch

@pytest.mark.parametrize('name', R.HALVES)
def test_grouped_one_tap_launch_with_both_stage_classes_and_accumulation(name):
	"""four problems over 3 x 100 frames, one- and two-stage ones in one call; a plain launch with biases and statistics (integers: bit for
	bit), and an accumulating one into a random 16-bit start: round16(round16(sum + bias) + start), what conv1x1_tile computes"""
	from convasr_amd import ops, _lib
	B, T = R.GROUPED_FRAMES
	dt, d = R.DTYPES[name], dev()
	assert {ci >= 3 * co for ci, co in R.GROUPED} == {True, False}
	g = torch.Generator().manual_seed(11)
	for kind in ('int', 'rand'):
		xs, ws, bs, cases = [], [], [], []
		for i, (ci, co) in enumerate(R.GROUPED):
			c = R.case(f'grouped {i}', (B, ci, co, T, 1, 1, 1), {}, epi = R.BIAS_STATS, ints = R.SMALL)
			o = R.integer_operands(c, seed = i) if kind == 'int' else R.random_operands(c, name, seed = i, bias_sigmas = R.ONE_TAP_BIAS_SIGMAS)
			cases.append((c, o, R.reference(c, o)))
		xg = [ops.as_cl(o['x'].to(d), dt) for _, o, _ in cases]
		wp = [ops.pack_weight(o['w'].to(d), dt, _lib.PACK_FWD) for _, o, _ in cases]
		bias = [o['bias'].to(d) for _, o, _ in cases]
		couts = [co for _, co in R.GROUPED]
		# plain, with statistics
		sts = [ops.ConvStats(co, B, T, d) for co in couts]
		for s in sts:
			s.buf.view(torch.int64).fill_(-1)
		outs = [ops.empty_cl(B, co, T, dt, d) for co in couts]
		for y in outs:
			y.fill_(float('nan'))
		ys = ops.conv1x1_grouped(xg, wp, couts, biases = bias, stats = sts, outs = outs)
		assert ys is not None
		for (c, o, ref), y, s in zip(cases, ys, sts):
			assert s.rows == -(-B * T // 128)
			part = s.buf[:s.rows * 2 * c.Cout].view(s.rows, 2, c.Cout).cpu().sum(dim = 0)
			got = dict(y = y.cpu(), stats = (part[0], part[1]), route = dict(route = 'one_tap'))
			if kind == 'int':
				check_integers(c, name, got, ref, None, f'{c.name} {name}')
			else:
				check_random(c, name, got, o, ref, f'{c.name} {name}')
		# accumulating into a random 16-bit start
		starts = [torch.randn(B, co, T, generator = g).mul(4).round().to(dt) if kind == 'int' else torch.randn(B, co, T, generator = g).to(dt) for co in couts]
		outs = [ops.as_cl(s.to(d), dt) for s in starts]
		assert all(ops.is_cl(y) for y in outs)
		ys = ops.conv1x1_grouped(xg, wp, couts, biases = bias, outs = outs, accumulate = R.GROUPED_ACCUMULATE)
		for (c, o, ref), y, start, acc in zip(cases, ys, starts, R.GROUPED_ACCUMULATE):
			if kind == 'int':
				want = R.round16(R.round16(ref['y'], name) + start.double(), name) if acc else R.round16(ref['y'], name)
				first_wrong(y.cpu().double(), want, f'{c.name} {name} accumulate {acc}')
			else:  # the first rounding may fall either way within the bar, the second adds its own
				bar = R.bound(c, name, name, o, ref)
				lo, hi = ref['y'] - bar, ref['y'] + bar
				if acc:
					lo, hi = lo + start.double(), hi + start.double()
					slack = R.U16[name] * torch.maximum(lo.abs(), hi.abs()) + 0.5 * R.SUB16[name]
					lo, hi = lo - slack, hi + slack
				v = y.cpu().double()
				assert bool(((v >= lo) & (v <= hi)).all()), (c.name, name, acc)


# ---- the packers

def _pack_want(w, name):
	"""packed_fwd[k][co][ci] = w[co][ci][k], packed_dgrad[k][ci][co] = w[co][ci][K - 1 - k], rounded to the storage type; padded rows untouched (zero)"""
	Cout, Cin, K = w.shape
	r = R.round16(w, name) if name != 'f32' else w.double()
	fwd, dgr = torch.zeros(K, -(-Cout // 128) * 128, Cin, dtype = torch.float64), torch.zeros(K, -(-Cin // 128) * 128, Cout, dtype = torch.float64)
	fwd[:, :Cout] = r.permute(2, 0, 1)
	dgr[:, :Cin] = r.flip(2).permute(2, 1, 0)
	return fwd, dgr


@pytest.mark.parametrize('name', R.ALL)
def test_weight_packers_bit_for_bit(name):
	from convasr_amd import ops, _lib
	dt, d = R.DTYPES[name], dev()
	g = torch.Generator().manual_seed(2)
	for shape in R.PACK[:2 if name == 'f32' else 3]:
		w = torch.randn(*shape, generator = g)
		wf, wd = _pack_want(w, name)
		fwd, dgr = ops.pack_weight(w.to(d), dt)
		assert torch.equal(fwd.cpu().double(), wf) and torch.equal(dgr.cpu().double(), wd), shape
		# a K-major source: the same logical parameter in the training arena's memory order
		Cout, Cin, K = shape
		wk = w.permute(2, 0, 1).contiguous().to(d).permute(1, 2, 0)
		assert ops.weight_layout(wk) == _lib.W_KMAJOR
		if Cout * Cin % 8:  # the K-major packer's contract (Cout Cin % 8 == 0): refused before any launch
			with pytest.raises(_lib.ConvasrHipError, match = 'K-major source needs'):
				ops.pack_weight(wk, dt)
			continue
		fwd, dgr = ops.pack_weight(wk, dt)
		assert torch.equal(fwd.cpu().double(), wf) and torch.equal(dgr.cpu().double(), wd), (shape, 'K-major')


@pytest.mark.parametrize('name', R.HALVES)
def test_grouped_dgrad_packer_bit_for_bit(name):
	"""convasr_pack_dgrad_grouped over three items (its contract: even channel counts, so (38, 40, 3) stands for the scalar kernels' shape)"""
	import struct
	from convasr_amd import ops, _lib
	dt, d = R.DTYPES[name], dev()
	g = torch.Generator().manual_seed(4)
	shapes = [(38, 40, 3)] + R.PACK[1:]
	assert _lib.load().convasr_pack_dgrad_item_bytes() == 40
	blob, first, items = b'', 0, []
	for Cout, Cin, K in shapes:
		w = torch.randn(Cout, Cin, K, generator = g)
		fwd = ops.pack_weight(w.to(d), dt, _lib.PACK_FWD)
		dbuf, dgr = _guarded(torch.zeros(K, ops.cout_pad(Cin), Cout), dt, SENTINEL)
		blob += struct.pack('<QQiiiiii', fwd.data_ptr(), dgr.data_ptr(), Cout, Cin, K, ops.cout_pad(Cout), ops.cout_pad(Cin), first)
		first += K * ((Cout + 63) // 64) * ((Cin + 63) // 64)
		items.append((w, fwd, dbuf, dgr))
	table = torch.frombuffer(bytearray(blob), dtype = torch.uint8).to(d)
	_lib.call('convasr_pack_dgrad_grouped', _lib.ptr(table), len(items), first, _lib.stream_ptr())
	torch.cuda.synchronize()
	for w, fwd, dbuf, dgr in items:
		assert torch.equal(dgr.cpu().double(), _pack_want(w, name)[1]) and _guards_intact(dbuf, dgr.numel()), tuple(w.shape)
