"""Float64 restatement of the forward conv and its input gradient, the yardsticks the GPU tests hold the kernels to, a Python restatement of
the dispatcher, and the case tables.

Plain torch / numpy on the CPU; the library is not imported here.  tests/test_conv_ref.py holds this file to float64 F.conv1d and autograd,
holds the planner to the library's own route query (convasr_conv1d_fwd_route) for every case, and holds every case to the edge it claims;
tests/test_conv_routes_gpu.py runs the tables on the MI355X.

Tensors are the logical (B, C, T) ones; the kernels' channels-last memory is the GPU file's business.  A case gives its shape as
(B, Cin, Cout, T, K, stride, dil) with T the INPUT length; pad = dil (K - 1) / 2 unless stated, Tout = what the geometry yields less `trunc`."""
import collections

import numpy as np
import torch

U32 = 2.0 ** -24    # unit roundoff of fp32
TINY = 2.0 ** -126  # smallest normal fp32
CORNER = 32         # chain32 carries the first CORNER output channels
U16 = dict(bf16 = 2.0 ** -8, f16 = 2.0 ** -11)           # unit roundoff of the storage types
SUB16 = dict(bf16 = 2.0 ** -133, f16 = 2.0 ** -24)       # their subnormal spacing

DTYPES = dict(f32 = torch.float32, bf16 = torch.bfloat16, f16 = torch.float16)
HALVES = ('bf16', 'f16')
ALL = ('f32', 'bf16', 'f16')

# ConvParams::debug bits the dispatchers read (csrc/conv_v2s.hip, csrc/conv1x1.hip, csrc/conv.hip)
NO_QUARTERS, NO_NARROW, NO_TAIL, NO_FLATTEN, NO_SHORT, NO_1X1, FLIP_STAGES = 16, 32, 128, 512, 2048, 8192, 16384

# chain lengths of the statistics: the addends of one fp32 chain before the sums are carried in fp64.  csrc/conv.hip's epilogue adds 2 x 16
# values per lane and one cross-lane term (33); csrc/conv_v2s.hip's at most 4 x 4 and two (18) -- both as
# test_conv1d_epilogue_stats_of_channels_far_from_zero_mean states them; csrc/conv1x1.hip's conv1x1_tile adds MI x 4 = 16 values per lane
# (s1 += val over mi, g) and two __shfl_xor terms (18), the two wave halves then meet in fp64.
STATS_L = dict(general = 33, lds_dma = 18, one_tap = 18)


def out_len(Tin, K, stride, dil, pad):
	return (Tin + 2 * pad - dil * (K - 1) - 1) // stride + 1


def _tap_range(k, Tin, Tout, stride, dil, pad):
	"""output frames [t0, t1) whose tap k reads inside [0, Tin), and the first input frame read"""
	off = k * dil - pad
	t0 = max(0, -(off // stride)) if off < 0 else 0
	t1 = min(Tout, (Tin - 1 - off) // stride + 1) if Tin - 1 - off >= 0 else 0
	return t0, max(t1, t0), t0 * stride + off


def conv(x, w, bias, stride, dil, pad, Tout):
	"""y[b, co, t] = sum_k sum_ci w[co, ci, k] x[b, ci, t stride + k dil - pad] (+ bias[co]), terms outside [0, Tin) dropped, the first Tout
	frames: float64 (B, Cout, Tout), tap after tap."""
	x, w = x.double(), w.double()
	(B, Cin, Tin), (Cout, _, K) = x.shape, w.shape
	y = torch.zeros(B, Cout, Tout, dtype = torch.float64)
	for k in range(K):
		t0, t1, i0 = _tap_range(k, Tin, Tout, stride, dil, pad)
		if t1 > t0:
			y[:, :, t0:t1] += torch.einsum('oc,bct->bot', w[:, :, k], x[:, :, i0:i0 + (t1 - t0 - 1) * stride + 1:stride])
	return y if bias is None else y + bias.double().view(1, -1, 1)


def dgrad(dy, w, dil, pad, Tin = None):
	"""dx[b, ci, t + k dil - pad] += sum_co w[co, ci, k] dy[b, co, t] (stride 1), frames outside [0, Tin) dropped: float64 (B, Cin, Tin)"""
	dy, w = dy.double(), w.double()
	(B, Cout, Tout), (_, Cin, K) = dy.shape, w.shape
	Tin = Tout + dil * (K - 1) - 2 * pad if Tin is None else Tin
	dx = torch.zeros(B, Cin, Tin, dtype = torch.float64)
	for k in range(K):
		off = k * dil - pad
		t0, t1 = max(0, -off), min(Tout, Tin - off)
		if t1 > t0:
			dx[:, :, t0 + off:t1 + off] += torch.einsum('oc,bot->bct', w[:, :, k], dy[:, :, t0:t1])
	return dx


def valid_len(xlen, Tout):
	"""ceil(xlen * Tout) in fp32, as csrc/common.h valid_len computes it; (B,) int64"""
	return torch.ceil(xlen.float() * torch.tensor(float(Tout), dtype = torch.float32)).long()


def activation(v, act):
	"""act: None, 'relu' or ('hardtanh', lo, hi)"""
	if act is None:
		return v
	if act == 'relu':
		return v.clamp(min = 0.0)
	return v.clamp(min = act[1], max = act[2])


def epilogue(raw, scale, shift, act, xlen):
	"""raw (bias included) -> (* scale + shift) -> activation -> frames at or past valid_len zeroed: float64"""
	v = raw.double()
	if scale is not None:
		v = v * scale.double().view(1, -1, 1) + shift.double().view(1, -1, 1)
	v = activation(v, act)
	if xlen is not None:
		v = torch.where(live_mask(xlen, v.shape[2]), v, torch.zeros((), dtype = torch.float64))  # (+0 exactly)
	return v


def live_mask(xlen, Tout):
	"""(B, 1, Tout) bool: frame t of utterance b is before valid_len"""
	return torch.arange(Tout).view(1, 1, -1) < valid_len(xlen, Tout).view(-1, 1, 1)


def stats(raw):
	"""(sum, sum of squares) over (b, t) of the value BEFORE scale, activation, mask and storage rounding: float64 (Cout,) each"""
	raw = raw.double()
	return raw.sum(dim = (0, 2)), (raw * raw).sum(dim = (0, 2))


def absdot(x, w, bias, stride, dil, pad, Tout):
	"""conv(|x|, |w|) + |bias|"""
	return conv(x.abs(), w.abs(), None if bias is None else bias.abs(), stride, dil, pad, Tout)


def chain32(x, w, bias, stride, dil, pad, Tout, corner = CORNER):
	"""The first `corner` output channels of the same sum carried in ONE fp32 accumulator per output element, running over (ci, tap) in
	order, the bias added last: the least accurate order a plain fp32 kernel could use.  Each product is rounded to fp32 first (exact
	already when the operands are 16-bit values).  float32 (B, co, Tout) numpy array."""
	xn, wn = x.float().numpy(), w.float().numpy()
	(B, Cin, Tin), (Cout, _, K) = xn.shape, wn.shape
	co = min(corner, Cout)
	hi = max(0, (Tout - 1) * stride + (K - 1) * dil - pad - (Tin - 1))
	xp = np.zeros((B, Cin, pad + Tin + hi), dtype = np.float32)  # zero frames outside [0, Tin): adding 0.0 leaves an accumulator as it is
	xp[:, :, pad:pad + Tin] = xn
	acc = np.zeros((B, co, Tout), dtype = np.float32)
	span = (Tout - 1) * stride + 1
	for ci in range(Cin):
		for k in range(K):
			acc += wn[:co, ci, k][None, :, None] * xp[:, ci, k * dil:k * dil + span:stride][:, None, :]
	if bias is not None:
		acc += bias.float().numpy()[None, :co, None]
	assert acc.dtype == np.float32
	return acc


def round16(v, name):
	"""float64 -> the nearest value of the storage type (ties to even, subnormals, overflow to infinity), as float64"""
	p, smin, big = (8, -133, 2.0 ** 128 * (1 - 2.0 ** -9)) if name == 'bf16' else (11, -24, 65520.0)
	a = np.asarray(v.double().numpy() if isinstance(v, torch.Tensor) else v, dtype = np.float64)
	_, e = np.frexp(a)
	s = np.maximum(e - p, smin)
	q = np.ldexp(np.rint(np.ldexp(a, -s)), s)
	q = np.where(np.abs(a) >= big, np.copysign(np.inf, a), q)
	return torch.from_numpy(q)


# ---- operands

Case = collections.namedtuple('Case', 'name B Cin Cout T K stride dil pad trunc bits v2 epi out dtypes ints splitk edges')
PLAIN = dict(bias = False, scale = False, act = None, xlen = None, stats = False)
FULL = dict(bias = True, scale = True, act = ('hardtanh', 0.0, 20.0), xlen = (0.7, 1.0, 0.35), stats = True)
BIAS_STATS = dict(bias = True, scale = False, act = None, xlen = None, stats = True)


def case(name, shape, edges, bits = 0, v2 = 1, epi = None, out = 'same', dtypes = HALVES, pad = None, trunc = 0, ints = (-1, 6, -3, 3), splitk = False):
	"""shape = (B, Cin, Cout, T, K, stride, dil); bits: the debug bits the case runs under; v2: bit 0 of convasr_debug_set_conv_v2; epi: which
	epilogue operands the launch is given (keys of PLAIN); out: 'same' or 'f32'; ints: (x lo, x hi, w lo, w hi) of the integer operands, inclusive;
	edges: what the route record must show"""
	B, Cin, Cout, T, K, stride, dil = shape
	return Case(name, B, Cin, Cout, T, K, stride, dil, dil * (K - 1) // 2 if pad is None else pad, trunc, bits, v2, dict(PLAIN, **(epi or {})), out, tuple(dtypes), ints, splitk, edges)


def tout(c):
	return out_len(c.T, c.K, c.stride, c.dil, c.pad) - c.trunc


def _xlen(c):
	return None if c.epi['xlen'] is None else torch.tensor([c.epi['xlen'][b % len(c.epi['xlen'])] for b in range(c.B)])


def integer_operands(c, seed = 0):
	"""dict(x, w, bias, scale, shift, xlen) of small integers (exact in bf16, f16 and fp32; x deliberately not centred, so partial sums grow past
	every short format), ranges per case (c.ints) so that every partial sum stays below 2^24 and every 16-bit result below 60000
	(tests/test_conv_ref.py asserts both from the reference).  The epilogue stays exact: integer bias and shift, scale a power of two."""
	g = torch.Generator().manual_seed(1000 + seed)
	xl, xh, wl, wh = c.ints
	x = torch.randint(xl, xh + 1, (c.B, c.Cin, c.T), generator = g).float()
	w = torch.randint(wl, wh + 1, (c.Cout, c.Cin, c.K), generator = g).float()
	bias = torch.randint(-4, 5, (c.Cout, ), generator = g).float() if c.epi['bias'] else None
	scale = (2.0 ** torch.randint(-3, 1, (c.Cout, ), generator = g).float()) if c.epi['scale'] else None
	shift = torch.randint(-2, 9, (c.Cout, ), generator = g).float() if c.epi['scale'] else None
	return dict(x = x, w = w, bias = bias, scale = scale, shift = shift, xlen = _xlen(c))


def integer_dy(c, seed = 0):
	"""the output gradient of a case run as a dgrad: integers of the range of x, the frames the conv was not asked for zero"""
	dy = torch.randint(c.ints[0], c.ints[1] + 1, (c.B, c.Cout, tout(c) + c.trunc), generator = torch.Generator().manual_seed(3000 + seed)).float()
	dy[:, :, tout(c):] = 0
	return dy


def random_dy(c, name, seed = 0):
	dy = torch.randn(c.B, c.Cout, tout(c) + c.trunc, generator = torch.Generator().manual_seed(4000 + seed)).to(DTYPES[name]).float()
	dy[:, :, tout(c):] = 0
	return dy


def random_operands(c, name, seed = 0, bias_sigmas = 0.0):
	"""the same of randn values already rounded to the storage type (x, w; bias, scale and shift are fp32 operands of the kernels);
	bias_sigmas: the bias is that many standard deviations of the output (the statistics far from a zero mean)"""
	g = torch.Generator().manual_seed(2000 + seed)
	dt = DTYPES[name]
	x = torch.randn(c.B, c.Cin, c.T, generator = g).to(dt).float()
	w = (torch.randn(c.Cout, c.Cin, c.K, generator = g) / (c.Cin * c.K) ** 0.5).to(dt).float()
	bias = (torch.randn(c.Cout, generator = g) + bias_sigmas) if c.epi['bias'] else None
	scale = (torch.rand(c.Cout, generator = g) + 0.5) * (1 - 2 * (torch.arange(c.Cout) % 5 == 0).float()) if c.epi['scale'] else None
	shift = torch.randn(c.Cout, generator = g) + 1.0 if c.epi['scale'] else None
	return dict(x = x, w = w, bias = bias, scale = scale, shift = shift, xlen = _xlen(c))


def reference(c, ops_):
	"""dict(raw, y, absdot) in float64 for a case's operands: raw = conv + bias, y = the epilogue of it"""
	To = tout(c)
	raw = conv(ops_['x'], ops_['w'], ops_['bias'], c.stride, c.dil, c.pad, To)
	return dict(raw = raw, y = epilogue(raw, ops_['scale'], ops_['shift'], c.epi['act'], ops_['xlen']), absdot = absdot(ops_['x'], ops_['w'], ops_['bias'], c.stride, c.dil, c.pad, To))


def bound(c, name, out_name, ops_, ref, splits = 0):
	"""Check (b)'s element-wise bar, derived: before the epilogue |got - ref| <= e = 2 n u absdot + 2^-126 with n = Cin K + 1 + splits (the
	products of 16-bit operands are exact in fp32; fp32 operands add one rounding each, inside the factor 2); through the scale: e |scale| +
	2 u (|scale v| + |shift|); a non-expansive activation carries it unchanged; 16-bit storage adds u16 (|ref| + e) + half the subnormal spacing."""
	n = c.Cin * c.K + 1 + splits
	e = 2 * n * U32 * ref['absdot'] + TINY
	if ops_['scale'] is not None:
		sc, sh = ops_['scale'].double().view(1, -1, 1), ops_['shift'].double().view(1, -1, 1)
		e = e * sc.abs() + 2 * U32 * ((sc * ref['raw']).abs() + sh.abs())
	if out_name != 'f32':
		e = e + U16[out_name] * (ref['y'].abs() + e) + 0.5 * SUB16[out_name]
	return e


def stats_bound(c, route, ref):
	"""the same for the statistics (sum, sum of squares over (b, t) of raw): every element's own error e summed, plus the fp32 chains of L
	addends (STATS_L) that carry them: 2 L u sum |raw| and, with one more rounding for the square, 2 (L + 1) u sum raw^2."""
	n, L = c.Cin * c.K + 1, STATS_L[route]
	e = 2 * n * U32 * ref['absdot'] + TINY
	a = ref['raw'].abs()
	return e.sum(dim = (0, 2)) + 2 * L * U32 * a.sum(dim = (0, 2)), (2 * a * e + e * e).sum(dim = (0, 2)) + 2 * (L + 1) * U32 * (a * a).sum(dim = (0, 2))


# ---- the planner: csrc/conv.hip conv1d_route, csrc/conv1x1.hip convasr_conv1x1_plan, csrc/conv_v2s.hip convasr_conv1d_v2_plan restated

EINVAL, EUNSUPPORTED = -1, -3
FIELDS = ('error', 'B', 'T', 'tile_rows', 'm_tiles_per_b', 'n_tiles', 'total_tiles', 'full_tiles', 'narrow_parts', 'tail128', 'x_rows', 'xi', 'aligned_x', 'stages', 'lds_bytes', 'stats_rows')


def plan(xd, yd, B, Cin, Cout, Tin, Tout, K, stride, dil, pad, scale = False, act = False, xlen = False, stats = False, v2 = 1, bits = 0, n_cu = 256):
	"""what convasr_conv1d_fwd_route answers (ops.conv_route's dict) for dtype names xd -> yd on a chip of n_cu compute units"""
	refused = lambda code: dict(route = 'refused', error = code)
	half = xd in HALVES
	if min(B, Cin, Cout, Tin, Tout, K, stride, dil) <= 0 or Tout > out_len(Tin, K, stride, dil, pad):
		return refused(EINVAL)
	if K == 1 and stride == 1 and pad == 0 and Tin == Tout and B > 1 and not xlen and not bits & NO_FLATTEN and B * Tin * max(Cin, Cout) * 4 < 2 ** 31:
		Tin = Tout = B * Tin
		B = 1
	cout_pad = -(-Cout // 128) * 128
	n_tiles = cout_pad // 128
	osz = 4 if yd == 'f32' else 2
	r = dict.fromkeys(FIELDS, 0)
	r.update(B = B, T = Tout, n_tiles = n_tiles)
	x_rows = ((127 * stride + (K - 1) * dil + 1) + 1) & ~1
	smem = max(2 * x_rows * 128 + 2 * 128 * 128, 128 * (128 * osz + 16) + 4 * 128 * 4)
	if smem > 160 * 1024:
		return refused(EINVAL)
	small = lambda *n: all(v < 2 ** 31 for v in n)
	if half and v2:
		M = B * Tout
		if (K == 1 and stride == 1 and pad == 0 and Tin == Tout and Cin % 64 == 0 and Cout % 128 == 0 and yd == xd and not scale and not act and not xlen
		    and not bits & NO_1X1 and small(M * Cin * 2, M * Cout * 2, cout_pad * Cin * 2)):
			m_tiles = -(-M // 128)
			one_stage = (Cin < 3 * Cout) != bool(bits & FLIP_STAGES)
			r.update(route = 'one_tap', tile_rows = 128, m_tiles_per_b = m_tiles, total_tiles = m_tiles * n_tiles, full_tiles = m_tiles * n_tiles, stages = 1 if one_stage else 2,
			         lds_bytes = max(128 * (128 * 2 + 16) + 4 * 128 * 4, 2 * 128 * 128) if one_stage else 4 * 128 * 128, stats_rows = m_tiles if stats else 0)
			return r
		if stride == 1 and Cin % 64 == 0 and yd in (xd, 'f32'):
			bm = 256
			all_short = not bits & NO_SHORT and B * -(-Tout // 256) * n_tiles * 4 <= n_cu
			if all_short:
				bm = 128
			xr = (bm + (K - 1) * dil + 15) & ~15
			lds = 3 * xr * 128 + 3 * 16384 if K == 1 else 2 * xr * 128 + 5 * 16384
			lds = max(lds, bm * (128 * osz + 16) + 8 * 128 * 4)
			if lds <= 160 * 1024 and small(Tin * Cin * 2, K * cout_pad * Cin * 2, (Tout + bm) * Cout * 2):
				mt = -(-Tout // bm)
				total = B * mt * n_tiles
				tail_rows = Tout - (mt - 1) * bm
				full, parts = total, 2
				if not bits & NO_NARROW:
					rest = total % n_cu
					if rest > 0 and 2 * rest <= n_cu and (total - rest) % 8 == 0:
						full = total - rest
						if full > 0 and 4 * rest <= n_cu and not bits & NO_QUARTERS:
							parts = 4
				r.update(route = 'lds_dma', tile_rows = bm, m_tiles_per_b = mt, total_tiles = total, full_tiles = full, narrow_parts = parts, x_rows = xr, lds_bytes = lds,
				         tail128 = 2 if all_short else int(tail_rows <= 128 and not bits & NO_TAIL), stats_rows = B * mt if stats else 0)
				return r
	if not ((xd == 'f32' and yd == 'f32') or (half and yd in (xd, 'f32'))):
		return refused(EUNSUPPORTED)
	xi = -(-x_rows * 8 // 256)
	aligned = Cin * (2 if half else 4) % 16 == 0
	if xi > (16 if aligned else 9):
		return refused(EUNSUPPORTED)
	mt = -(-Tout // 128)
	r.update(route = 'general', tile_rows = 128, m_tiles_per_b = mt, total_tiles = B * mt * n_tiles, full_tiles = B * mt * n_tiles, x_rows = x_rows, lds_bytes = smem,
	         xi = 9 if not aligned else (5 if xi <= 5 else 9 if xi <= 9 else 16), aligned_x = int(aligned), stats_rows = B * mt if stats else 0)
	return r


def plan_of(c, name, **over):
	"""the planner's answer for a case in one dtype; over: v2 / bits / n_cu, or dgrad = True for the case run as an input gradient"""
	yd = 'f32' if c.out == 'f32' or name == 'f32' else name
	kw = dict(v2 = c.v2 if name != 'f32' else 1, bits = c.bits)
	dg = over.pop('dgrad', False)
	kw.update(over)
	if dg:  # the same kernels on dy: channels swapped, stride 1, pad' = dil (K - 1) - pad, no epilogue
		return plan(name, yd, c.B, c.Cout, c.Cin, tout(c) + c.trunc, c.T, c.K, 1, c.dil, c.dil * (c.K - 1) - c.pad, **kw)
	e = c.epi
	return plan(name, yd, c.B, c.Cin, c.Cout, c.T, tout(c), c.K, c.stride, c.dil, c.pad, scale = e['scale'], act = e['act'] is not None, xlen = e['xlen'] is not None, stats = e['stats'], **kw)


def splitk_plan(name, B, Cin, Cout, Tout, n_cu = 256):
	"""(splits, input blocks per split) of csrc/conv.hip splitk_plan; splits 1 = not split"""
	half = name in HALVES
	n_cib = Cin // 64 if half else -(-Cin // 32)
	tiles = B * -(-Tout // (256 if half else 128)) * (-(-Cout // 128))
	if (half and Cin % 64) or n_cib < 2 or tiles * 4 > n_cu or Cout % 8:
		return 1, 0
	cps = -(-n_cib // min(n_cu // tiles, n_cib, 32))
	return -(-n_cib // cps), cps


# ---- case tables (256 compute units)

_lds = lambda **e: dict(route = 'lds_dma', **e)
_gen = lambda **e: dict(route = 'general', **e)
_tap = lambda **e: dict(route = 'one_tap', **e)
SMALL = (-1, 3, -2, 2)  # operand range of the cases with statistics: every (tile, column) sum of squares stays below 2^24

LDS_DMA = [
	case('tile256_nb4_plain', (1, 64, 128, 256, 3, 1, 1), _lds(tile_rows = 256, total_tiles = 1, full_tiles = 1, tail128 = 0), NO_SHORT | NO_NARROW),
	case('tile256_tail128_ragged_cout', (2, 128, 136, 300, 11, 1, 1), _lds(tile_rows = 256, m_tiles_per_b = 2, n_tiles = 2, total_tiles = 8, full_tiles = 8, tail128 = 1, stats_rows = 4), NO_SHORT | NO_NARROW, epi = FULL, ints = SMALL),
	case('tail_off_same_bits', (2, 128, 136, 300, 11, 1, 1), _lds(tile_rows = 256, m_tiles_per_b = 2, total_tiles = 8, full_tiles = 8, tail128 = 0), NO_SHORT | NO_NARROW | NO_TAIL, epi = FULL, ints = SMALL),
	case('tail_128', (1, 64, 128, 384, 5, 1, 1), _lds(tile_rows = 256, m_tiles_per_b = 2, full_tiles = 2, tail128 = 1), NO_SHORT | NO_NARROW),
	case('tail_129', (1, 64, 128, 385, 5, 1, 1), _lds(tile_rows = 256, m_tiles_per_b = 2, full_tiles = 2, tail128 = 0), NO_SHORT | NO_NARROW),
	case('all_short_halves', (1, 64, 136, 129, 3, 1, 1), _lds(tile_rows = 128, m_tiles_per_b = 2, n_tiles = 2, total_tiles = 4, full_tiles = 0, narrow_parts = 2, tail128 = 2), epi = dict(bias = True)),
	case('quarters', (33, 64, 1024, 200, 3, 1, 1), _lds(tile_rows = 256, total_tiles = 264, full_tiles = 256, narrow_parts = 4, tail128 = 0), NO_SHORT, epi = dict(bias = True)),
	case('tile_walk', (17, 64, 384, 256, 3, 1, 1), _lds(tile_rows = 256, m_tiles_per_b = 1, n_tiles = 3, total_tiles = 51, full_tiles = 51), NO_SHORT | NO_NARROW, epi = dict(bias = True)),
	case('ring_wrap', (1, 320, 128, 257, 2, 1, 1), _lds(tile_rows = 256, total_tiles = 1), NO_SHORT, epi = dict(bias = True)),
	case('k1_three_buffers', (2, 192, 136, 300, 1, 1, 1), _lds(B = 2, T = 300, lds_bytes = 3 * 128 * 128 + 3 * 16384), epi = dict(bias = True, act = 'relu', xlen = (0.7, 1.0))),
	case('k1_flattened', (3, 128, 136, 100, 1, 1, 1), _lds(B = 1, T = 300, tile_rows = 128, m_tiles_per_b = 3), epi = dict(bias = True)),
	case('k1_not_flattened', (3, 128, 136, 100, 1, 1, 1), _lds(B = 3, T = 100, m_tiles_per_b = 1), NO_FLATTEN, epi = dict(bias = True)),
	case('wide_head', (2, 128, 38, 203, 1, 1, 1), _lds(B = 1, T = 406, n_tiles = 1), epi = dict(bias = True), out = 'f32'),
	case('halo_edge_in', (1, 64, 128, 300, 33, 1, 2), _lds(tile_rows = 256, x_rows = 320, lds_bytes = 160 * 1024), NO_SHORT, epi = dict(bias = True)),
	case('halo_edge_out', (1, 64, 128, 300, 34, 1, 2), _gen(x_rows = 194, xi = 9), NO_SHORT, epi = dict(bias = True)),
]
SAME_BITS = [('tile256_tail128_ragged_cout', 'tail_off_same_bits'), ('k1_flattened', 'k1_not_flattened')]
QUARTERS_BITS = (NO_SHORT | NO_QUARTERS, NO_SHORT | NO_NARROW)  # 'quarters' again as halves and as full tiles: the same bits

# split-K launches (ops.conv1d(..., splitk = True)): edges = (splits, input blocks per split, blocks of the last split)
SPLITK = [
	case('splitk_last_short', (1, 2112, 128, 100, 3, 1, 1), dict(splits = 17, cps = 2, last = 1), epi = dict(bias = True, scale = True, act = ('hardtanh', 0.0, 20.0), xlen = (0.7, )), splitk = True, ints = SMALL),
	case('splitk_f32', (1, 72, 256, 300, 5, 1, 1), dict(splits = 3, cps = 1, last = 1), epi = dict(bias = True, scale = True, act = ('hardtanh', 0.0, 20.0), xlen = (0.7, )), splitk = True, dtypes = ('f32', )),
]
# the split-K request the LDS-DMA kernel refuses at 256-row tiles ((K - 1) dil = 66 > 64): served by the unsplit launch
SPLITK_FALLBACK = case('splitk_outside_the_envelope', (1, 128, 128, 300, 23, 1, 3), _lds(tile_rows = 128, tail128 = 2), epi = dict(bias = True, scale = True, act = ('hardtanh', 0.0, 20.0), xlen = (0.7, )), splitk = True, dtypes = ('bf16', ))

# The register-staged kernel (csrc/conv.hip conv1d_igemm_kernel): fp32 always, 16-bit with the switch off (or outside the LDS-DMA envelope)
GENERAL = [
	case('xi5_partial_slab', (2, 96, 96, 77, 11, 1, 1), _gen(xi = 5, aligned_x = 1, x_rows = 138), v2 = 0, epi = dict(bias = True), dtypes = ALL),
	case('xi9_stride2_odd', (2, 64, 256, 301, 11, 2, 1), _gen(xi = 9, aligned_x = 1, x_rows = 266, T = 151), v2 = 0, epi = FULL, dtypes = ALL, ints = SMALL),
	case('xi16_stride2_dilated', (1, 64, 128, 301, 29, 2, 2), _gen(xi = 16, aligned_x = 1, x_rows = 312), v2 = 0, epi = dict(bias = True), dtypes = ALL),
	case('unaligned', (2, 38, 38, 203, 3, 1, 1), _gen(xi = 9, aligned_x = 0, x_rows = 130), v2 = 0, epi = FULL, dtypes = ALL, ints = SMALL),
	case('tout_truncated', (2, 64, 128, 141, 4, 1, 1), _gen(T = 139, m_tiles_per_b = 2), v2 = 0, epi = dict(bias = True), dtypes = ALL, trunc = 1),
]
REFUSED = case('unaligned_refused', (1, 38, 40, 301, 35, 2, 1), dict(route = 'refused', error = EUNSUPPORTED), v2 = 0, dtypes = ALL)

# The one-tap kernel (csrc/conv1x1.hip): M = 300 = 2 x 128 + 44 rows
ONE_TAP = [
	case('one_stage_ragged_m', (3, 64, 128, 100, 1, 1, 1), _tap(B = 1, T = 300, stages = 1, m_tiles_per_b = 3, total_tiles = 3, stats_rows = 3), epi = BIAS_STATS, ints = SMALL),
	case('two_stage_ragged_m', (3, 384, 128, 100, 1, 1, 1), _tap(B = 1, T = 300, stages = 2, m_tiles_per_b = 3, lds_bytes = 65536, stats_rows = 3), epi = BIAS_STATS, ints = SMALL),
]
ONE_TAP_BIAS_SIGMAS = 100.0
# grouped: (Cin, Cout) per problem over GROUPED_FRAMES = (B, T); both stage classes in one call
GROUPED = [(64, 128), (384, 128), (128, 256), (768, 256)]
GROUPED_FRAMES = (3, 100)
GROUPED_ACCUMULATE = [True, False, True, True]

# the packers: (Cout, Cin, K); the third 16-bit only (scalar kernels because 512 K 4 bytes > 64 KiB)
PACK = [(39, 37, 3), (136, 192, 5), (128, 64, 33)]

TABLES = dict(LDS_DMA = LDS_DMA, GENERAL = GENERAL, ONE_TAP = ONE_TAP)


def by_name(name):
	return next(c for t in (LDS_DMA, GENERAL, ONE_TAP, SPLITK, [SPLITK_FALLBACK, REFUSED]) for c in t if c.name == name)


def has_dgrad(c):
	"""every stride-1 case also runs as an input gradient (of a truncated case: dy has the frames the geometry yields, the last `trunc` zero)"""
	return c.stride == 1 and not c.splitk
