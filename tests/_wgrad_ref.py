"""Float64 restatement of the dense weight gradient, the yardsticks the GPU tests hold the kernels to, and the case tables.

Plain torch / numpy on the CPU; the library is not imported here.  tests/test_wgrad_ref.py holds this file to float64 autograd of F.conv1d
and holds every case of the tables to the edge it claims (asked of the library's own plan query); tests/test_wgrad_kernels_gpu.py runs
the tables on the MI355X.

Tensors are the logical (B, C, T) ones; the kernels' channels-last memory is the GPU file's business.

A case names the edge it is there for as data (`edges`, per dtype): route ('general' / 'lds_dma'), cps (chunks per split), last (chunks
of the last split), last_taps (taps of the last tap group), tap_groups, pieces (1-KiB LDS-DMA pieces per chunk), tail (frames of an
utterance's last chunk), align ((AX, AY): are rows of x / dy 16-byte multiples?), xi (the general kernel's XI instantiation, 5 or 12),
x_rows.  edges_of() derives the same names from a plan the library reports."""
import collections

import numpy as np
import torch

U32 = 2.0 ** -24    # unit roundoff of fp32
TINY = 2.0 ** -126  # smallest normal fp32
CORNER = 32         # chain32 carries the (co, ci) < CORNER corner

DTYPES = dict(f32 = torch.float32, bf16 = torch.bfloat16, f16 = torch.float16)
HALVES = ('bf16', 'f16')
ALL = ('f32', 'bf16', 'f16')


def tin_of(Tout, K, stride, dil, pad):
	"""the input length whose conv output has exactly Tout frames"""
	return (Tout - 1) * stride + dil * (K - 1) + 1 - 2 * pad


def _tap_range(k, Tin, Tout, stride, dil, pad):
	"""output frames [t0, t1) whose tap k reads inside [0, Tin), and the first input frame read"""
	off = k * dil - pad
	t0 = max(0, -(off // stride)) if off < 0 else 0
	t1 = min(Tout, (Tin - 1 - off) // stride + 1) if Tin - 1 - off >= 0 else 0
	return t0, max(t1, t0), t0 * stride + off


def wgrad(x, dy, K, stride, dil, pad):
	"""dw[co, ci, k] = sum_{b, t} dy[b, co, t] x[b, ci, t stride + k dil - pad] over the frames dy has (terms outside [0, Tin) dropped),
	dbias[co] = sum dy, and absdot = the same sum over |dy| |x|: float64 (Cout, Cin, K), (Cout,), (Cout, Cin, K)."""
	x, dy = x.double(), dy.double()
	(B, Cin, Tin), (_, Cout, Tout) = x.shape, dy.shape
	dw, absdot = torch.zeros(Cout, Cin, K, dtype = torch.float64), torch.zeros(Cout, Cin, K, dtype = torch.float64)
	ax, ady = x.abs(), dy.abs()
	for k in range(K):
		t0, t1, i0 = _tap_range(k, Tin, Tout, stride, dil, pad)
		if t1 <= t0:
			continue
		sel = slice(i0, i0 + (t1 - t0 - 1) * stride + 1, stride)
		for src_y, src_x, dst in ((dy, x, dw), (ady, ax, absdot)):
			a = src_y[:, :, t0:t1].permute(1, 0, 2).reshape(Cout, -1)
			b = src_x[:, :, sel].permute(1, 0, 2).reshape(Cin, -1)
			dst[:, :, k] = a @ b.t()
	return dw, dy.sum(dim = (0, 2)), absdot


def chain32(x, dy, K, stride, dil, pad, corner = CORNER):
	"""The (co, ci) < corner block of the same sum carried in ONE fp32 accumulator per element, frame after frame, utterance after
	utterance: the least accurate order a plain fp32 kernel could use.  Each product is rounded to fp32 first (exact already when the
	operands are 16-bit values).  float32 (co, ci, K) numpy array."""
	xn, yn = x.float().numpy(), dy.float().numpy()
	(B, Cin, Tin), (_, Cout, Tout) = xn.shape, yn.shape
	co, ci = min(corner, Cout), min(corner, Cin)
	lo = pad
	hi = max(0, (Tout - 1) * stride + (K - 1) * dil - pad - (Tin - 1))
	xp = np.zeros((B, ci, lo + Tin + hi), dtype = np.float32)  # zero frames outside [0, Tin): adding 0.0 leaves an accumulator as it is
	xp[:, :, lo:lo + Tin] = xn[:, :ci]
	taps = np.arange(K) * dil
	acc = np.zeros((co, ci, K), dtype = np.float32)
	for b in range(B):
		for t in range(Tout):
			acc += yn[b, :co, t][:, None, None] * xp[b][:, t * stride + taps][None]
	assert acc.dtype == np.float32
	return acc


def chain32_rows(y):
	"""column sums of a (rows, C) matrix, one fp32 accumulator per column, row after row (C < CORNER columns at most)"""
	a = np.ascontiguousarray(y.float().numpy()[:, :CORNER])
	acc = np.zeros(a.shape[1], dtype = np.float32)
	for r in range(a.shape[0]):
		acc += a[r]
	return acc


# ---- the stride-2 fold (csrc/conv.hip, "stride-2 fold"): P' = ceil(pad / 2), s0 = 2 P' - pad, K' = (K - 1 + s0) / 2 + 1, k = 2 j + p - s0

def fold2(K, pad):
	"""(K', P', s0)"""
	pf = (pad + 1) // 2
	s0 = 2 * pf - pad
	return (K - 1 + s0) // 2 + 1, pf, s0


def fold_view(x):
	"""(B, Cin, T) with T even -> the (B, 2 Cin, T / 2) view: row r = frames 2 r, 2 r + 1 side by side"""
	B, Cin, T = x.shape
	assert T % 2 == 0
	return x.reshape(B, Cin, T // 2, 2).permute(0, 3, 1, 2).reshape(B, 2 * Cin, T // 2)


def unfold(dwf, K, pad):
	"""(Cout, 2 Cin, K') gradient of the folded conv -> (Cout, Cin, K): dw[co, ci, k] = dwf[co, p Cin + ci, j] with 2 j + p - s0 = k"""
	Kf, _, s0 = fold2(K, pad)
	Cout, Cin2, kf = dwf.shape
	assert kf == Kf and Cin2 % 2 == 0
	Cin = Cin2 // 2
	dw = torch.empty(Cout, Cin, K, dtype = dwf.dtype)
	for k in range(K):
		j, p = (k + s0) >> 1, (k + s0) & 1
		dw[:, :, k] = dwf[:, p * Cin:(p + 1) * Cin, j]
	return dw


# ---- operands

def integer_operands(shape, seed):
	"""x, dy of integers from -1 ... 6 (exact in bf16, f16 and fp32; deliberately not centred, so partial sums grow past every short format)"""
	g = torch.Generator().manual_seed(seed)
	B, Cin, Tin, Cout, Tout = shape
	return torch.randint(-1, 7, (B, Cin, Tin), generator = g).float(), torch.randint(-1, 7, (B, Cout, Tout), generator = g).float()


def random_operands(shape, seed, dtype):
	"""randn rounded to the storage type, as fp32 tensors"""
	g = torch.Generator().manual_seed(seed)
	B, Cin, Tin, Cout, Tout = shape
	return torch.randn(B, Cin, Tin, generator = g).to(dtype).float(), torch.randn(B, Cout, Tout, generator = g).to(dtype).float()


# ---- case tables

Case = collections.namedtuple('Case', 'name B Cin Cout Tout K stride dil pad v2 trunc edges')


def case(name, shape, edges, pad = None, v2 = 1, trunc = 0):
	"""shape = (B, Cin, Cout, Tout, K, stride, dil); pad None = dil (K - 1) / 2; trunc: frames fewer than the geometry yields; v2: the
	convasr_debug_set_conv_v2 state the case runs under; edges: {dtype name: {edge name: value}} -- the dtypes are the ones it runs in"""
	B, Cin, Cout, Tout, K, stride, dil = shape
	return Case(name, B, Cin, Cout, Tout, K, stride, dil, dil * (K - 1) // 2 if pad is None else pad, v2, trunc, edges)


def tin(c):
	return tin_of(c.Tout + c.trunc, c.K, c.stride, c.dil, c.pad)


def edges_of(c, dtype_name, plan):
	"""what a plan reported by the library (ops.wgrad_plan) says about the edges a case may claim"""
	e = dict(route = plan['route'])
	if plan['route'] == 'refused':
		return e
	esize = 4 if dtype_name == 'f32' else 2
	total = c.B * plan['chunks_per_b']
	bkt = 64 if plan['route'] == 'lds_dma' or esize == 2 else 32  # frames per chunk: W2_BKT, WgTile<T>::BKT
	e.update(cps = plan['chunks_per_split'], splits = plan['splits'], last = total - (plan['splits'] - 1) * plan['chunks_per_split'], tap_groups = plan['tap_groups'],
	         last_taps = c.K - 4 * (plan['tap_groups'] - 1), x_rows = plan['x_rows'], tail = c.Tout - bkt * (plan['chunks_per_b'] - 1))
	if plan['route'] == 'lds_dma':
		e['pieces'] = 64 // 4 + plan['x_rows'] // 4
	else:
		e['align'] = ((c.Cin * esize) % 16 == 0, (c.Cout * esize) % 16 == 0)
		per_row = 32 if esize == 4 else 16  # 16-byte pieces of a staged row: WgTile<T>::CPR
		e['xi'] = 5 if e['align'] == (True, True) and -(-plan['x_rows'] * per_row // 256) <= 5 else 12
		e['xi_used'] = -(-plan['x_rows'] * per_row // 256)
	return e


def _both(**e):
	return dict(bf16 = dict(route = 'lds_dma', **e), f16 = dict(route = 'lds_dma', **e))


def _bf(**e):
	return dict(bf16 = dict(route = 'lds_dma', **e))


# The LDS-DMA kernel (csrc/wgrad_v2.hip): 64-frame chunks, a 4-stage ring issued three chunks ahead, tap groups of 4.
LDS_DMA = [
	# taps of the last group: 1, 2, 3, 4 taps are different loop instantiations; 1 and 3 share a tap between the wave halves
	case('one_chunk', (1, 128, 128, 64, 1, 1, 1), _both(cps = 1, splits = 1, last_taps = 1, pieces = 32, tail = 64)),
	case('taps2_tail1', (2, 128, 128, 65, 2, 1, 1), _bf(last_taps = 2, tail = 1)),
	case('taps3', (2, 128, 256, 129, 3, 1, 1), _both(last_taps = 3, tail = 1)),
	case('taps4+1', (1, 128, 128, 200, 5, 1, 1), _bf(tap_groups = 2, last_taps = 1)),
	case('taps4+2', (1, 128, 128, 200, 6, 1, 1), _bf(tap_groups = 2, last_taps = 2)),
	case('taps4+3', (1, 128, 128, 200, 7, 1, 1), _both(tap_groups = 2, last_taps = 3)),
	case('taps4+4+3', (1, 128, 128, 200, 11, 1, 1), _bf(tap_groups = 3, last_taps = 3)),
	# DMA pieces per chunk: the four loader waves issue ceil((pieces - w) / 4) each and wait on their own count
	case('pieces33', (1, 256, 128, 200, 4, 1, 1), _bf(pieces = 33, last_taps = 4)),
	case('pieces34', (1, 256, 128, 200, 4, 1, 2), _bf(pieces = 34)),
	case('pieces35', (1, 256, 128, 200, 4, 1, 3), _bf(pieces = 35)),
	case('pieces36', (1, 256, 128, 200, 4, 1, 5), _bf(pieces = 36)),
	case('pieces37', (1, 256, 128, 200, 4, 1, 6), _bf(pieces = 37)),
	case('pieces38', (1, 256, 128, 200, 4, 1, 7), _bf(pieces = 38)),
	case('pieces39', (1, 256, 128, 200, 4, 1, 9), _bf(pieces = 39)),
	case('pieces40_envelope_edge', (1, 256, 128, 200, 4, 1, 10), _both(pieces = 40, x_rows = 96)),
	case('past_the_envelope', (1, 256, 128, 200, 4, 1, 11), dict(bf16 = dict(route = 'general', x_rows = 97), f16 = dict(route = 'general', x_rows = 97))),
	# ring depth: a slot of the 4-stage ring is reused from 5 chunks per split on
	case('ring2_last1', (1, 128, 128, 2112, 1, 1, 1), _bf(cps = 2, last = 1)),
	case('ring3', (2, 128, 128, 2049, 1, 1, 1), _bf(cps = 3, tail = 1)),
	case('ring4_last1', (1, 128, 128, 6208, 1, 1, 1), _bf(cps = 4, last = 1)),
	case('ring5_last2', (4, 128, 128, 2100, 3, 1, 1), _both(cps = 5, last = 2, last_taps = 3)),  # splits cross utterance ends: 33 chunks per utterance
	case('ring5_last4_two_groups', (3, 128, 128, 2752, 6, 1, 1), _bf(cps = 5, last = 4, tap_groups = 2)),
	case('ring8_last2', (2, 128, 128, 7171, 1, 1, 1), _bf(cps = 8, last = 2)),
	case('ring12_workload', (8, 128, 128, 3000, 2, 1, 1), _both(cps = 12, last = 4, splits = 32)),
	case('ring4_pieces37', (2, 256, 256, 1100, 7, 1, 6), _bf(cps = 4, pieces = 37, splits = 9, tap_groups = 2)),
	# padding, with B >= 2 and Tout % 64 != 0: frames before an utterance's start and after its end read as zero, never as its neighbour's
	case('pad0', (3, 128, 128, 150, 3, 1, 2), _bf(tail = 22), pad = 0),
	case('pad_symmetric', (3, 128, 128, 150, 3, 1, 2), _bf(tail = 22), pad = 2),
	case('pad_one_sided', (3, 128, 128, 150, 3, 1, 2), _bf(tail = 22), pad = 4),
	case('pad_beyond_window', (2, 128, 128, 100, 5, 1, 3), _bf(tail = 36, tap_groups = 2), pad = 12),
	# one frame fewer than the geometry yields (what the stride-2 fold asks for)
	case('truncated', (2, 128, 128, 150, 6, 1, 1), _bf(tap_groups = 2, last_taps = 2), pad = 3, trunc = 1),
	# 2.5 M gradient elements: the tap-major combine's 2048-workgroup cap turns it into a grid-stride loop
	case('combine_grid_cap', (1, 384, 384, 40, 17, 1, 1), _bf(tap_groups = 5, last_taps = 1)),
]
STARRED = [c for c in LDS_DMA if 'f16' in c.edges and c.edges['f16']['route'] == 'lds_dma']  # the ones the in-place plane reads run too
SAME_BITS = ('taps4+3', 'ring5_last2', 'pieces40_envelope_edge')  # both kernels on the same integer data, switch on and off


def _gen(f32 = None, h = None, **common):
	"""edges of a general-kernel case: f32 / h = what differs for fp32 and for the two 16-bit types"""
	out = {}
	if f32 is not None:
		out['f32'] = dict(route = 'general', **common, **f32)
	if h is not None:
		out['bf16'] = dict(route = 'general', **common, **h)
		out['f16'] = dict(route = 'general', **common, **h)
	return out


TT, TF, FT, FF = (True, True), (True, False), (False, True), (False, False)
# The general kernel (csrc/conv.hip conv1d_wgrad_kernel): chunks of 64 frames (16-bit) / 32 frames (fp32), a two-deep register-staged ring.
GENERAL = [
	case('one_frame', (2, 8, 8, 1, 1, 1, 1), _gen({}, {}, cps = 1, tail = 1)),
	# the four alignment instantiations: 36 channels are 16-byte rows in fp32 only, 35 in neither
	case('align_40_40', (2, 40, 40, 70, 3, 1, 1), _gen({}, {}, align = TT, xi = 5)),
	case('align_36_40', (2, 36, 40, 70, 3, 1, 1), _gen(dict(align = TT), dict(align = FT, xi = 12))),
	case('align_40_36', (2, 40, 36, 70, 3, 1, 1), _gen(dict(align = TT), dict(align = TF, xi = 12))),
	case('align_35_40', (2, 35, 40, 70, 3, 1, 1), _gen({}, {}, align = FT, xi = 12)),
	case('align_40_35', (2, 40, 35, 70, 3, 1, 1), _gen({}, {}, align = TF, xi = 12)),
	case('align_35_35', (2, 35, 35, 70, 3, 1, 1), _gen({}, {}, align = FF, xi = 12)),
	# the XI = 5 / 12 instantiation boundary of the aligned kernel
	case('xi5_f32', (2, 72, 72, 90, 4, 1, 2), _gen(dict(xi = 5, xi_used = 5, align = TT))),
	case('xi12_f32', (2, 72, 72, 90, 4, 1, 3), _gen(dict(xi = 12, xi_used = 6, align = TT))),
	case('xi5_h', (2, 72, 72, 90, 4, 1, 5), _gen(None, dict(xi = 5, xi_used = 5, align = TT))),
	case('xi12_h', (2, 72, 72, 90, 4, 1, 6), _gen(None, dict(xi = 12, xi_used = 6, align = TT))),
	# the x_rows limit: the widest tap window the kernel takes
	case('x_rows_limit_h', (1, 16, 16, 40, 4, 2, 21), _gen(None, dict(xi_used = 12, x_rows = 190))),
	case('x_rows_limit_f32', (1, 16, 16, 40, 4, 2, 11), _gen(dict(xi_used = 12, x_rows = 96))),
	# ragged tiles
	case('ragged_cout_130', (2, 100, 130, 70, 5, 2, 1), _gen({}, {}, tap_groups = 2, last_taps = 1)),
	case('ragged_3x2_tiles', (1, 129, 257, 33, 9, 1, 3), _gen({}, {}, tap_groups = 3, last_taps = 1, align = FF)),
	case('ragged_k13_stride2', (3, 64, 200, 97, 13, 2, 2), _gen({}, {}, tap_groups = 4, last_taps = 1)),
	# K = 64: 16 tap groups, the reference combine's [64][65] LDS tile
	case('k64', (1, 24, 136, 31, 64, 1, 1), _gen({}, {}, tap_groups = 16, last_taps = 4)),
	# loop depth: the double-buffer loop body runs more than once from 2 chunks per split on
	case('loop3_5', (4, 100, 72, 1100, 5, 1, 1), _gen(dict(cps = 5), dict(cps = 3))),
	case('loop5_9_short_last', (3, 64, 72, 2752, 6, 1, 1), _gen(dict(cps = 9, last = 6), dict(cps = 5, last = 4))),
	case('loop8_15', (2, 64, 64, 7171, 1, 1, 1), _gen(dict(cps = 15), dict(cps = 8, last = 2))),
	case('loop8_15_switch_off', (2, 128, 128, 7171, 1, 1, 1), _gen(dict(cps = 15), dict(cps = 8, last = 2)), v2 = 0),
	# one frame fewer than the geometry yields, stride 1, K even
	case('truncated', (2, 40, 40, 70, 4, 1, 1), _gen({}, {}, align = TT), pad = 2, trunc = 1),
]

# the reference-layout combine (wgrad_reduce_kernel) works on 64-column blocks of Cin with a k += 4 loop
REDUCE_CIN, REDUCE_K = (24, 64, 65, 129), (1, 3, 4, 5, 64)

# the bias gradient: colsum_kernel owns 256 rows per block, colsum_final_kernel adds the partial rows over 16 row-lanes (4097 rows = the 17th)
BIAS_ROWS, BIAS_C = (1, 255, 256, 257, 4096, 4097, 70001), (1, 38, 64, 65, 200)

# the grouped one-tap launch: (frames (B, T), [(Cin, Cout) per problem], claimed (splits, chunks per split) or None)
GROUPED_MAX = 12
GROUPED = [
	((1, 64), [(128, 128)], (1, 1)),
	((1, 64), [(128, 256), (384, 128)], (1, 1)),
	((2, 2049), [(128, 256), (256, 128)], (22, 3)),
	((2, 2049), [(128, 128), (256, 128), (128, 384), (384, 256), (256, 256)], (14, 5)),
	((2, 2049), [(128, 128), (256, 128), (128, 256)] * 4, (11, 6)),
	((8, 3000), [(128, 128)], (32, 12)),
	((8, 3000), [(256, 128), (128, 256)], (32, 12)),
	((8, 3000), [(128, 256), (128, 128), (128, 128), (128, 128), (128, 128)], (32, 12)),  # the workload's depth, the split count set by the 6 summed units
	((8, 3000), [(128, 384), (256, 128), (384, 256), (128, 128), (256, 256)], (16, 24)),
	((8, 3000), [(128, 128)] * 12, (21, 18)),
]

# the stride-2 fold: (Cout, Cin, K, pad); the first is the prologue's own geometry, the last (720 k elements) makes the unfold a grid-stride loop
FOLD = [(256, 64, 11, 5), (128, 64, 13, 6), (128, 64, 4, 2), (128, 64, 5, 0), (256, 128, 3, 1), (128, 64, 1, 0), (256, 256, 11, 5)]
FOLD_B, FOLD_TIN = 2, 300
