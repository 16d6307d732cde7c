"""The fused BN-backward epilogue of the dgrad launch with stored gates (conv_v2s.hip, form 2) and the narrow tiles of a last partial
round, at the smallest shapes that reach each of their paths.  `-m gpu` needs an MI355X.

What is checked: dx is bit-identical to the plain launch of the same conv; sum g and sum g xhat agree with a float64 restatement
within the bound of the kernel's arithmetic; repeated launches are bit-identical; half and quarter tiles change no bit.

The bound.  Per 256-row tile and channel the kernel sums G = gate ? dz : 0 and G y (products of two 16-bit values: exact in fp32) in
fp32 chains of n <= 256 terms, scales both by k = 1 / (1 - p) and centres once: (s2 - mean s1) invstd, all in fp32 (u = 2^-24); the
per-tile rows are then added in fp64.  With A1 = k sum |G| and A2 = k sum |G y| over the whole launch:
  |sum g      - exact| <= (n + 2) u A1                              (the chain, the scaling, k's own rounding)
  |sum g xhat - exact| <= (n + 6) u |invstd| (A2 + |mean| A1)      (two chains with their scalings, product, difference, product)
"""
import pytest
import torch

gpu = pytest.mark.gpu
DT = dict(bf16 = torch.bfloat16, f16 = torch.float16)
U, N_CHAIN = 2.0 ** -24, 256
NO_SHORT_LAUNCH, NO_NARROW, NO_QUARTERS = 2048, 32, 16  # ConvParams::debug bits (csrc/conv_v2s.hip, the dispatcher)


def dev():
	return torch.device('cuda:0')


class debug_bits:
	"""The forward / dgrad kernel's experiment flags for the duration of a block."""

	def __init__(self, bits):
		self.bits = bits

	def __enter__(self):
		from convasr_amd import _lib
		_lib.load().convasr_debug_set_conv_v2(1 | (self.bits << 8))

	def __exit__(self, *exc):
		from convasr_amd import _lib
		_lib.load().convasr_debug_set_conv_v2(1)


def problem(dt, B, T, C, Cdy, K, dil, seed = 0):
	"""A dgrad launch that produces dz of a C-channel layer over T frames from a Cdy-channel dy, and that layer's conv output y."""
	from convasr_amd import ops
	d = dev()
	torch.manual_seed(seed)
	pad = dil * (K - 1) - dil * (K // 2)
	Tdy = T + dil * (K - 1) - 2 * pad
	dy = ops.as_cl(torch.randn(B, Cdy, Tdy, device = d), dt)
	w = torch.randn(Cdy, C, K, device = d) / (Cdy * K) ** 0.5
	_, wd = ops.pack_weight(w, dt, None)
	y = ops.as_cl(torch.randn(B, C, T, device = d) * 4 + 2, dt)
	scale, shift = torch.rand(C, device = d) + 0.5, torch.randn(C, device = d)
	mean, invstd = torch.randn(C, device = d), torch.rand(C, device = d) + 0.5
	return dict(B = B, T = T, C = C, K = K, dil = dil, pad = pad, dy = dy, wd = wd, y = y, scale = scale, shift = shift, mean = mean, invstd = invstd)


def gates_of(pr, kind):
	"""(gate bytes, dropout p, xlen) -- ones / zeros: every gradient passes / none does; random: what the forward pass stores for hardtanh,
	utterances of half the frames and more, dropout 0.2."""
	from convasr_amd import ops, _lib
	d = dev()
	B, T, C = pr['B'], pr['T'], pr['C']
	n = B * T * C // 8
	if kind == 'ones':
		return torch.full((n,), 255, dtype = torch.uint8, device = d), 0.0, torch.ones(B, device = d)
	if kind == 'zeros':
		return torch.zeros(n, dtype = torch.uint8, device = d), 0.0, torch.ones(B, device = d)
	xlen = torch.linspace(0.5, 1, B, device = d)
	gate = torch.zeros(n, dtype = torch.uint8, device = d)
	ops.bn_act(pr['y'], pr['scale'], pr['shift'], ACT(), xlen = xlen, dropout_p = 0.2, seed = 3, offset = 5, gate = gate)
	return gate, 0.2, xlen


def ACT():
	from convasr_amd import _lib
	return (_lib.ACT_HARDTANH, 0.0, 20.0)


def fused(pr, gate, p_drop, xlen):
	from convasr_amd import ops
	sums = ops.ConvStats(pr['C'], pr['B'], pr['T'], dev())
	dx = ops.conv1d_dgrad_bn_reduce(pr['dy'], pr['wd'], pr['C'], pr['K'], pr['dil'], pr['pad'], pr['y'], pr['scale'], pr['shift'], pr['mean'], pr['invstd'], ACT(), p_drop, 3, 5, xlen, sums, gate = gate)
	assert dx is not None
	return dx, sums


def plain(pr):
	from convasr_amd import ops
	return ops.conv1d(pr['dy'], pr['wd'], pr['C'], pr['K'], 1, pr['dil'], pr['pad'])


def check_sums(pr, dx, sums, gate, p_drop, what):
	"""sum g and sum g xhat of the launch against float64 on the same dx, y and gate bits, within the derived bound (module docstring)."""
	B, T, C = pr['B'], pr['T'], pr['C']
	d = dev()
	bits = ((gate.view(B, T, C // 8, 1) >> torch.arange(8, device = d, dtype = torch.uint8)) & 1).reshape(B, T, C).permute(0, 2, 1).double()
	k = float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p_drop))) if p_drop else 1.0
	G, y = dx.double() * bits * k, pr['y'].double()
	mean, invstd = pr['mean'].double(), pr['invstd'].double()
	s1 = G.sum(dim = (0, 2))
	s2 = (G * (y - mean.view(1, C, 1))).sum(dim = (0, 2)) * invstd
	A1, A2 = G.abs().sum(dim = (0, 2)), (G * y).abs().sum(dim = (0, 2))
	b1 = (N_CHAIN + 2) * U * A1
	b2 = (N_CHAIN + 6) * U * invstd.abs() * (A2 + mean.abs() * A1)
	got = sums.totals()
	e1, e2 = (got[:C] - s1).abs(), (got[C:] - s2).abs()
	print(f'{what}: sum g err / bound {float((e1 / b1.clamp_min(1e-300)).max()):.3f}, sum g xhat err / bound {float((e2 / b2.clamp_min(1e-300)).max()):.3f}')
	assert bool(torch.isfinite(got).all()), what
	assert bool((e1 <= b1).all()), f'{what}: sum g, worst err {float(e1.max()):.3e} (bound there {float(b1[e1.argmax()]):.3e})'
	assert bool((e2 <= b2).all()), f'{what}: sum g xhat, worst err {float(e2.max()):.3e} (bound there {float(b2[e2.argmax()]):.3e})'


# (B, T, C, Cdy, K, dil): T = 256 one full tile, 450 a full-height tail with the row predicate, 300 a 128-row tail; C = 192 a ragged second
# n tile; every K with its own loop form (1: three X buffers; 2: no read-ahead; 3: one and a half tap pairs; 11) and both dilations;
# Cdy = 128 two input slabs (the y half fetched early sits in the other X buffer than with one).  Each runs as the dispatcher would run it
# (so few tiles: 128-row tiles for the whole launch; B = 1, T = 256, C = 128 is that form's smallest) and with 256-row tiles.
SHAPES = [
	(1, 256, 128, 64, 3, 1),
	(2, 256, 128, 64, 1, 1),
	(2, 450, 128, 64, 2, 1),
	(2, 300, 128, 64, 3, 2),
	(3, 450, 192, 128, 11, 1),
	(2, 300, 192, 64, 11, 2),
	(4, 256, 192, 128, 2, 2),
	(2, 300, 128, 128, 1, 1),
	(2, 450, 192, 128, 3, 1),
]


@gpu
@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('shape', SHAPES, ids = lambda s: 'B%d-T%d-C%d-Cdy%d-K%d-d%d' % s)
def test_fused_gated_dgrad_against_the_plain_launch_and_float64(shape, dtype):
	pr = problem(DT[dtype], *shape)
	for bits in (0, NO_SHORT_LAUNCH):
		with debug_bits(bits):
			ref = plain(pr)
			for kind in ('ones', 'zeros', 'random'):
				gate, p_drop, xlen = gates_of(pr, kind)
				dx, sums = fused(pr, gate, p_drop, xlen)
				what = f'{shape} {dtype} debug {bits} gates {kind}'
				assert torch.equal(dx, ref), what
				if kind == 'zeros':
					assert not bool(sums.totals().any()), what
				check_sums(pr, dx, sums, gate, p_drop, what)


@gpu
@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
def test_fused_gated_dgrad_is_bit_identical_over_20_launches(dtype):
	pr = problem(DT[dtype], 4, 450, 192, 128, 11, 1, seed = 1)
	gate, p_drop, xlen = gates_of(pr, 'random')
	for bits in (0, NO_SHORT_LAUNCH):
		with debug_bits(bits):
			dx0, s0 = fused(pr, gate, p_drop, xlen)
			rows0 = s0.buf[:s0.rows * 2 * pr['C']].clone()
			for _ in range(19):
				dx, s = fused(pr, gate, p_drop, xlen)
				assert s.rows == s0.rows and torch.equal(dx, dx0) and torch.equal(s.buf[:s.rows * 2 * pr['C']], rows0)


@gpu
@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('part', ['quarter', 'half'])
def test_narrow_tiles_of_a_last_partial_round_change_no_bit(part, dtype):
	"""One whole round of tiles plus r: r at most a quarter of the CUs (the rest runs as quarter tiles), r between a quarter and a half (half
	tiles).  Forward with BN statistics and fused dgrad: outputs and partial rows bit-identical to the launch with narrow tiles off."""
	from convasr_amd import ops
	n_cu = torch.cuda.get_device_properties(dev()).multi_processor_count
	r = n_cu // 8 if part == 'quarter' else 3 * n_cu // 8
	pr = problem(DT[dtype], n_cu + r, 256, 128, 64, 3, 1, seed = 2)  # one tile per utterance
	gate, p_drop, xlen = gates_of(pr, 'random')

	def run():
		st = ops.ConvStats(pr['C'], pr['B'], pr['T'], dev())
		yf = ops.conv1d(pr['dy'], pr['wd'], pr['C'], pr['K'], 1, pr['dil'], pr['pad'], stats = st)
		dx, sums = fused(pr, gate, p_drop, xlen)
		return yf, st.buf[:st.rows * 2 * pr['C']].clone(), dx, sums.buf[:sums.rows * 2 * pr['C']].clone(), sums

	got = run()
	assert torch.equal(got[2], got[0])  # (the fused launch's dx is the plain launch's output)
	check_sums(pr, got[2], got[4], gate, p_drop, f'{part} tiles {dtype}')
	for bits in (NO_NARROW, NO_QUARTERS):
		with debug_bits(bits):
			ref = run()
		for a, b in zip(got[:4], ref[:4]):
			assert torch.equal(a, b), (part, dtype, bits)
