"""The reverberation kernels (csrc/augment.hip: convasr_augment_reverb_params, convasr_augment_reverb) through ops.reverb_params,
ops.augment_reverb, augment.WaveformAugment and augment.batches, against the float64 restatement (tests/_reverb_ref.py, itself checked on the CPU by
tests/test_reverb_ref.py).  The augmentation is this project's own, unpinned against any outside library.

Samples.  The FFT route is held to an independent float32 formulation of the same convolution: e32 = max |z32 - z64| of a whole-signal
torch.fft.rfft / irfft convolution (one power-of-two FFT over out_len + rir_len - 1 samples, on the CPU) of the same y and h, and the bar is
    max |z_gpu - z64| <= 4 e32   for every utterance,
the factor 4 paying for another radix schedule and tabulated twiddles.  The worst ratio seen on the GPU, 1.67, is recorded per kind of impulse
response in profiles/r20_reverb.json (a float32 emulation of the partitioned method on the CPU stayed below 1.8 e32 on these inputs).  An utterance with min(rir_len, out_len) <=
ops.reverb_direct() is summed directly, t <= min(rir_len, out_len) fma per sample in ascending tap index, and held to the sequential-sum bound of
tests/test_resample_gpu.py:  |z_gpu - z64| <= (t + 2) 2^-24 sum_k |h[k] y[n + d - k]|  per sample.

Integers (drawn rows, parameters) and everything stated as exact are compared with torch.equal."""
import math

import numpy as np
import pytest
import torch

import _augment_ref as A
import _reverb_ref as RR

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
BK = 1024  # convasr_augment_reverb_block(), asserted below
T = 5 * BK + 3
NPARTS = -(-T // RR.TILE)  # min(tiles, convasr_augment_parts()) workgroups leave a pair of energies per utterance
OUT_LENS = [1, BK - 1, BK, BK + 1, 2 * BK + 3, T]
RIR_LENS = [1, 2, BK - 1, BK, BK + 1, 3 * BK + 5]
KINDS = ['unit spike', 'two spikes', 'flat noise', 'decaying noise']
WORST = {}  # kind -> the worst |z_gpu - z64| / e32 seen (printed; profiles/r20_reverb.json records it)


def dev():
	return torch.device('cuda:0')


def make_params(out_len, T):
	"""A (B, 8) parameter tensor of the caller's own making: speed 1, no gain, no noise, the given out_len."""
	p = np.zeros((len(out_len), 8), dtype = np.int64)
	p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 6], p[:, 7] = -1, A.ONE, -1, -1, T, out_len
	return p


def make_rir(kind, L, d, rng):
	"""One impulse response of L taps whose first largest |tap| sits at d."""
	h = np.zeros(L, dtype = np.float64)
	if kind == 'unit spike':
		h[d] = 1.0
	elif kind == 'two spikes':
		h[L - 1] = -0.5
		h[0] = 1.0  # (L == 1: the one tap is 1)
	else:
		h = rng.normal(size = L) * (np.exp(-math.log(1000.0) * np.arange(L) / L) if kind == 'decaying noise' else 1.0)
		h[d] = 1.5 * np.abs(h).max()
		h /= math.sqrt((h * h).sum())
	return h.astype(np.float32)


def delays_of(kind, L):
	return [0] if kind == 'two spikes' else sorted({0, min(1, L - 1), L - 1})


def e32_of(y, h, d, out_len, z64):
	"""The float32 whole-signal FFT convolution's max error against z64 over n < out_len."""
	n = out_len + len(h) - 1
	nf = 1 << max(int(math.ceil(math.log2(n))), 1)
	z32 = torch.fft.irfft(torch.fft.rfft(torch.from_numpy(y[:out_len].copy()), nf) * torch.fft.rfft(torch.from_numpy(h), nf), nf).numpy()[d:d + out_len]
	return float(np.abs(z32.astype(np.float64) - z64[:out_len]).max())


def judge(z_gpu, y, h, d, out_len, what, extra = 0.0, kind = None):
	"""One utterance against the restatement: the direct route's per-sample bound or 4 e32 (+ extra, per sample)."""
	from convasr_amd import ops
	z64 = RR.reverb_one(y, h, d, out_len)
	err = np.abs(z_gpu.astype(np.float64) - z64)
	assert not z_gpu[out_len:].any(), what
	t = min(len(h), out_len)
	if t <= ops.reverb_direct():
		bound = (t + 2) * U * RR.reverb_one(np.abs(y), np.abs(h), d, out_len) + extra
		assert (err <= bound).all(), (what, 'direct', float(err.max()))
		return z64
	e32 = e32_of(y, h, d, out_len, z64)
	assert e32 > 0, what
	if kind is not None:
		WORST[kind] = max(WORST.get(kind, 0.0), float(err.max()) / e32)
	assert (err[:out_len] <= 4 * e32 + (extra[:out_len] if isinstance(extra, np.ndarray) else extra)).all(), (what, float(err.max()), e32, float(err.max()) / e32)
	return z64


def bank_tensors(hs, d):
	from convasr_amd import ops
	Lmax = max(len(h) for h in hs)
	bank = np.zeros((len(hs), Lmax), dtype = np.float32)
	for r, h in enumerate(hs):
		bank[r, :len(h)] = h
	lengths = torch.tensor([len(h) for h in hs], dtype = torch.int64)
	rir = torch.from_numpy(bank)
	delays = ops.rir_delays(rir, lengths)
	return bank, rir.to(d), lengths.to(d), delays.to(d), (lengths, delays)


# ------------------------------------------------------------------------------------------------ samples

@pytest.mark.parametrize('kind', KINDS)
def test_every_utterance_is_within_four_times_the_float32_fft_error_of_float64(kind):
	from convasr_amd import ops
	assert ops.reverb_block() == BK and 1 <= ops.reverb_direct() < BK - 1
	d = dev()
	B = 8
	rng = np.random.default_rng(KINDS.index(kind))
	y_host = rng.uniform(-0.5, 0.5, (B, T)).astype(np.float32)  # (garbage behind every out_len: the kernel reads y as 0 there)
	y = torch.from_numpy(y_host).to(d)
	out_len = np.array(OUT_LENS + [BK + 7, 3 * BK], dtype = np.int64)
	params = torch.from_numpy(make_params(out_len, T)).to(d)
	for which in range(3):  # the delay: 0, 1, rir_len - 1 (fewer where the kind or the length leaves fewer)
		hs, want_d = [], []
		for L in RIR_LENS:
			ds = delays_of(kind, L)
			want_d.append(ds[min(which, len(ds) - 1)])
			hs.append(make_rir(kind, L, want_d[-1], rng))
		bank, rir, lengths, delays, host = bank_tensors(hs, d)
		assert host[1].tolist() == want_d
		for shift in range(len(RIR_LENS)):  # every out_len meets every rir_len; utterance 6 draws no row, utterance 7 one outside the bank
			rows = np.array([(b + shift) % len(hs) for b in range(6)] + [-1, len(hs) + 3], dtype = np.int64)
			rir_row = torch.from_numpy(rows).to(d)
			out, partials = ops.augment_reverb(y, params, rir_row, rir, lengths, delays, host = host)
			ex = partials[:, :NPARTS, 0].sum(dim = 1).cpu().numpy()  # (the parts behind min(tiles, parts) are neither written nor read)
			again, _ = ops.augment_reverb(y, params, rir_row, rir, lengths, delays, host = host)
			assert torch.equal(out, again)  # two runs are bit-equal
			got = out.cpu().numpy()
			for b in range(B):
				what = (kind, 'delay', which, 'shift', shift, 'utterance', b)
				if b >= 6:  # no row: y bit for bit below out_len, 0 behind it
					assert np.array_equal(got[b, :out_len[b]], y_host[b, :out_len[b]]) and not got[b, out_len[b]:].any(), what
					continue
				r = rows[b]
				judge(got[b], y_host[b], hs[r], want_d[r], int(out_len[b]), what, kind = kind)
				if kind == 'unit spike' and min(len(hs[r]), out_len[b]) <= ops.reverb_direct():
					assert np.array_equal(got[b, :out_len[b]], y_host[b, :out_len[b]]), what  # 1 * y + 0 is exact
				e = float((got[b].astype(np.float64) ** 2).sum())
				assert abs(ex[b] - e) <= 1e-12 * e, what  # the energies are float64 sums of the samples written
	print(f'worst |z_gpu - z64| / e32, {kind}: {WORST.get(kind, 0.0):.3f}')
	torch.cuda.synchronize()


def test_an_utterance_is_bit_equal_wherever_it_sits_and_whatever_else_is_in_the_batch():
	from convasr_amd import ops
	d = dev()
	rng = np.random.default_rng(10)
	B = 8
	y_host = rng.uniform(-0.5, 0.5, (B, T)).astype(np.float32)
	out_len = np.array(OUT_LENS + [BK + 7, 3 * BK], dtype = np.int64)
	hs = [make_rir('decaying noise', L, 0, rng) for L in RIR_LENS]
	_, rir, lengths, delays, host = bank_tensors(hs, d)
	rows = np.array([5, 4, 3, 5, 2, 5, -1, 0], dtype = np.int64)
	run = lambda idx: ops.augment_reverb(torch.from_numpy(y_host[idx]).to(d), torch.from_numpy(make_params(out_len[idx], T)).to(d), torch.from_numpy(rows[idx]).to(d), rir, lengths, delays, host = host)
	out, partials = run(np.arange(B))
	out, partials = out.clone(), partials[:, :NPARTS].clone()
	perm = rng.permutation(B)
	moved, moved_partials = run(perm)
	assert torch.equal(moved, out[perm]) and torch.equal(moved_partials[:, :NPARTS], partials[perm])
	for b in (0, 3, 5, 6):  # alone in a batch of one
		alone, alone_partials = run(np.array([b]))
		assert torch.equal(alone[0], out[b]) and torch.equal(alone_partials[0, :NPARTS], partials[b])
	# a longer bank beside it (a larger workspace layout) changes nothing either
	_, rir2, lengths2, delays2, host2 = bank_tensors(hs + [make_rir('flat noise', 5 * BK, 3, rng)], d)
	wide, _ = ops.augment_reverb(torch.from_numpy(y_host).to(d), torch.from_numpy(make_params(out_len, T)).to(d), torch.from_numpy(rows).to(d), rir2, lengths2, delays2, host = host2)
	assert torch.equal(wide, out)
	torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ draws

def test_the_drawn_rows_equal_the_restatement_and_the_other_parameters_do_not_move():
	from convasr_amd import augment, ops
	d = dev()
	rng = np.random.default_rng(11)
	keys = np.concatenate([np.array([0, (1 << 40) + 1, 7, -1], dtype = np.int64), rng.integers(0, 1 << 50, 296)])
	dk = torch.from_numpy(keys).to(d)
	for p in (0.0, 0.5, 1.0):
		got = ops.reverb_params(dk, 77, 3, 11, ops.prob_threshold(p))
		assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.from_numpy(RR.rir_row(keys, 77, 3, 11, A.threshold(p))))
		assert torch.equal(got, ops.reverb_params(dk, 77, 3, 11, ops.prob_threshold(p)))
	half = ops.reverb_params(dk, 77, 3, 11, ops.prob_threshold(0.5)).cpu()
	assert 100 < int((half >= 0).sum()) < 200 and int(half.max()) == 10
	assert ops.reverb_params(dk[:0], 77, 3, 11, 0).shape == (0,)
	# the (B, 8) parameters and xlen_out of an augmenter with a bank are those of the same augmenter without one
	bank, lengths = augment.synthetic_rirs(5, 8000, rt60 = (0.01, 0.05))
	noise = torch.zeros(3, 500, device = d)
	xlen = torch.from_numpy(rng.uniform(0, 1, 300).astype(np.float32)).to(d)
	with_bank = augment.WaveformAugment(9, noise = noise, rir = bank.to(d), rir_lengths = lengths)
	without = augment.WaveformAugment(9, noise = noise)
	a, a_len = with_bank.params(xlen, dk, 4000, epoch = 2)
	b, b_len = without.params(xlen, dk, 4000, epoch = 2)
	assert set(a) == set(b) | {'rir_row'} and all(torch.equal(a[n], b[n]) for n in b) and torch.equal(a_len, b_len)
	assert torch.equal(a['rir_row'].cpu(), torch.from_numpy(RR.rir_row(keys, 9, 2, 5, A.threshold(0.5))))
	torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the whole augmenter: speed, gain, reverberation, noise

def test_the_noise_is_mixed_at_an_snr_relative_to_the_reverberated_speech():
	from convasr_amd import augment
	d = dev()
	rng = np.random.default_rng(12)
	B = 8
	keys = np.array([0, (1 << 40) + 1, 7, 123456789, 5, (1 << 33) + 9, 99, 31337], dtype = np.int64)
	xlen = np.float32([1.0, 0.85, 0.5, 0.0, 0.9, 0.3, 0.7, 0.95])
	x_host = rng.uniform(-0.5, 0.5, (B, T)).astype(np.float32)
	noise_host = rng.uniform(-0.5, 0.5, (3, 777)).astype(np.float32)
	hs = [make_rir('decaying noise', L, dd, rng) for L, dd in ((BK + 1, 0), (3 * BK + 5, 40), (300, 299))]
	bank, rir, _, _, host = bank_tensors(hs, d)
	x, noise, dx, dk = torch.from_numpy(x_host).to(d), torch.from_numpy(noise_host).to(d), torch.from_numpy(xlen).to(d), torch.from_numpy(keys).to(d)
	full = augment.WaveformAugment(21, noise = noise, noise_prob = 0.75, rir = rir, rir_lengths = host[0], reverb_prob = 0.6, normalize_rir = False)
	dry = augment.WaveformAugment(21)                       # speed and gain only: y
	no_rir = augment.WaveformAugment(21, noise = noise, noise_prob = 0.75)
	out, xlen_out, scales = full(x, dx, dk, epoch = 1, return_scales = True)
	out2, xlen_out2, scales2 = full(x, dx, dk, epoch = 1, return_scales = True)
	assert torch.equal(out, out2) and torch.equal(xlen_out, xlen_out2) and torch.equal(scales, scales2)
	y, y_len = dry(x, dx, dk, epoch = 1)
	plain, plain_len, plain_scales = no_rir(x, dx, dk, epoch = 1, return_scales = True)
	assert torch.equal(xlen_out, y_len) and torch.equal(xlen_out, plain_len)  # xlen_out is the bank-less value
	named, _ = full.params(dx, dk, T, epoch = 1)
	p = torch.stack([named[n] for n in A.FIELDS], dim = 1).cpu().numpy()
	rows = named['rir_row'].cpu().numpy()
	assert np.array_equal(rows, RR.rir_row(keys, 21, 1, 3, A.threshold(0.6))) and (rows >= 0).any() and (rows < 0).any()
	assert full.rir_host[1].tolist() == [0, 40, 299]
	y_host, got, got_scales = y.cpu().numpy(), out.cpu().numpy(), scales.cpu().numpy()
	snr_table = full.snr_table.numpy()
	mixed = 0
	for b in range(B):
		f = dict(zip(A.FIELDS, (int(v) for v in p[b])))
		if rows[b] < 0:  # no row: the bank-less augmenter's output, noise included, bit for bit
			assert torch.equal(out[b], plain[b]) and got_scales[b] == plain_scales[b].item(), b
			continue
		h, dd = hs[rows[b]], int(full.rir_host[1][rows[b]])
		z64 = RR.reverb_one(y_host[b], h, dd, f['out_len'])
		want = RR.scale(RR.partials(z64, noise_host, f), f, snr_table)
		assert abs(float(got_scales[b]) - want) <= float(np.spacing(np.float32(want))), (b, got_scales[b], want)  # 1 fp32 ulp
		extra = 0.0
		if f['noise_row'] >= 0 and f['out_len'] > 0:
			assert got_scales[b] > 0
			mixed += 1
			v = np.zeros(T)
			v[:f['out_len']] = float(got_scales[b]) * A.noise_window(noise_host, f, f['out_len'])
			extra = np.abs(v) * U
			# judge() compares with z64 alone: take the device's own noise term off in float64 first (the fma's rounding is `extra`)
			err = np.abs(got[b].astype(np.float64) - (z64 + v))
			e32 = e32_of(y_host[b], h, dd, f['out_len'], z64)
			assert e32 > 0 and (err <= 4 * e32 + extra).all(), (b, float(err.max()), e32)
		else:
			judge(got[b], y_host[b], h, dd, f['out_len'], ('mix', b))
		assert not got[b, f['out_len']:].any()
	assert mixed >= 2
	torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ guards

def test_envelope_violations_raise_and_launch_nothing():
	from convasr_amd import augment, ops, _lib
	d = dev()
	E = _lib.ConvasrHipError
	B, n = 2, 100
	y = torch.rand(B, n, device = d)
	params = torch.from_numpy(make_params(np.array([n, n]), n)).to(d)
	row = torch.zeros(B, dtype = torch.int64, device = d)
	rir = torch.ones(2, 40, device = d)
	i64 = lambda *v: torch.tensor(v, dtype = torch.int64)
	ok_len, ok_delay = i64(40, 3), i64(0, 2)
	call = lambda y = y, params = params, row = row, rir = rir, lens = ok_len, delays = ok_delay, **kw: ops.augment_reverb(y, params, row, rir, lens.to(d), delays.to(d), host = (lens, delays), **kw)
	out, _ = call()
	assert out.shape == (B, n)
	with pytest.raises(E, match = 'taps, outside'):
		call(lens = i64(0, 3))      # a length of 0
	with pytest.raises(E, match = 'taps, outside'):
		call(lens = i64(41, 3))     # a length above Lmax
	with pytest.raises(E, match = 'delay'):
		call(delays = i64(0, 3))    # a delay of rir_len
	with pytest.raises(E, match = 'delay'):
		call(delays = i64(-1, 0))
	big = torch.zeros(1, 32769, device = d)
	with pytest.raises(E, match = '> 32768'):
		ops.augment_reverb(y, params, row, big, i64(32769).to(d), i64(0).to(d), host = (i64(32769), i64(0)))
	edge, _ = ops.augment_reverb(y, params, row, big, i64(32768).to(d), i64(0).to(d), host = (i64(32768), i64(0)))  # 32,768 taps are inside
	assert not bool(edge.any())
	lib = _lib.load()
	dev_len, dev_delay, dev_partials, dev_ws = ok_len.to(d), ok_delay.to(d), torch.zeros(B * 64, dtype = torch.float64, device = d), torch.zeros(1 << 20, dtype = torch.uint8, device = d)
	null = lambda **kw: lib.convasr_augment_reverb(*[kw.get(k, v) for k, v in (('y', y.data_ptr()), ('B', B), ('T', n), ('params', params.data_ptr()), ('row', row.data_ptr()), ('rir', rir.data_ptr()), ('R', 2),
		('Lmax', 40), ('len', dev_len.data_ptr()), ('delay', dev_delay.data_ptr()), ('len_host', ok_len.data_ptr()), ('delay_host', ok_delay.data_ptr()), ('tw', ops.reverb_twiddles(d).data_ptr()),
		('noise', None), ('noise_rows', 0), ('noise_len', 0), ('out', out.data_ptr()), ('partials', dev_partials.data_ptr()),
		('ws', dev_ws.data_ptr()), ('ws_bytes', 1 << 20), ('stream', None))])
	EINVAL, EUNSUPPORTED = -1, -3
	torch.cuda.synchronize()
	assert null() == 0
	torch.cuda.synchronize()
	for name in ('y', 'params', 'row', 'rir', 'len', 'delay', 'len_host', 'delay_host', 'tw', 'out', 'partials', 'ws'):
		assert null(**{name: None}) == EINVAL, name
	assert null(R = 0) == EINVAL and null(Lmax = 0) == EINVAL and null(ws_bytes = 1000) == EINVAL and null(out = y.data_ptr()) == EINVAL
	assert null(B = 65536) == EUNSUPPORTED and null(T = 1 << 31) == EUNSUPPORTED
	assert null(B = 0) == 0 and null(T = 0) == 0 and null(B = 0, y = None, out = None) == 0
	assert lib.convasr_augment_reverb_params(row.data_ptr(), B, 1, 0, 1 << 31, 0, row.data_ptr(), None) == EUNSUPPORTED  # R < 2^31
	assert lib.convasr_augment_reverb_params(row.data_ptr(), B, 1, 0, 0, 0, row.data_ptr(), None) == EINVAL
	assert lib.convasr_augment_reverb_params(row.data_ptr(), 65536, 1, 0, 5, 0, row.data_ptr(), None) == EUNSUPPORTED
	assert lib.convasr_augment_reverb_params(None, B, 1, 0, 5, 0, row.data_ptr(), None) == EINVAL
	assert lib.convasr_augment_reverb_params(row.data_ptr(), B, 1, 1 << 32, 5, 0, row.data_ptr(), None) == EINVAL
	assert lib.convasr_augment_reverb_params(row.data_ptr(), B, 1, 0, 5, (1 << 24) + 1, row.data_ptr(), None) == EINVAL
	# a row outside the bank, and a bank whose device-side length or delay is out of range, read as "none": y comes back
	wild, _ = call(row = i64(-5, 2).to(d))
	assert torch.equal(wild, y)
	wild, _ = ops.augment_reverb(y, params, row, rir, i64(41, 3).to(d), i64(0, 2).to(d), host = (ok_len, ok_delay))
	assert torch.equal(wild, y)
	# empty batches launch nothing and keep their shapes
	e, ep = ops.augment_reverb(y[:0], params[:0], row[:0], rir, ok_len.to(d), ok_delay.to(d), host = (ok_len, ok_delay))
	assert e.shape == (0, n) and ep.shape[0] == 0
	# a CPU tensor is refused as elsewhere; so are a bank on another device and wrong types
	with pytest.raises(E, match = 'MI355X'):
		ops.augment_reverb(y.cpu(), params, row, rir, ok_len.to(d), ok_delay.to(d), host = (ok_len, ok_delay))
	with pytest.raises(E, match = 'MI355X'):
		ops.reverb_params(torch.zeros(2, dtype = torch.int64), 1, 0, 5, 0)
	with pytest.raises(E, match = 'lives on'):
		augment.WaveformAugment(1, rir = torch.ones(2, 40))(y, torch.ones(B, device = d), row)
	with pytest.raises(ValueError):
		ops.augment_reverb(y.double(), params, row, rir, ok_len.to(d), ok_delay.to(d), host = (ok_len, ok_delay))
	with pytest.raises(ValueError):
		ops.augment_reverb(y, params, row, rir, ok_len.to(d), ok_delay.to(d), host = (ok_len.to(d), ok_delay.to(d)))
	with pytest.raises(ValueError):
		ops.augment_waveform(y, params, rir = rir)
	torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ end to end

def test_reverberated_batches_feed_a_training_step_and_follow_seed_and_epoch():
	import convasr_amd as ca
	from convasr_amd import augment, datasets, train
	d = dev()
	ds = datasets.SyntheticAudioTextDataset(6, min_duration = 0.3, max_duration = 0.6, sample_rate = 8000)
	bank, lengths = augment.synthetic_rirs(7, 8000, rt60 = (0.05, 0.3), seed = 2)
	wave = augment.WaveformAugment(seed = 4, rir = bank.to(d), rir_lengths = lengths, reverb_prob = 0.5)
	order = [[0, 1, 2], [3, 4, 5]]
	run = lambda epoch: list(augment.batches(datasets.gpu_batches(ds, order, d), waveform = wave, epoch = epoch))
	first, again, other = run(0), run(0), run(1)
	assert all(torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) for a, b in zip(first, again))  # the same (seed, epoch) repeats
	keys = torch.arange(6, dtype = torch.int64, device = d)
	rows = [wave.params(torch.ones(6, device = d), keys, 4800, epoch = e)[0]['rir_row'].cpu() for e in (0, 1)]
	assert not torch.equal(rows[0], rows[1]) and bool((rows[0] >= 0).any()) and bool((rows[0] < 0).any())  # two epochs' rows differ
	assert not all(torch.equal(a[2], b[2]) for a, b in zip(first, other))
	plain = list(datasets.gpu_batches(ds, order, d))
	for (_, _, x, xlen, _, _), (_, _, px, pxlen, _, _), ids in zip(first, plain, order):
		assert x.shape == px.shape and x.dtype == torch.float32 and bool(torch.isfinite(x).all())
		for i, k in enumerate(ids):  # an utterance without a row differs from the reverberated one; all keep the padded shape
			assert (rows[0][k] >= 0) == (not torch.equal(x[i], augment.WaveformAugment(seed = 4)(px, pxlen, keys[ids])[0][i]))
	torch.manual_seed(0)
	fe = ca.models.LogFilterBankFrontend(64, 8000, 0.02, 0.01, 'hann_window')
	model = ca.models.Wav2Letter(64, [38], frontend = fe, dropout = 0, base_width = 64, check_time_dim_padded = False).to(d).train()
	opt = train.SGD(train.FlatParameters(model), lr = 1e-3, momentum = 0.9, weight_decay = 1e-3)
	meta, s, x, xlen, y, ylen = first[0]
	res = train.train_step(model, opt, x, xlen, y, ylen)
	torch.cuda.synchronize()
	assert math.isfinite(float(res['loss']))


def test_recorded_impulse_responses_are_read_and_resampled_into_a_bank(tmp_path):
	from convasr_amd import audio, augment
	d = dev()
	rng = np.random.default_rng(13)
	same = np.zeros(700, dtype = np.float32)
	same[5], same[6:] = 0.9, (rng.uniform(-0.2, 0.2, 694) * np.exp(-np.arange(694) / 150.0)).astype(np.float32)  # a direct path behind 5 samples of flight
	double = np.zeros((2, 1000), dtype = np.float32)  # two channels at twice the rate: mixed to mono and resampled to half as many taps
	double[:, 20] = 0.8
	paths = [audio.write_audio(str(tmp_path / 'a.wav'), torch.from_numpy(same)[None], 8000), audio.write_audio(str(tmp_path / 'b.wav'), torch.from_numpy(double), 16000)]
	bank, lengths = augment.load_rirs(paths, 8000)
	assert bank.dtype == torch.float32 and not bank.is_cuda and bank.shape == (2, 700) and lengths.tolist() == [700, 500]
	assert np.abs(bank[0].numpy() - same).max() <= 1.0 / 32767 and not bank[1, 500:].any()  # 16-bit PCM in between
	cut, cut_lengths = augment.load_rirs(paths, 8000, max_len = 600)
	assert cut.shape == (2, 600) and cut_lengths.tolist() == [600, 500] and torch.equal(cut[0], bank[0, :600])
	aug = augment.WaveformAugment(3, rir = bank.to(d), rir_lengths = lengths, reverb_prob = 1.0)
	assert aug.rir_host[1].tolist() == [5, 10]  # the direct paths: tap 5, and tap 20 of the 16 kHz file at half the rate
	x = torch.from_numpy(rng.uniform(-0.5, 0.5, (2, 3000)).astype(np.float32)).to(d)
	out, xlen = aug(x, torch.ones(2, device = d), torch.arange(2, dtype = torch.int64, device = d))
	assert out.shape == x.shape and bool(torch.isfinite(out).all()) and not torch.equal(out, x)
	with pytest.raises(ValueError):
		augment.load_rirs([], 8000)
	torch.cuda.synchronize()
