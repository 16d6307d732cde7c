"""numpy restatement of the training-time augmentation that include/convasr_hip.h defines (convasr_philox, convasr_augment_params,
convasr_augment_waveform, convasr_augment_mix, convasr_spec_augment): every integer exact, every sample in float64.  The augmentation is this
project's own, unpinned against torchaudio, NeMo or Kaldi.

    decision(seed, epoch, key, purpose, index) = word 0 of Philox4x32-10(counter = (key lo, key hi, epoch, purpose << 16 | index), key = (seed lo, seed hi))
    fires(r, p) = (r >> 8) < floor(p 2^24);   uniform integer in [0, n] = ((r >> 8) (n + 1)) >> 24

The filter here is evaluated from its definition with _resample_ref's own I0 series and reduced-argument sinc (the product's host table uses
numpy's i0 and sinc)."""
import math

import numpy as np

import _resample_ref as R

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)
ONE = 1 << 32
PHASES, PBITS = 128, 7
FIELDS = ('speed', 'step', 'gain', 'noise_row', 'noise_offset', 'snr', 'len', 'out_len')
SPEED_FIRE, SPEED, GAIN_FIRE, GAIN, NOISE_FIRE, NOISE_ROW, NOISE_OFFSET, SNR, FREQ_WIDTH, FREQ_START, TIME_WIDTH, TIME_START = range(12)
U = 2.0 ** -24  # one fp32 rounding, relative


def philox(counters, key):
	"""counters (N, 4) and key (2,) of 32-bit words (any integer type) -> (N, 4) uint64 holding the four output words: plain integer arithmetic."""
	c = [np.asarray(counters)[:, i].astype(np.uint64) & MASK for i in range(4)]
	k0, k1 = np.uint64(int(key[0]) & 0xffffffff), np.uint64(int(key[1]) & 0xffffffff)
	for _ in range(10):
		p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 -> 64 bits: no overflow
		c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
		k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
	return np.stack(c, axis = 1)


def draw(seed, epoch, keys, purpose, index = 0):
	"""The random word of every key: (N,) uint64 below 2^32."""
	keys = np.atleast_1d(np.asarray(keys, dtype = np.int64)).astype(np.uint64)
	ctr = np.stack([keys & MASK, keys >> np.uint64(32), np.full_like(keys, int(epoch)), np.full_like(keys, (int(purpose) << 16) | int(index))], axis = 1)
	seed = int(seed) & 0xffffffffffffffff
	return philox(ctr, (seed & 0xffffffff, seed >> 32))[:, 0]


def uint(r, n):
	"""Uniform integer in [0, n] per word: ((r >> 8) (n + 1)) >> 24, n < 2^40 (Python integers where n is an array of them)."""
	top = (np.asarray(r, dtype = np.uint64) >> np.uint64(8))
	return ((top * (np.asarray(n, dtype = np.int64).astype(np.uint64) + np.uint64(1))) >> np.uint64(24)).astype(np.int64)


def threshold(p):
	return int(math.floor(float(p) * (1 << 24)))


def fires(r, thr):
	return (np.asarray(r, dtype = np.uint64) >> np.uint64(8)) < np.uint64(thr)


def steps(speeds):
	return [int(math.floor(float(s) * ONE + 0.5)) for s in speeds]


def valid_len(xlen, T):
	"""ceil(xlen T) in fp32 (ops.output_lengths' rule), clamped to [0, T]."""
	v = np.ceil(np.asarray(xlen, dtype = np.float32) * np.float32(T)).astype(np.int64)
	return np.clip(v, 0, int(T))


def params(xlen, keys, T, seed, epoch, step_table, speed_thr = 1 << 24, gain_steps = 0, gain_thr = 0, noise_shape = None, snr_steps = 1, noise_thr = 0, min_out_len = None):
	"""(params (B, 8) int64 with the columns FIELDS, xlen_out (B,) float32)."""
	keys = np.asarray(keys, dtype = np.int64)
	B, T = len(keys), int(T)
	length = valid_len(xlen, T)
	speed = uint(draw(seed, epoch, keys, SPEED), len(step_table) - 1)
	step = np.array([step_table[i] for i in speed], dtype = object)
	out_len = np.array([(int(l) << 32) // int(s) for l, s in zip(length, step)], dtype = np.int64)
	keep = ~fires(draw(seed, epoch, keys, SPEED_FIRE), speed_thr) | (out_len > T)
	if min_out_len is not None:
		keep |= out_len < np.asarray(min_out_len, dtype = np.int64)
	speed = np.where(keep, -1, speed)
	step = np.where(keep, ONE, step).astype(np.int64)
	out_len = np.where(keep, length, out_len)
	gain = np.full(B, -1, dtype = np.int64)
	if gain_steps > 0:
		gain = np.where(fires(draw(seed, epoch, keys, GAIN_FIRE), gain_thr), uint(draw(seed, epoch, keys, GAIN), gain_steps - 1), -1)
	row, offset, snr = np.full(B, -1, dtype = np.int64), np.zeros(B, dtype = np.int64), np.zeros(B, dtype = np.int64)
	if noise_shape is not None:
		on = fires(draw(seed, epoch, keys, NOISE_FIRE), noise_thr)
		row = np.where(on, uint(draw(seed, epoch, keys, NOISE_ROW), noise_shape[0] - 1), -1)
		offset = np.where(on, uint(draw(seed, epoch, keys, NOISE_OFFSET), noise_shape[1] - 1), 0)
		snr = np.where(on, uint(draw(seed, epoch, keys, SNR), snr_steps - 1), 0)
	p = np.stack([speed, step, gain, row, offset, snr, length, out_len], axis = 1).astype(np.int64)
	return p, (out_len.astype(np.float32) / np.float32(T)) if T > 0 else np.asarray(xlen, dtype = np.float32)


def cutoff(step, rolloff = R.ROLLOFF):
	return rolloff * min(1.0, ONE / step)


def taps_for(step_table, zeros = R.ZEROS, rolloff = R.ROLLOFF):
	if all(s == ONE for s in step_table):
		return 0
	return 2 * int(math.floor(zeros / min(cutoff(s, rolloff) for s in step_table))) + 2


def filt(d, c, zeros = R.ZEROS, beta = R.BETA):
	"""h(d) = c sinc(c d) w(d c / Z) where |d| c <= Z, else 0: the continuous-phase filter in float64."""
	d = np.asarray(d, dtype = np.float64)
	v = np.clip(d * c / zeros, -1.0, 1.0)
	return np.where(np.abs(d) * c <= zeros, c * R.sinc(c * d) * R.bessel_i0(beta * np.sqrt(1.0 - v * v)) / float(R.bessel_i0(beta)), 0.0)


def table(step_table):
	"""(n_speeds, taps, PHASES + 1) float32: table[i][j][p] = h_i((j - H) - p / PHASES), rounded once."""
	taps = taps_for(step_table)
	H = taps // 2 - 1
	d = (np.arange(taps, dtype = np.float64)[:, None] - H) - np.arange(PHASES + 1, dtype = np.float64)[None, :] / PHASES
	return np.stack([filt(d, cutoff(s)).astype(np.float32) for s in step_table])


def positions(n, step):
	"""Output n sits at n step / 2^32: (k0, phase, f) = the integer part, the tabulated phase below and the 24-bit fraction between it and the next."""
	pos = np.asarray(n, dtype = np.uint64) * np.uint64(step)  # n < 2^31, step <= 2^33: below 2^64
	frac = pos & MASK
	sub = ((frac << np.uint64(PBITS)) & MASK) >> np.uint64(8)
	return (pos >> np.uint64(32)).astype(np.int64), (frac >> np.uint64(32 - PBITS)).astype(np.int64), sub.astype(np.float64) * U


def decode(x):
	"""int16 -> float32 by a correctly rounded divide by 32767; float32 stays."""
	x = np.asarray(x)
	return np.divide(x, np.float32(32767), dtype = 'float32') if x.dtype == np.int16 else x.astype(np.float32)


def speed_one(x32, length, out_len, step, tab32, continuous = None):
	"""One utterance through the speed filter in float64: (y (out_len,), A (out_len,) = sum_j |x_j| max(|t0_j|, |t1_j|)).  tab32: (taps, PHASES + 1), the
	tabulated filter, interpolated linearly as the kernel does; continuous = the cutoff: the filter from its definition at the exact position."""
	x = np.asarray(x32, dtype = np.float64)
	n = np.arange(out_len, dtype = np.int64)
	if step == ONE:
		return x[:out_len].copy(), np.abs(x[:out_len])
	taps = tab32.shape[0]
	H = taps // 2 - 1
	k0, ph, f = positions(n, step)
	k = k0[:, None] - H + np.arange(taps, dtype = np.int64)[None, :]
	xk = np.where((k >= 0) & (k < length), x[np.clip(k, 0, max(len(x) - 1, 0))] if len(x) else 0.0, 0.0)
	j = np.arange(taps)[None, :]
	t0, t1 = tab32[j, ph[:, None]].astype(np.float64), tab32[j, ph[:, None] + 1].astype(np.float64)
	if continuous is not None:
		c = filt((k - k0[:, None]) - ((ph + f) / PHASES)[:, None], continuous)  # k - position, exact: a small integer minus the 32-bit fraction
	else:
		c = t0 + f[:, None] * (t1 - t0)
	return (xk * c).sum(-1), (np.abs(xk) * np.maximum(np.abs(t0), np.abs(t1))).sum(-1)


def waveform(x, p, tab32 = None, gain_table = None, noise = None, scales = None):
	"""The waveform pass and the mix given the parameters (B, 8) and -- for the mix -- the (B,) scales: (y (B, T) float64, A (B, T)); the kernel's fp32
	result lies within (taps + 6) 2^-24 A of y (tests/test_augment_gpu.py derives it)."""
	x32 = decode(x)
	B, T = x32.shape
	y, A = np.zeros((B, T)), np.zeros((B, T))
	for b in range(B):
		f = dict(zip(FIELDS, (int(v) for v in p[b])))
		yb, Ab = speed_one(x32[b], f['len'], f['out_len'], f['step'], None if f['speed'] < 0 else tab32[f['speed']])
		if f['gain'] >= 0:
			g = float(gain_table[f['gain']])
			yb, Ab = yb * g, Ab * g
		if noise is not None and f['noise_row'] >= 0 and scales is not None and float(scales[b]) != 0.0:
			v = noise_window(noise, f, f['out_len'])
			yb, Ab = yb + float(scales[b]) * v, Ab + np.abs(float(scales[b]) * v)
		y[b, :f['out_len']], A[b, :f['out_len']] = yb, Ab
	return y, A


def noise_window(noise, f, count):
	L = noise.shape[1]
	return np.asarray(noise[f['noise_row']], dtype = np.float64)[(f['noise_offset'] + np.arange(count, dtype = np.int64)) % L]


def noise_scale(y, noise, f, snr_table):
	"""table[snr] sqrt(Ex / En) in float64 over the out_len valid samples; 0 without a row or when either energy is 0."""
	if f['noise_row'] < 0:
		return 0.0
	ex, en = float((np.asarray(y[:f['out_len']], dtype = np.float64) ** 2).sum()), float((noise_window(noise, f, f['out_len']) ** 2).sum())
	return float(snr_table[f['snr']]) * math.sqrt(ex / en) if ex > 0 and en > 0 else 0.0


def db_table(lo, hi, n, sign = 1.0):
	db = np.linspace(float(lo), float(hi), int(n), dtype = np.float64) if n > 1 else np.full(int(n), float(lo))
	return (10.0 ** (sign * db / 20.0)).astype(np.float32)


def spec_masks(keys, epoch, seed, F, valid, freq_masks, freq_width, time_masks, time_width, time_fraction):
	"""(B, freq_masks + time_masks, 2) int64 (start, width), frequency masks first."""
	keys, valid = np.asarray(keys, dtype = np.int64), np.asarray(valid, dtype = np.int64)
	out = np.zeros((len(keys), freq_masks + time_masks, 2), dtype = np.int64)
	for i in range(freq_masks):
		w = uint(draw(seed, epoch, keys, FREQ_WIDTH, i), np.full(len(keys), min(freq_width, F)))
		out[:, i, 0], out[:, i, 1] = uint(draw(seed, epoch, keys, FREQ_START, i), F - w), w
	limit = np.minimum(time_width, (valid * threshold(time_fraction)) >> 24)
	for i in range(time_masks):
		w = uint(draw(seed, epoch, keys, TIME_WIDTH, i), limit)
		out[:, freq_masks + i, 0], out[:, freq_masks + i, 1] = uint(draw(seed, epoch, keys, TIME_START, i), valid - w), w
	return out


def spec_covered(masks, freq_masks, F, T, valid):
	"""(B, F, T) bool: the cells a mask covers, inside the valid frames only."""
	B = len(masks)
	m = np.zeros((B, F, T), dtype = bool)
	for b in range(B):
		for i, (s, w) in enumerate(masks[b]):
			if i < freq_masks:
				m[b, s:s + w, :] = True
			else:
				m[b, :, s:s + w] = True
		m[b, :, int(valid[b]):] = False
	return m


def spec_mean(x, valid):
	"""The float64 mean of every utterance over all channels and its valid frames (0 without any)."""
	return np.array([np.asarray(x[b][:, :int(v)], dtype = np.float64).mean() if v > 0 and x.shape[1] > 0 else 0.0 for b, v in enumerate(valid)])


def spec_augment(x, masks, freq_masks, valid, fill):
	"""fill (B,) float32 -> the masked features, float32, everything else copied."""
	x = np.asarray(x, dtype = np.float32)
	return np.where(spec_covered(masks, freq_masks, x.shape[1], x.shape[2], valid), np.asarray(fill, dtype = np.float32)[:, None, None], x)
