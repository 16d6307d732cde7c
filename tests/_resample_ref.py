"""float64 numpy restatement of the resampler that include/convasr_hip.h defines (convasr_resample): the direct sum, no coefficient table.

    g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g, T_out = ceil(T_in L / M), s = rolloff min(1, L / M); output n at tau = n M / L:
    y[n] = s sum_k x[k] sinc(s (k - tau)) w((k - tau) s / Z)   over the integers k with |k - tau| s <= Z, x[k] = 0 outside [0, T_in)
    sinc(u) = sin(pi u) / (pi u),  w(v) = I0(beta sqrt(1 - v^2)) / I0(beta) for |v| <= 1, otherwise 0

k - tau is formed as the exact integer L k - n M over L (one rounding).  I0 is its own power series here (the product's host table uses numpy's
i0), the sine is taken of the argument reduced by the integer nearest to it.  The resampler is this project's, unpinned against librosa."""
import math

import numpy as np

ZEROS, BETA, ROLLOFF = 64, 14.769656459379492, 0.9475937167399596  # the parameters resampy publishes for 'kaiser_best'


def bessel_i0(x):
	"""I0(x) = sum_m ((x / 2)^2m) / (m!)^2, float64, for 0 <= x <= 16 (at x = 16 the term m = 45 is below 1e-30 of the sum)."""
	q = np.asarray(x, dtype = np.float64) ** 2 / 4
	term, total = np.ones_like(q), np.ones_like(q)
	for m in range(1, 46):
		term = term * q / (m * m)
		total = total + term
	return total


def sinc(u):
	"""sin(pi u) / (pi u) with the sine of the reduced argument: sin(pi u) = (-1)^r sin(pi (u - r)), r = round(u)."""
	u = np.asarray(u, dtype = np.float64)
	r = np.rint(u)
	num = np.where(r.astype(np.int64) % 2 == 0, 1.0, -1.0) * np.sin(np.pi * (u - r))
	safe = np.where(u == 0, 1.0, u)
	return np.where(u == 0, 1.0, num / (np.pi * safe))


def ratio(sr_in, sr_out):
	g = math.gcd(int(sr_in), int(sr_out))
	return int(sr_out) // g, int(sr_in) // g


def out_len(T_in, sr_in, sr_out):
	L, M = ratio(sr_in, sr_out)
	return -(-int(T_in) * L // M)


def filter_scale(sr_in, sr_out, rolloff = ROLLOFF):
	L, M = ratio(sr_in, sr_out)
	return rolloff * min(1.0, L / M)


def resample(x, sr_in, sr_out, zeros = ZEROS, beta = BETA, rolloff = ROLLOFF):
	"""x (C, T_in) -> (y (C, T_out) float64, n_k (T_out,) taps with k inside [0, T_in), A (C, T_out) = s sum_k |x[k] h[k]|), the two that the
	fp32 error bound of the kernel is made of.  Equal rates: y = x, n_k = 0, A = |x|."""
	x = np.atleast_2d(np.asarray(x, dtype = np.float64))
	C, T_in = x.shape
	L, M = ratio(sr_in, sr_out)
	if L == M:
		return x.copy(), np.zeros(T_in, dtype = np.int64), np.abs(x)
	T_out = out_len(T_in, sr_in, sr_out)
	s = filter_scale(sr_in, sr_out, rolloff)
	half = int(zeros / s) + 2  # more than enough integers on either side of tau
	y, A, n_k = np.zeros((C, T_out)), np.zeros((C, T_out)), np.zeros(T_out, dtype = np.int64)
	i0_beta = float(bessel_i0(beta))
	offs = np.arange(-half, half + 1, dtype = np.int64)
	block = 2048
	for lo in range(0, T_out, block):
		n = np.arange(lo, min(lo + block, T_out), dtype = np.int64)
		k = (n * M // L)[:, None] + offs[None, :]                          # (n, j) candidate inputs
		d = (L * k - (n * M)[:, None]) / float(L)                           # k - tau
		inside = (np.abs(d) * s <= zeros) & (k >= 0) & (k < T_in)
		v = np.clip(d * s / zeros, -1.0, 1.0)
		h = np.where(inside, sinc(s * d) * bessel_i0(beta * np.sqrt(1.0 - v * v)) / i0_beta, 0.0)
		xk = x[:, np.clip(k, 0, max(T_in - 1, 0))] if T_in else np.zeros((C, ) + k.shape)
		y[:, n] = s * (xk * h[None]).sum(-1)
		A[:, n] = s * np.abs(xk * h[None]).sum(-1)
		n_k[n] = inside.sum(-1)
	return y, n_k, A


def decode_int16(pcm):
	"""(T, C) int16 -> (C, T) float32 by s2f_numpy (audio.py:15): a float32 divide by 32767."""
	return np.divide(np.asarray(pcm).T, np.float32(32767), dtype = 'float32')


def mono_mean(x32):
	"""The fp32 mean over channels as the kernel takes it: the sum in ascending channel order, divided by C, both in float32."""
	x32 = np.asarray(x32, dtype = np.float32)
	total = x32[0].copy()
	for c in range(1, x32.shape[0]):
		total = total + x32[c]
	return (total / np.float32(x32.shape[0]))[None]
