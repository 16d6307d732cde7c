"""float64 numpy restatement of the room reverberation that include/convasr_hip.h defines (convasr_augment_reverb_params, convasr_augment_reverb):
the two draws, the direct convolution, the shift by the direct-path delay, the cut at out_len and the energies the mix reads.  It reuses the
generator of tests/_augment_ref.py and shares no code with the package.  Checked on the CPU by tests/test_reverb_ref.py.

    rir_row = uniform in [0, R - 1] (purpose 13) when purpose 12 fires, else -1
    z[n] = sum over k < rir_len[r] of h_r[k] y[n + d_r - k] for n < out_len, y = 0 outside [0, out_len);  z[n] = 0 for out_len <= n < T"""
import numpy as np

import _augment_ref as A

REVERB_FIRE, REVERB_ROW = 12, 13
TILE, PARTS = 1024, 32  # convasr_augment_tile(), convasr_augment_parts()


def rir_row(keys, seed, epoch, rows, thr):
	"""(B,) int64: the drawn row of every key, -1 = none."""
	keys = np.asarray(keys, dtype = np.int64)
	on = A.fires(A.draw(seed, epoch, keys, REVERB_FIRE), thr)
	return np.where(on, A.uint(A.draw(seed, epoch, keys, REVERB_ROW), int(rows) - 1), -1).astype(np.int64)


def delay(h, length):
	"""The index of the first largest |h[k]|, k < length."""
	return int(np.argmax(np.abs(np.asarray(h, dtype = np.float64)[:int(length)])))


def normalize(bank, lengths):
	"""Every row scaled to unit energy in float64, rounded once to float32; nothing behind a row's length survives."""
	bank = np.asarray(bank, dtype = np.float64) * (np.arange(np.shape(bank)[1])[None, :] < np.asarray(lengths)[:, None])
	energy = (bank * bank).sum(axis = 1, keepdims = True)
	return (bank / np.where(energy > 0, np.sqrt(energy), 1.0)).astype(np.float32)


def reverb_one(y, h, d, out_len):
	"""One utterance: y (T,), h (rir_len,) -> z (T,) float64.  np.convolve is the direct sum: full[i] = sum_k h[k] y[i - k]."""
	y = np.asarray(y, dtype = np.float64)
	z = np.zeros(len(y))
	if out_len > 0:
		full = np.convolve(y[:out_len], np.asarray(h, dtype = np.float64))  # (out_len + rir_len - 1,)
		z[:out_len] = full[d:d + out_len]                                    # d < rir_len: the slice is whole
	return z


def reverb(y, out_len, rows, bank, lengths, delays):
	"""The batch: y (B, T) float32, out_len and rows (B,), bank (R, Lmax), lengths and delays (R,) -> z (B, T) float64.  A row of -1 (or outside
	the bank) copies y below out_len; everything behind out_len is 0 either way."""
	y = np.asarray(y)
	z = y.astype(np.float64)
	for b in range(y.shape[0]):
		r = int(rows[b])
		if 0 <= r < len(bank):
			z[b] = reverb_one(y[b], bank[r][:int(lengths[r])], int(delays[r]), int(out_len[b]))
		z[b, int(out_len[b]):] = 0.0
	return z


def partials(z, noise, fields):
	"""(PARTS, 2) float64 of one utterance: part p owns the tiles p, p + nparts, ... of TILE outputs (nparts = min(tiles, PARTS)) and holds (sum z^2,
	sum v^2) over its outputs n < out_len; the parts beyond nparts stay 0 (the mix does not read them)."""
	T, out_len = len(z), fields['out_len']
	ntiles = -(-T // TILE)
	nparts = min(ntiles, PARTS)
	v = A.noise_window(noise, fields, out_len) if noise is not None and fields['noise_row'] >= 0 else np.zeros(out_len)
	p = np.zeros((PARTS, 2))
	for tile in range(ntiles):
		lo, hi = tile * TILE, min((tile + 1) * TILE, out_len)
		if hi > lo:
			p[tile % nparts, 0] += float((np.asarray(z[lo:hi], dtype = np.float64) ** 2).sum())
			p[tile % nparts, 1] += float((v[lo:hi] ** 2).sum())
	return p


def scale(p, fields, snr_table):
	"""convasr_augment_mix's factor from the partial pairs added in index order."""
	if fields['noise_row'] < 0:
		return 0.0
	ex, en = 0.0, 0.0
	for q in range(len(p)):
		ex, en = ex + p[q, 0], en + p[q, 1]
	return float(snr_table[fields['snr']]) * float(np.sqrt(ex / en)) if ex > 0 and en > 0 else 0.0
