"""The float64 restatement of the resampler (tests/_resample_ref.py) checked on the CPU, and the product's host coefficient table against it.

The resampler is defined by this project and unpinned against librosa; scipy.signal.resample_poly, the independent implementation that is
installed, has the same length rule and timing with a different filter and serves as a check of the alignment only."""
import numpy as np
import pytest

import _resample_ref as R

RATIOS = [(8000, 16000), (16000, 8000), (48000, 16000), (44100, 16000), (8000, 11025)]


def tones(sr, T, freqs, amps = (0.6, 0.35)):
	t = np.arange(T, dtype = np.float64) / sr
	return sum(a * np.sin(2 * np.pi * f * t + 0.3 + i) for i, (a, f) in enumerate(zip(amps, freqs)))


def interior(sr_in, sr_out, T_out):
	"""Outputs further than Z / s input samples from both ends of the signal (where the filter's support is cut)."""
	skip = int(np.ceil(R.ZEROS / R.filter_scale(sr_in, sr_out) * max(1.0, sr_out / sr_in))) + 2
	assert T_out > 2 * skip + 100
	return slice(skip, T_out - skip)


@pytest.mark.parametrize('sr_in,sr_out', RATIOS)
@pytest.mark.parametrize('fractions', [(0.11, 0.43), (0.05, 0.7), (0.29, 0.61)])
def test_tones_below_both_nyquist_limits_come_out_as_the_same_tones_at_the_new_rate(sr_in, sr_out, fractions):
	"""Within 1e-6 on the interior: 100 x the 1.1e-8 measured on two-tone signals (the stop-band ripple of the 'kaiser_best' window)."""
	nyquist = min(sr_in, sr_out) / 2
	freqs = [f * nyquist for f in fractions]
	T_in = int(3000 * max(1.0, sr_in / sr_out))
	y, n_k, A = R.resample(tones(sr_in, T_in, freqs)[None], sr_in, sr_out)
	T_out = y.shape[1]
	inner = interior(sr_in, sr_out, T_out)
	err = np.abs(y[0] - tones(sr_out, T_out, freqs))[inner].max()
	print(f'{sr_in} -> {sr_out} tones at {fractions} of the lower Nyquist limit: max interior error {err:.3e}')
	assert err <= 1e-6
	assert int(n_k[inner].min()) >= int(2 * R.ZEROS / R.filter_scale(sr_in, sr_out)) - 1 and (A >= np.abs(y) - 1e-15).all()


def test_length_rule():
	for sr_in, sr_out in RATIOS + [(16000, 16000), (11025, 8000), (7, 3)]:
		L, M = R.ratio(sr_in, sr_out)
		for T_in in (0, 1, 2, 63, 64, 65, 1000, 4097):
			T_out = R.out_len(T_in, sr_in, sr_out)
			assert T_out == int(np.ceil(T_in * sr_out / sr_in)) and (T_out - 1) * M < T_in * L <= T_out * M + M * (T_in == 0)
			assert R.resample(np.zeros((1, T_in)), sr_in, sr_out)[0].shape == (1, T_out)


def test_equal_rates_are_the_identity():
	x = np.random.default_rng(0).uniform(-1, 1, (2, 257))
	y, n_k, A = R.resample(x, 16000, 16000)
	assert np.array_equal(y, x) and np.array_equal(A, np.abs(x))


@pytest.mark.parametrize('sr_in,sr_out', RATIOS)
def test_linearity_and_the_mono_mix_commute_with_the_filter(sr_in, sr_out):
	rng = np.random.default_rng(sr_in + sr_out)
	x = rng.uniform(-1, 1, (3, 700))
	y = R.resample(x, sr_in, sr_out)[0]
	combo = R.resample((0.5 * x[0] - 2.0 * x[1] + 0.25 * x[2])[None], sr_in, sr_out)[0][0]
	assert np.abs(combo - (0.5 * y[0] - 2.0 * y[1] + 0.25 * y[2])).max() <= 1e-12
	assert np.abs(R.resample(x.mean(0, keepdims = True), sr_in, sr_out)[0] - y.mean(0, keepdims = True)).max() <= 1e-12


@pytest.mark.parametrize('sr_in,sr_out', [(8000, 16000), (8000, 11025)])
def test_zero_delay_against_resample_poly(sr_in, sr_out):
	"""A sanity check of the alignment, not a parity claim: the same timing and length, another filter (measured 1.6e-3 / 1.8e-3)."""
	import scipy.signal
	L, M = R.ratio(sr_in, sr_out)
	x = tones(sr_in, 3000, [0.11 * sr_in / 2, 0.43 * sr_in / 2])
	y = R.resample(x[None], sr_in, sr_out)[0][0]
	z = scipy.signal.resample_poly(x, L, M)
	assert z.shape == y.shape
	diff = np.abs(y - z)[interior(sr_in, sr_out, len(y))].max()
	print(f'{sr_in} -> {sr_out}: max interior difference from resample_poly {diff:.3e}')
	assert diff <= 5e-3


@pytest.mark.parametrize('sr_in,sr_out', RATIOS + [(48000, 1000)])
def test_the_host_table_holds_the_filter_of_the_restatement(sr_in, sr_out):
	"""ops.resample_table (float64 on the host, rounded to fp32 once): entry (j, p) is the response of output n to a unit impulse at input
	k0 - H + j, for every phase p = (n M) mod L -- within one fp32 rounding of the restatement's value (2^-24 relative; the two Bessel
	evaluations and the two sines differ by parts in 1e-16 of a coefficient of at most 1)."""
	from convasr_amd import ops
	table = ops.resample_table(sr_in, sr_out).numpy().astype(np.float64)
	taps, L = table.shape
	L_, M = R.ratio(sr_in, sr_out)
	assert L == L_ and taps == 2 * int(R.ZEROS / R.filter_scale(sr_in, sr_out)) + 2
	H = taps // 2 - 1
	n0 = -(-(H + 2) * L // M)  # the first output whose window starts inside the signal
	for n in sorted({n0, n0 + 1, n0 + L // 2, n0 + L - 1}):
		k0, p = n * M // L, n * M % L
		T_in = k0 + H + 3
		for j in (0, 1, H - 1, H, H + 1, H + 2, taps - 2, taps - 1):
			x = np.zeros((1, T_in))
			x[0, k0 - H + j] = 1.0
			want = R.resample(x, sr_in, sr_out)[0][0, n]
			assert abs(table[j, p] - want) <= 2.0 ** -24 * abs(want) + 1e-14, (n, j, p, table[j, p], want)
	# and nothing of the filter lies outside the table: every phase sums to the DC gain 1 within the stop-band ripple
	assert np.abs(table.sum(0) - 1.0).max() <= 1e-5
