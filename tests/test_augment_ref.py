"""The augmentation's rule on the CPU (include/convasr_hip.h: convasr_philox, convasr_augment_params, convasr_augment_waveform): the numpy
restatement the kernels are held to (tests/_augment_ref.py) against known answers, its own statistics, and the continuous-phase filter.  No GPU.
The augmentation is this project's own, unpinned against any outside library."""
import numpy as np

import _augment_ref as A
import _resample_ref as R


def words(*hexes):
	return np.array([[int(h, 16) for h in hexes]], dtype = np.uint64)


def test_philox_reproduces_the_random123_known_answers():
	"""Random123's kat_vectors for philox4x32-10: zeros, all ones, and the digits of pi."""
	assert np.array_equal(A.philox(words('0', '0', '0', '0'), (0, 0)), words('6627e8d5', 'e169c58d', 'bc57ac4c', '9b00dbd8'))
	assert np.array_equal(A.philox(words('ffffffff', 'ffffffff', 'ffffffff', 'ffffffff'), (0xffffffff, 0xffffffff)), words('408f276d', '41c83b0e', 'a20bc7c6', '6d5451fd'))
	assert np.array_equal(A.philox(words('243f6a88', '85a308d3', '13198a2e', '03707344'), (0xa4093822, 0x299f31d0)), words('d16cfe09', '94fdcceb', '5001e420', '24126ea1'))


def test_a_half_probability_draw_fires_for_about_half_of_4096_keys():
	"""Binomial(4096, 0.5): sigma = 32 = 0.0078 of 4096, so [0.45, 0.55] is 6 sigma wide on either side; the seed is fixed, so the share is one number."""
	share = A.fires(A.draw(1234, 0, np.arange(4096), A.NOISE_FIRE), A.threshold(0.5)).mean()
	assert 0.45 <= share <= 0.55, share
	assert not A.fires(A.draw(1234, 0, np.arange(4096), A.NOISE_FIRE), A.threshold(0.0)).any()
	assert A.fires(A.draw(1234, 0, np.arange(4096), A.NOISE_FIRE), A.threshold(1.0)).all()


def test_integer_draws_cover_the_closed_range_and_never_leave_it():
	r = np.concatenate([np.array([0, 0xff, 0x100, 0x7fffffff, 0x80000000, 0xffffff00, 0xffffffff], dtype = np.uint64), A.draw(7, 3, np.arange(4096), A.GAIN)])
	for n in (0, 1, (1 << 24) - 1):
		v = A.uint(r, np.full(len(r), n))
		assert v.min() == 0 and v.max() == n, (n, v.min(), v.max())  # (word 0 gives 0, the all-ones word gives n)
	assert set(A.uint(r, np.full(len(r), 1)).tolist()) == {0, 1}
	# with n = 2^24 - 1 the draw is the word's top 24 bits scaled by 2^24 / 2^24: every value is reachable and the map is monotone
	top = np.arange(0, 1 << 24, 4099, dtype = np.uint64)
	assert np.array_equal(A.uint(top << np.uint64(8), np.full(len(top), (1 << 24) - 1)), top.astype(np.int64))


def test_the_parameters_of_a_key_do_not_depend_on_the_rest_of_the_call():
	rng = np.random.default_rng(0)
	keys = np.concatenate([[0, (1 << 40) + 1], rng.integers(0, 1 << 50, 30)])
	xlen = rng.uniform(0.3, 1.0, len(keys)).astype(np.float32)
	kw = dict(T = 4000, seed = 99, step_table = A.steps((0.9, 1.0, 1.1)), gain_steps = 64, gain_thr = A.threshold(1.0), noise_shape = (5, 777), snr_steps = 64, noise_thr = A.threshold(0.5))
	full, full_len = A.params(xlen, keys, epoch = 2, **kw)
	for b in (0, 1, 17):
		one, one_len = A.params(xlen[b:b + 1], keys[b:b + 1], epoch = 2, **kw)
		assert np.array_equal(one[0], full[b]) and one_len[0] == full_len[b]
	perm = rng.permutation(len(keys))
	assert np.array_equal(A.params(xlen[perm], keys[perm], epoch = 2, **kw)[0], full[perm])
	assert not np.array_equal(A.params(xlen, keys, epoch = 3, **kw)[0], full)
	assert set(full[:, 0].tolist()) <= {-1, 0, 1, 2} and (full[:, 3] >= -1).all() and (full[:, 3] < 5).all() and (full[:, 4] < 777).all()


def test_output_lengths_are_floor_of_len_over_speed_and_the_fallbacks_are_exact():
	for speed, want in ((0.9, 1111), (1.1, 909)):
		p, xl = A.params(np.float32([1000 / 2048]), [5], 2048, 1, 0, A.steps((speed, )))
		assert p[0, 6] == 1000 and p[0, 7] == want and p[0, 0] == 0, p
		assert xl[0] == np.float32(want) / np.float32(2048)
	# 0.9 x 1000 samples does not fit T = 1110 (1111 > 1110) but fits 1111; min_out_len = 910 refuses 1.1 (909 < 910), 909 accepts it
	assert A.params(np.float32([1000 / 1110]), [5], 1110, 1, 0, A.steps((0.9, )))[0][0].tolist() == [-1, A.ONE, -1, -1, 0, 0, 1000, 1000]
	assert A.params(np.float32([999.5 / 1111]), [5], 1111, 1, 0, A.steps((0.9, )))[0][0, 6:].tolist() == [1000, 1111]  # (999.5: the fp32 product of 1000 / 1111 and 1111 rounds above 1000)
	assert A.params(np.float32([1000 / 2048]), [5], 2048, 1, 0, A.steps((1.1, )), min_out_len = [910])[0][0, 7] == 1000
	assert A.params(np.float32([1000 / 2048]), [5], 2048, 1, 0, A.steps((1.1, )), min_out_len = [909])[0][0, 7] == 909


def band_limited(rng, n, top = 0.4):
	t = np.arange(n, dtype = np.float64)
	return sum(rng.uniform(0.2, 1.0) * np.sin(2 * np.pi * rng.uniform(0.01, top) * t + rng.uniform(0, 2 * np.pi)) for _ in range(8)) / 8


def test_the_tabulated_filter_follows_the_continuous_windowed_sinc_within_its_interpolation_bound():
	"""The kernel interpolates linearly between PHASES tabulated phases, delta = 1 / PHASES apart.  For a twice differentiable h the error of the
	chord over one cell is at most delta^2 / 8 max |h''| over the cell.  A second difference D(d) = h(d - delta) - 2 h(d) + h(d + delta) equals
	delta^2 h''(xi) for some xi within delta of d, so the largest |D| over the four grid points around a cell stands for delta^2 max |h''| there,
	up to the change of h'' over at most 2 delta: h is the product of a sinc of at most 0.95 / 2 cycles per sample and a slow window, band-limited to
	half a cycle per sample for this purpose, so by Bernstein's inequality |h'''| <= pi max |h''| and that change is at most 2 pi delta times the
	largest |D| of the whole filter.  Hence per tap
	    E <= (max |D| around the cell + 2 pi delta max |D| overall) / 8,
	plus, where the cell straddles the end of the filter's support (h jumps to 0 there, by about 1e-8), the largest |h| at its grid points; plus half
	an fp32 ulp of the larger of the two table entries for the table's one rounding.  An output's bound is the sum over its taps of |x_k| E_k."""
	rng = np.random.default_rng(5)
	step_table = A.steps((0.5, 0.9, 1.1, 2.0))
	tab = A.table(step_table)
	taps, H, delta = tab.shape[1], tab.shape[1] // 2 - 1, 1.0 / A.PHASES
	assert taps == A.taps_for(step_table) == 272
	x = band_limited(rng, 700)
	for i, step in enumerate(step_table):
		c = A.cutoff(step)
		d = (np.arange(taps, dtype = np.float64)[:, None] - H) - np.arange(-1, A.PHASES + 2, dtype = np.float64)[None, :] * delta  # grid points p = -1 .. PHASES + 1
		h = A.filt(d, c)
		D = np.abs(A.filt(d - delta, c) - 2 * h + A.filt(d + delta, c))
		inside = np.abs(d) * c <= R.ZEROS
		local = np.maximum.reduce([D[:, q:q + A.PHASES] for q in range(4)])  # cell p (between grid points p and p + 1) sees the points p - 1 .. p + 2
		edge = np.logical_or.reduce([inside[:, q:q + A.PHASES] != inside[:, 1:1 + A.PHASES] for q in range(4)])
		E = (local + 2 * np.pi * delta * D.max()) / 8 + np.where(edge, np.maximum.reduce([np.abs(h[:, q:q + A.PHASES]) for q in range(4)]), 0.0)
		out_len = (len(x) << 32) // step
		got, _ = A.speed_one(x, len(x), out_len, step, tab[i])
		want, _ = A.speed_one(x, len(x), out_len, step, tab[i], continuous = c)
		k0, ph, _ = A.positions(np.arange(out_len), step)
		k = k0[:, None] - H + np.arange(taps)[None, :]
		xk = np.where((k >= 0) & (k < len(x)), np.abs(x[np.clip(k, 0, len(x) - 1)]), 0.0)
		j = np.arange(taps)[None, :]
		bound = (xk * (E[j, ph[:, None]] + 2.0 ** -25 * np.maximum(np.abs(tab[i][j, ph[:, None]]), np.abs(tab[i][j, ph[:, None] + 1])))).sum(-1)
		err = np.abs(got - want)
		assert (err <= bound).all(), (step / A.ONE, float(err.max()), float(bound[err.argmax()]))
		assert bound.max() < 2e-4, bound.max()  # (the bound itself is small: the interpolation costs about 1e-5 of full scale)


def test_a_sine_comes_out_at_its_frequency_times_the_speed():
	sr, f0, n_in = 16000, 440.0, 8000
	x = np.sin(2 * np.pi * f0 * np.arange(n_in) / sr)
	step_table = A.steps((0.9, 1.1))
	tab = A.table(step_table)
	for i, (speed, step) in enumerate(zip((0.9, 1.1), step_table)):
		out_len = (n_in << 32) // step
		y, _ = A.speed_one(x, n_in, out_len, step, tab[i])
		seg = y[300:out_len - 300]  # away from the ends, where the filter sees the zero padding
		crossings = int((np.signbit(seg[1:]) != np.signbit(seg[:-1])).sum())
		expect = 2 * f0 * speed * (len(seg) - 1) / sr
		assert abs(crossings - expect) <= 1.0, (speed, crossings, expect)
		want = np.sin(2 * np.pi * f0 * speed * np.arange(out_len) / sr)
		assert np.abs(y - want)[300:out_len - 300].max() < 1e-3  # (pass-band ripple of the filter: a sanity bound, the exact one is in the test above)


def test_the_host_tables_of_the_product_are_the_restatements():
	"""ops.augment_steps / augment_table / db_table (numpy's i0 and sinc) against the restatement's own series: the two float64 evaluations agree far
	below fp32 resolution, so after the one rounding they differ by at most one fp32 ulp of the entry (plus 1e-12 where the entry is near 0)."""
	from convasr_amd import ops
	speeds = (0.9, 1.0, 1.1)
	assert ops.augment_steps(speeds) == A.steps(speeds) and ops.augment_steps((0.5, 2.0)) == [1 << 31, 1 << 33]
	assert ops.augment_phases() == A.PHASES and ops.AUG_FIELDS == A.FIELDS and ops.AUG_ONE == A.ONE
	tab, taps = ops.augment_table(A.steps(speeds))
	ref = A.table(A.steps(speeds))
	assert taps == A.taps_for(A.steps(speeds)) == 150 and tuple(tab.shape) == ref.shape
	assert (np.abs(tab.numpy().astype(np.float64) - ref) <= 2.0 ** -23 * np.abs(ref) + 1e-12).all()
	assert ops.augment_table([A.ONE]) == (None, 0) and A.taps_for([A.ONE]) == 0
	assert np.array_equal(ops.db_table(-6, 6, 64).numpy(), A.db_table(-6, 6, 64)) and np.array_equal(ops.db_table(5, 25, 3, sign = -1.0).numpy(), A.db_table(5, 25, 3, -1.0))
	assert ops.prob_threshold(0.5) == A.threshold(0.5) == 1 << 23 and ops.prob_threshold(1.0) == 1 << 24
