"""The weight average's restatement tests/_ema_ref.py against known answers on the CPU: the closed form of the recursion, the warm-up
schedule's values, the skip rule, and torch's own round-to-nearest-even for the 16-bit mirror.  Nothing here loads the library; it is what
makes the reference of tests/test_ema_gpu.py trustworthy."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ema_ref as R  # noqa: E402

F32 = np.float32
INF, NAN = float('inf'), float('nan')


def rand32(n, seed, scale = 1.0):
	return (np.random.default_rng(seed).standard_normal(n) * scale).astype(F32)


def test_warm_up_values_and_the_cap():
	# k = 0, 1, 9, 10 -> 1/10, 2/11, 10/19, 11/20, the fp32 quotient of the fp32 sums
	for k, (a, b) in {0: (1, 10), 1: (2, 11), 9: (10, 19), 10: (11, 20)}.items():
		d, omd = R.schedule(0.999, k)
		assert d.dtype == F32 and omd.dtype == F32
		assert d == F32(a) / F32(b), (k, d)
		assert abs(float(d) - a / b) <= 2.0 ** -24 * a / b
		assert omd == F32(1) - d
	# capped at decay: 0.3 lies between 2/11 and 10/19
	assert [float(R.schedule(0.3, k)[0]) for k in (0, 1, 9, 10)] == [float(F32(1) / F32(10)), float(F32(2) / F32(11)), float(F32(0.3)), float(F32(0.3))]
	# far along the schedule the cap is what counts, and at the counter's ceiling the quotient is still below 1
	assert R.schedule(0.999, 10 ** 6)[0] == F32(0.999)
	assert R.schedule(1.0, R.K_MAX)[0] < 1


def test_first_update_copies_the_weights():
	w, e = rand32(257, 1), rand32(257, 2).astype(np.float64)
	e1, k1 = R.update(w, e, 0, 0.999)
	assert k1 == 1 and np.array_equal(e1, w.astype(np.float64))


def test_decay_zero_gives_the_weights_after_one_update():
	w, e = rand32(257, 3), rand32(257, 4).astype(np.float64)
	for k in (0, 1, 7, 1000):
		e1, k1 = R.update(w, e, k, 0.0)
		assert k1 == k + 1
		assert np.array_equal(e1, w.astype(np.float64)), k  # (d = 0: e + 1 (w - e), exact in float64 for fp32 operands of this range)


def test_constant_weights_follow_the_closed_form_and_converge():
	"""e_k - w = prod_j d_j (e_0 - w) for constant w: the error shrinks by the schedule's own factors, and goes to zero."""
	w, e0 = rand32(129, 5).astype(np.float64), rand32(129, 6).astype(np.float64)
	for decay, k0, steps in ((0.5, 3, 80), (0.9, 1, 400), (0.999, 5, 40)):
		e, k, prod = e0.copy(), k0, 1.0
		for _ in range(steps):
			prod *= float(R.schedule(decay, k)[0])  # (1 - omd differs from d by one fp32 rounding of the difference: inside the bar below)
			e, k = R.update(w, e, k, decay)
			assert np.abs((e - w) - prod * (e0 - w)).max() <= 1e-6 * max(prod, 1e-30) * np.abs(e0 - w).max() + 1e-14  # (1e-14: float64's own rounding of values of this size, a few 2^-52 per update)
		assert k == k0 + steps
		if decay < 0.999:
			assert np.abs(e - w).max() <= 1e-14, decay  # 0.5^77, 0.9^390: below float64's resolution of the values
		else:
			assert np.abs(e - w).max() < np.abs(e0 - w).max() * 0.999 ** 25


def test_skip_rule_leaves_everything_and_the_next_update_uses_the_same_k():
	w, e = rand32(65, 7), rand32(65, 8).astype(np.float64)
	clean = np.zeros(8)
	overflowed = clean.copy()
	overflowed[R.LS_OVERFLOW] = 1.0
	assert not R.skipped() and not R.skipped(0.5) and not R.skipped(-3e38, clean)
	for kw in (dict(loss_gate = NAN), dict(loss_gate = INF), dict(loss_gate = -INF), dict(scaler_state = overflowed), dict(loss_gate = 1.0, scaler_state = overflowed), dict(loss_gate = NAN, scaler_state = clean)):
		assert R.skipped(**kw), kw
		for k in (0, 4):
			e1, k1 = R.update(w, e, k, 0.999, **kw)
			assert k1 == k and np.array_equal(e1, e), (kw, k)
			# the update after the skip is the update that would have come without it
			a, b = R.update(w, e1, k1, 0.999), R.update(w, e, k, 0.999)
			assert a[1] == b[1] == k + 1 and np.array_equal(a[0], b[0])
	e1, k1 = R.update(w, e, 4, 0.999, loss_gate = 2.5, scaler_state = clean)
	assert k1 == 5 and not np.array_equal(e1, e)


def test_counter_saturates():
	w, e = rand32(8, 9), rand32(8, 10).astype(np.float64)
	assert R.update(w, e, int(R.K_MAX), 0.999)[1] == R.K_MAX
	assert R.update(w, e, int(R.K_MAX) - 1, 0.999)[1] == R.K_MAX


def test_mirror_is_torch_round_to_nearest_even():
	edge = [0.0, -0.0, 1.0, -1.0, 1e4, -1e4, 65504.0, 65519.9, 65520.0, 7e4, 3e38, -3e38, INF, -INF, NAN, 1e-40, -1e-40, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 6e-8, 2.0 ** -133,
	        1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.00390625, 0.333333343]
	x = np.concatenate([np.array(edge, dtype = F32), rand32(4096, 11), rand32(4096, 12, 1e4), rand32(4096, 13, 1e-6)])
	t = torch.from_numpy(x.copy())
	for name, dtype in (('bf16', torch.bfloat16), ('f16', torch.float16)):
		got = R.mirror_bits(x, name)
		exp = t.to(dtype).view(torch.int16).numpy().view(np.uint16)
		nan = np.isnan(x)
		assert np.array_equal(got[~nan], exp[~nan]), name
		back = torch.from_numpy(got[nan].view(np.int16).copy()).view(dtype)
		assert bool(torch.isnan(back).all()), name
