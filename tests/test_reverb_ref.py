"""The room reverberation's rule on the CPU (include/convasr_hip.h: convasr_augment_reverb_params, convasr_augment_reverb): the numpy restatement
the kernels are held to (tests/_reverb_ref.py) against a double loop over taps, known answers and the generator's existing draws, and the
host-side companions augment.synthetic_rirs and WaveformAugment's bank handling.  No GPU."""
import numpy as np
import pytest
import torch

import _augment_ref as A
import _reverb_ref as RR


def loop(y, h, d, out_len):
	z = np.zeros(len(y))
	for n in range(out_len):
		for k in range(len(h)):
			i = n + d - k
			if 0 <= i < out_len:
				z[n] += float(h[k]) * float(y[i])
	return z


def test_the_restatement_equals_a_double_loop_over_taps():
	rng = np.random.default_rng(0)
	for T, out_len, L, d in [(1, 1, 1, 0), (7, 7, 3, 0), (7, 5, 3, 2), (20, 13, 9, 4), (20, 20, 31, 30), (20, 0, 4, 1), (33, 17, 40, 11)]:
		y, h = rng.uniform(-1, 1, T).astype(np.float32), rng.normal(size = L).astype(np.float32)
		z = RR.reverb_one(y, h, d, out_len)
		assert z.shape == (T,) and np.allclose(z, loop(y, h, d, out_len), rtol = 0, atol = 1e-13)
		assert not z[out_len:].any()


def test_a_unit_spike_at_the_delay_gives_the_input_back_exactly():
	rng = np.random.default_rng(1)
	y = rng.uniform(-1, 1, (3, 50)).astype(np.float32)
	bank = np.zeros((3, 12), dtype = np.float32)
	lengths, delays = np.array([1, 5, 12]), np.array([0, 3, 11])
	bank[np.arange(3), delays] = 1.0
	assert [RR.delay(bank[r], lengths[r]) for r in range(3)] == delays.tolist()
	out_len = np.array([50, 20, 0])
	z = RR.reverb(y, out_len, [0, 1, 2], bank, lengths, delays)
	for b in range(3):
		assert np.array_equal(z[b, :out_len[b]], y[b, :out_len[b]].astype(np.float64)) and not z[b, out_len[b]:].any()
	# a row of -1, or one outside the bank, copies
	z = RR.reverb(y, [50, 50, 50], [-1, 3, -7], bank, lengths, delays)
	assert np.array_equal(z, y.astype(np.float64))


def test_the_first_largest_tap_is_the_delay_and_rows_are_normalised_to_unit_energy():
	assert RR.delay([0.5, -2.0, 2.0, 1.0], 4) == 1 and RR.delay([0.5, -2.0, 3.0, 1.0], 2) == 1 and RR.delay([0.0], 1) == 0
	bank = np.array([[3.0, 4.0, 100.0], [0.0, 0.0, 0.0]], dtype = np.float32)
	n = RR.normalize(bank, np.array([2, 3]))
	assert np.allclose(n[0], [0.6, 0.8, 0.0]) and not n[1].any()


def test_the_new_draws_leave_purposes_0_to_11_alone_and_fire_at_their_rate():
	keys = np.arange(4000, dtype = np.int64) * 7919 + (1 << 35)
	rows = RR.rir_row(keys, 5, 2, 9, A.threshold(0.5))
	on = rows >= 0
	assert abs(on.mean() - 0.5) < 0.03 and rows.max() == 8 and set(rows[on].tolist()) == set(range(9))
	assert (RR.rir_row(keys, 5, 2, 9, A.threshold(0.0)) == -1).all() and (RR.rir_row(keys, 5, 2, 9, A.threshold(1.0)) >= 0).all()
	assert not np.array_equal(rows, RR.rir_row(keys, 5, 3, 9, A.threshold(0.5))) and np.array_equal(rows, RR.rir_row(keys, 5, 2, 9, A.threshold(0.5)))
	# the words of purposes 12 and 13 are the generator's own blocks: counter (key lo, key hi, epoch, purpose << 16)
	for purpose in (RR.REVERB_FIRE, RR.REVERB_ROW):
		ctr = np.stack([keys & 0xffffffff, keys >> 32, np.full_like(keys, 2), np.full_like(keys, purpose << 16)], axis = 1)
		assert np.array_equal(A.draw(5, 2, keys, purpose), A.philox(ctr, (5, 0))[:, 0])
	# purposes 0 - 11: the parameter restatement has no bank argument, so what it draws is what it drew before -- pinned here by known answers
	p, _ = A.params(np.float32([1.0, 0.5]), np.array([0, 7], dtype = np.int64), 1000, 99, 2, A.steps((0.9, 1.0, 1.1)), gain_steps = 64, gain_thr = 1 << 24, noise_shape = (5, 777), snr_steps = 64, noise_thr = 1 << 24)
	assert (RR.REVERB_FIRE, RR.REVERB_ROW) == (12, 13) and len({A.SPEED_FIRE, A.SPEED, A.GAIN_FIRE, A.GAIN, A.NOISE_FIRE, A.NOISE_ROW, A.NOISE_OFFSET, A.SNR, A.FREQ_WIDTH, A.FREQ_START, A.TIME_WIDTH, A.TIME_START}) == 12
	assert max(A.SPEED_FIRE, A.SPEED, A.GAIN_FIRE, A.GAIN, A.NOISE_FIRE, A.NOISE_ROW, A.NOISE_OFFSET, A.SNR, A.FREQ_WIDTH, A.FREQ_START, A.TIME_WIDTH, A.TIME_START) == 11
	assert p[:, A.FIELDS.index('gain')].tolist() == A.uint(A.draw(99, 2, [0, 7], A.GAIN), 63).tolist()
	assert p[:, A.FIELDS.index('noise_row')].tolist() == A.uint(A.draw(99, 2, [0, 7], A.NOISE_ROW), 4).tolist()


def test_partials_follow_the_tile_ownership_of_the_waveform_pass():
	rng = np.random.default_rng(2)
	T = 40 * RR.TILE + 5
	z = rng.uniform(-1, 1, T)
	noise = rng.uniform(-1, 1, (2, 333)).astype(np.float32)
	f = dict(noise_row = 1, noise_offset = 17, snr = 0, out_len = 35 * RR.TILE + 9)
	p = RR.partials(z, noise, f)
	assert p.shape == (RR.PARTS, 2)
	v = A.noise_window(noise, f, f['out_len'])
	assert np.isclose(p[:, 0].sum(), (z[:f['out_len']] ** 2).sum(), rtol = 1e-13) and np.isclose(p[:, 1].sum(), (v ** 2).sum(), rtol = 1e-13)
	# part 3 owns tiles 3 and 35 (the last, partial one)
	own = np.r_[z[3 * RR.TILE:4 * RR.TILE], z[35 * RR.TILE:f['out_len']]]
	assert np.isclose(p[3, 0], (own ** 2).sum(), rtol = 1e-13)
	assert np.isclose(RR.scale(p, f, np.float32([0.5])), 0.5 * np.sqrt((z[:f['out_len']] ** 2).sum() / (v ** 2).sum()), rtol = 1e-12)
	assert RR.scale(p, dict(f, noise_row = -1), np.float32([0.5])) == 0.0


def test_synthetic_rirs_are_reproducible_and_have_their_largest_tap_first():
	from convasr_amd import augment
	bank, lengths = augment.synthetic_rirs(6, 8000, rt60 = (0.05, 0.3), seed = 4)
	again, lengths2 = augment.synthetic_rirs(6, 8000, rt60 = (0.05, 0.3), seed = 4)
	assert torch.equal(bank, again) and torch.equal(lengths, lengths2)
	other, _ = augment.synthetic_rirs(6, 8000, rt60 = (0.05, 0.3), seed = 5)
	assert other.shape != bank.shape or not torch.equal(other, bank)
	assert bank.dtype == torch.float32 and lengths.dtype == torch.int64 and bank.shape == (6, int(lengths.max()))
	assert int(lengths.min()) >= 400 and int(lengths.max()) <= 2400 and len(set(lengths.tolist())) > 1
	for r in range(6):
		L = int(lengths[r])
		h = bank[r].numpy()
		assert h[0] == 1.0 and RR.delay(h, L) == 0 and np.abs(h[1:L]).max() <= 0.9 and not h[L:].any()
		# the tail decays: its last quarter carries far less energy than its first
		assert (h[1:L // 4] ** 2).sum() > 50 * (h[3 * L // 4:L] ** 2).sum()
	# the generator underneath is the section's Philox: the first block of row 0 (counter (0, 0, 0, 'RIR'), key = the seed)
	u = augment._philox_uniforms(4, 0, 4)
	assert np.array_equal(u, (A.philox(np.array([[0, 0, 0, 0x00524952]]), (4, 0))[0].astype(np.float64) + 0.5) / 2.0 ** 32)


def test_waveform_augment_validates_and_normalises_its_bank_on_the_host():
	from convasr_amd import augment, _lib
	rng = np.random.default_rng(3)
	bank = rng.normal(size = (3, 40)).astype(np.float32)
	bank[1, 7] = 9.0
	lengths = [40, 20, 1]
	aug = augment.WaveformAugment(1, rir = torch.from_numpy(bank), rir_lengths = lengths, reverb_prob = 0.25)
	assert torch.equal(aug.rir, torch.from_numpy(RR.normalize(bank, np.array(lengths))))
	assert aug.rir_host[0].tolist() == lengths and aug.rir_host[1].tolist() == [RR.delay(bank[r], lengths[r]) for r in range(3)] and aug.rir_host[1][1] == 7
	assert aug.reverb_thr == A.threshold(0.25)
	raw = augment.WaveformAugment(1, rir = torch.from_numpy(bank), normalize_rir = False)
	assert torch.equal(raw.rir, torch.from_numpy(bank)) and raw.rir_host[0].tolist() == [40, 40, 40]
	assert augment.WaveformAugment(1).rir is None
	for bad in (dict(rir = torch.zeros(3)), dict(rir = torch.zeros(2, 4, dtype = torch.float64)), dict(rir = torch.zeros(0, 4)), dict(rir = torch.zeros(2, 4), rir_lengths = [1, 5]),
	            dict(rir = torch.zeros(2, 4), rir_lengths = [0, 4]), dict(rir = torch.zeros(2, 4), rir_lengths = [1])):
		with pytest.raises(ValueError):
			augment.WaveformAugment(1, **bad)
	with pytest.raises(_lib.ConvasrHipError, match = '32768'):
		augment.WaveformAugment(1, rir = torch.zeros(1, 32769))
