"""The augmentation kernels (csrc/augment.hip) through ops.philox, augment.WaveformAugment, ops.spec_augment / augment.SpecAugment,
augment.batches and JasperNet.feature_transform, against the numpy restatement (tests/_augment_ref.py, itself checked on the CPU by
tests/test_augment_ref.py).  The augmentation is this project's own, unpinned against any outside library.

Integers -- the generator's words, every drawn parameter, lengths, mask positions -- are compared with torch.equal.

Samples, derived (u = 2^-24, one fp32 rounding).  A resampled sample is sum_j x_j c_j over `taps` taps in fp32 with c_j = fma(f, t1 - t0, t0):
the coefficient carries two roundings, |dc_j| <= u f |t1 - t0| + u |c_j| <= 3 u m_j with m_j = max(|t0|, |t1|) >= |c_j|; a sequential fma sum of
`taps` products is within taps u sum |x_j c_j| of the exact one.  Together (taps + 3) u A, A = sum_j |x_j| m_j: the bound of
tests/test_resample_gpu.py with the coefficient's interpolation counted.  The gain multiplies once (+ 1 u g A), the mix is one fma (+ 1 u of the
result, at most g A + |a v|), and one more u is left for the second-order terms:
    |y_gpu - y_ref| <= (taps + 6) u (g A + |a v|).
The restatement is fed the device's own parameters and noise scales, so the bound separates the sample arithmetic from the reductions.

Reductions, derived.  Ex and En are float64 sums of exact products (an fp32 square is exact in float64): n terms cost at most n 2^-53 relative,
in the kernel's tree as in numpy's pairwise sum.  The divide, the square root and the multiply are three more float64 roundings on either side,
then the kernel rounds ONCE to fp32:  |a_gpu - a_ref| <= (u + (2 n + 8) 2^-52) |a_ref|.  The mean fill is one float64 sum of n values and one
divide, rounded once to fp32: |m_gpu - m_ref| <= u |m_ref| + (n + 2) 2^-52 mean |x|."""
import json
import math

import numpy as np
import pytest
import torch

import _augment_ref as A

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TILE = 1024       # convasr_augment_tile(), asserted below
SPEC_TILE = 1024  # convasr_spec_augment_tile()
KEYS = [0, (1 << 40) + 1, 7, 123456789, 5, (1 << 33) + 9, 99, 31337]
XLEN = [1.0, 0.85, 0.5, 0.0, 0.9, 0.3, 0.7, 0.95]


def dev():
	return torch.device('cuda:0')


def host_keys(B, seed = 0):
	rng = np.random.default_rng(seed)
	return np.array((KEYS + rng.integers(0, 1 << 50, max(B - len(KEYS), 0)).tolist())[:B], dtype = np.int64)


def ref_params(aug, xlen, keys, T, epoch, min_out_len = None):
	return A.params(xlen, keys, T, aug.seed, epoch, aug.steps, aug.speed_thr, 0 if aug.gain_table is None else aug.gain_table.numel(), aug.gain_thr,
	                None if aug.noise is None else tuple(aug.noise.shape), 1 if aug.snr_table is None else aug.snr_table.numel(), aug.noise_thr, min_out_len)


# ------------------------------------------------------------------------------------------------ generator

def test_philox_equals_the_restatement_word_for_word():
	from convasr_amd import ops
	vectors = [([0, 0, 0, 0], (0, 0), ['6627e8d5', 'e169c58d', 'bc57ac4c', '9b00dbd8']),
	           ([0xffffffff] * 4, (0xffffffff, 0xffffffff), ['408f276d', '41c83b0e', 'a20bc7c6', '6d5451fd']),
	           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], (0xa4093822, 0x299f31d0), ['d16cfe09', '94fdcceb', '5001e420', '24126ea1'])]
	for ctr, key, want in vectors:
		got = ops.philox(torch.tensor([ctr], dtype = torch.int64, device = dev()), key).cpu()
		assert got.tolist() == [[int(w, 16) for w in want]]
	rng = np.random.default_rng(1)
	ctr = rng.integers(0, 1 << 32, (1000, 4), dtype = np.int64)
	key = (int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)))
	got = ops.philox(torch.from_numpy(ctr).to(dev()), key).cpu()
	assert torch.equal(got, torch.from_numpy(A.philox(ctr, key).astype(np.int64)))
	assert ops.philox(torch.zeros(0, 4, dtype = torch.int64, device = dev()), key).shape == (0, 4)


# ------------------------------------------------------------------------------------------------ parameters

@pytest.mark.parametrize('B', [1, 3, 64])
def test_every_integer_parameter_equals_the_restatement(B):
	from convasr_amd import augment
	d = dev()
	T = 4000
	rng = np.random.default_rng(B)
	keys = host_keys(B, seed = 2)
	xlen = np.float32(XLEN[:B]) if B <= 8 else rng.uniform(0.0, 1.0, B).astype(np.float32)
	length = A.valid_len(xlen, T)
	min_out_len = np.where(np.arange(B) % 4 == 0, (length * 0.95).astype(np.int64), np.where(np.arange(B) % 4 == 2, length // 2, 0))  # a quarter refuses to lose more than 5 % (speed 1.1 loses 9 %), a quarter more than half
	noise = torch.zeros(5, 777, device = d)
	aug = augment.WaveformAugment(seed = 99, noise = noise, noise_prob = 0.5)
	run = lambda e, k = keys, xl = xlen, m = min_out_len: aug.params(torch.from_numpy(xl).to(d), torch.from_numpy(k).to(d), T, epoch = e, min_out_len = None if m is None else torch.from_numpy(m).to(d))
	got, got_len = run(2)
	want, want_len = ref_params(aug, xlen, keys, T, 2, min_out_len)
	for i, name in enumerate(A.FIELDS):
		assert torch.equal(got[name].cpu(), torch.from_numpy(want[:, i])), name
	assert torch.equal(got_len.cpu(), torch.from_numpy(want_len))
	again, again_len = run(2)
	assert all(torch.equal(got[n], again[n]) for n in A.FIELDS) and torch.equal(got_len, again_len)  # two calls are bit-equal
	if B == 64:
		# both fallback rules are hit by at least one utterance and missed by at least one that drew the speed in question
		drawn = A.uint(A.draw(99, 2, keys, A.SPEED), 2)
		raw = np.array([(int(l) << 32) // aug.steps[i] for l, i in zip(length, drawn)])
		too_long, too_short = raw > T, raw < min_out_len
		assert too_long.any() and (~too_long & (drawn == 0)).any() and too_short.any() and (~too_short & (drawn == 2) & (min_out_len > 0)).any()
		assert (want[too_long | too_short, 0] == -1).all() and (want[:, 0] >= 0).any()
		perm = rng.permutation(B)
		moved, moved_len = run(2, keys[perm], xlen[perm], min_out_len[perm])
		assert all(torch.equal(moved[n].cpu(), got[n].cpu()[perm]) for n in A.FIELDS) and torch.equal(moved_len.cpu(), got_len.cpu()[perm])  # a permuted batch gives permuted results
		other, _ = run(3)
		assert not all(torch.equal(other[n], got[n]) for n in A.FIELDS)  # two epochs differ


# ------------------------------------------------------------------------------------------------ samples

def make_batch(rng, B, T, dtype, offset_view, d):
	"""Random samples with GARBAGE behind every utterance's length (the kernel reads x as 0 there); optionally a view that starts one element into
	its storage."""
	x = rng.integers(-32768, 32768, (B, T)).astype(np.int16) if dtype == torch.int16 else rng.uniform(-1, 1, (B, T)).astype(np.float32)
	if offset_view:
		storage = torch.zeros(B * T + 1, dtype = dtype, device = d)
		storage[1:] = torch.from_numpy(x).reshape(-1).to(d)
		return x, storage[1:].view(B, T)
	return x, torch.from_numpy(x).to(d)


@pytest.mark.parametrize('T', [1, 40, TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_every_sample_is_within_the_fp32_bound_of_the_restatement(T):
	from convasr_amd import augment, ops
	assert ops.augment_tile() == TILE
	d = dev()
	B = 8
	keys, xlen = host_keys(B), np.float32(XLEN)
	# (dtype, the view starts one element into its storage, noise samples per row: 1, fewer than out_len (wraps several times), more than T, none)
	for case, (dtype, offset_view, L) in enumerate([(torch.float32, False, 1), (torch.int16, False, 37), (torch.float32, True, T + 50), (torch.int16, True, None)]):
		rng = np.random.default_rng(1000 * T + case)
		x_host, x = make_batch(rng, B, T, dtype, offset_view, d)
		noise_host = None if L is None else rng.uniform(-0.5, 0.5, (3, L)).astype(np.float32)
		noise = None if L is None else torch.from_numpy(noise_host).to(d)
		aug = augment.WaveformAugment(seed = 21, noise = noise, noise_prob = 0.75)  # (this seed draws 0.9, 1.0 and 1.1 and leaves two utterances without noise)
		assert aug.taps == 150
		args = (x, torch.from_numpy(xlen).to(d), torch.from_numpy(keys).to(d))
		out, xlen_out, scales = aug(*args, epoch = 1, return_scales = True)
		out2, xlen_out2, scales2 = aug(*args, epoch = 1, return_scales = True)
		assert torch.equal(out, out2) and torch.equal(xlen_out, xlen_out2) and torch.equal(scales, scales2)  # two runs are bit-equal
		assert out.shape == (B, T) and out.dtype == torch.float32
		p, _ = aug._params(args[1], args[2], T, 1, None)
		want_p, want_len = ref_params(aug, xlen, keys, T, 1)
		assert torch.equal(p.cpu(), torch.from_numpy(want_p)) and torch.equal(xlen_out.cpu(), torch.from_numpy(want_len))
		y, mag = A.waveform(x_host, want_p, aug.table.numpy(), aug.gain_table.numpy(), noise_host, scales.cpu().numpy())
		got = out.cpu().numpy().astype(np.float64)
		err, bound = np.abs(got - y), (aug.taps + 6) * U * mag
		print(f'T {T} case {case}: max err {err.max():.3e}, worst err / bound {(err / np.maximum(bound, 1e-300)).max():.3f}')
		assert (err <= bound).all(), (T, case, float((err - bound).max()))
		for b in range(B):
			assert not got[b, want_p[b, 7]:].any()  # exact zeros from out_len on
		if L is not None:
			# the scale against float64, from the device's own signal before the mix (the same seed without a noise bank draws the same speed and gain)
			plain = augment.WaveformAugment(seed = 21)
			pre, _ = plain(*args, epoch = 1)
			pre = pre.cpu().numpy()
			snr = A.db_table(5.0, 25.0, 64, -1.0)
			assert np.array_equal(aug.snr_table.numpy(), snr)
			for b in range(B):
				f = dict(zip(A.FIELDS, (int(v) for v in want_p[b])))
				a_ref = A.noise_scale(pre[b], noise_host, f, snr)
				assert abs(float(scales[b]) - a_ref) <= (U + (2 * f['out_len'] + 8) * 2.0 ** -52) * abs(a_ref), (T, case, b, float(scales[b]), a_ref)
			if T >= 40:
				assert (want_p[:, 3] >= 0).any() and (want_p[:, 3] < 0).any() and (scales.cpu().numpy()[want_p[:, 7] > 0][want_p[want_p[:, 7] > 0, 3] >= 0] > 0).all()


def test_speed_one_without_gain_and_noise_is_the_input_bit_for_bit():
	from convasr_amd import augment
	d = dev()
	B, T = 4, 2 * TILE + 5
	rng = np.random.default_rng(3)
	keys = torch.from_numpy(host_keys(B)).to(d)
	ones = torch.ones(B, device = d)
	aug = augment.WaveformAugment(seed = 5, speed = (1.0, ), gain_db = None)
	assert aug.table is None and aug.taps == 0
	for dtype in (torch.float32, torch.int16):
		x_host, x = make_batch(rng, B, T, dtype, True, d)
		out, xlen_out = aug(x, ones, keys, epoch = 4)
		assert torch.equal(out.cpu(), torch.from_numpy(A.decode(x_host))) and torch.equal(xlen_out, ones)
		# shorter utterances: the input up to the length, zeros behind it (the garbage there is not copied)
		xlen = torch.tensor([0.5, 0.0, 1.0, 0.25], device = d)
		out, xlen_out = aug(x, xlen, keys, epoch = 4)
		for b, n in enumerate(A.valid_len(xlen.cpu().numpy(), T)):
			assert torch.equal(out[b, :n].cpu(), torch.from_numpy(A.decode(x_host))[b, :n]) and not bool(out[b, n:].any())
		assert torch.equal(xlen_out.cpu(), torch.from_numpy((A.valid_len(xlen.cpu().numpy(), T).astype(np.float32) / np.float32(T))))
	# a speed table that holds 1.0 among others copies the utterances that draw it
	mixed = augment.WaveformAugment(seed = 5, speed = (0.9, 1.0), gain_db = None)
	x_host, x = make_batch(rng, 32, 300, torch.float32, False, d)
	keys32 = torch.arange(32, device = d)
	out, _ = mixed(x, torch.full((32, ), 0.8, device = d), keys32, epoch = 0)
	p, _ = mixed.params(torch.full((32, ), 0.8, device = d), keys32, 300)
	same = (p['step'] == A.ONE).cpu().numpy()
	assert same.any() and not same.all()
	assert torch.equal(out[torch.from_numpy(same).to(d), :240], x[torch.from_numpy(same).to(d), :240])


def test_silence_and_silent_noise_add_nothing_and_empty_batches_launch_nothing():
	from convasr_amd import augment
	d = dev()
	B, T = 4, TILE + 3
	rng = np.random.default_rng(4)
	keys, ones = torch.from_numpy(host_keys(B)).to(d), torch.ones(B, device = d)
	x_host, x = make_batch(rng, B, T, torch.float32, False, d)
	x[1] = 0
	noise = torch.from_numpy(rng.uniform(-1, 1, (2, 100)).astype(np.float32)).to(d)
	loud = augment.WaveformAugment(seed = 8, speed = (1.0, ), noise = noise, noise_prob = 1.0)
	out, _, scales = loud(x, ones, keys, return_scales = True)
	assert float(scales[1]) == 0.0 and not bool(out[1].any()) and bool((scales[[0, 2, 3]] > 0).all())  # an all-zero signal: Ex = 0
	silent = augment.WaveformAugment(seed = 8, speed = (1.0, ), noise = torch.zeros(2, 100, device = d), noise_prob = 1.0)
	plain = augment.WaveformAugment(seed = 8, speed = (1.0, ))
	out, _, scales = silent(x, ones, keys, return_scales = True)
	assert not bool(scales.any()) and torch.equal(out, plain(x, ones, keys)[0])  # an all-zero noise row: En = 0
	for shape in ((0, 100), (3, 0)):
		e = torch.zeros(shape, device = d)
		out, xlen_out, scales = loud(e, torch.ones(shape[0], device = d), torch.zeros(shape[0], dtype = torch.int64, device = d), return_scales = True)
		assert out.shape == shape and xlen_out.shape == (shape[0], ) and scales.shape == (shape[0], )
	torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ SpecAugment

def spec_case(F, T, seed):
	rng = np.random.default_rng(seed)
	x = rng.normal(-3.0, 2.0, (5, F, T)).astype(np.float32)
	xlen = np.float32([0.0, 0.5 / T, 1.0, 0.6, 0.05])  # valid 0, 1, T, about 0.6 T, about 0.05 T frames
	keys = np.array([0, (1 << 40) + 1, 3, 4, 5], dtype = np.int64)
	return x, xlen, keys, A.valid_len(xlen, T)


@pytest.mark.parametrize('F', [1, 64, 80])
@pytest.mark.parametrize('T', [SPEC_TILE - 1, SPEC_TILE, SPEC_TILE + 1])
def test_spec_augment_masks_and_fill_equal_the_restatement(F, T):
	from convasr_amd import ops
	assert ops.spec_augment_tile() == SPEC_TILE
	d = dev()
	x, xlen, keys, valid = spec_case(F, T, 100 * F + T)
	assert valid.tolist()[:3] == [0, 1, T]
	dx, dxlen, dkeys, depoch = torch.from_numpy(x).to(d), torch.from_numpy(xlen).to(d), torch.from_numpy(keys).to(d), torch.tensor([6], dtype = torch.int64, device = d)
	# (frequency masks, width, time masks, width, fraction, fill): the defaults; a frequency width >= F and a fraction that leaves no room for a time mask; many masks, a constant fill
	for fm, fw, tm, tw, frac, fill in [(2, 10, 2, 50, 0.05, 'mean'), (3, 100, 2, 50, 0.0009, 'mean'), (16, 7, 16, 30, 1.0, -1.5), (0, 10, 0, 10, 0.5, 'mean')]:
		out, fill_out, masks = ops.spec_augment(dx, dxlen, dkeys, depoch, 21, fm, fw, tm, tw, frac, fill, return_masks = True)
		want_masks = A.spec_masks(keys, 6, 21, F, valid, fm, fw, tm, tw, frac)
		assert torch.equal(masks.cpu().to(torch.int64), torch.from_numpy(want_masks)), (fm, fw, tm, tw, frac)
		# no mask leaves the valid region (frequency masks: the F channels)
		assert (want_masks[:, :fm].sum(-1) <= F).all() and (want_masks[:, fm:].sum(-1) <= valid[:, None]).all() and (want_masks >= 0).all()
		if frac == 0.0009:
			assert (want_masks[:, fm:, 1] == 0).all() and (want_masks[:, :fm, 1] <= F).all()
		fill_host = fill_out.cpu().numpy()
		if fill == 'mean':
			mean = A.spec_mean(x, valid)
			mean_abs = np.array([np.abs(x[b][:, :v]).mean() if v > 0 else 0.0 for b, v in enumerate(valid)])
			assert (np.abs(fill_host - mean) <= U * np.abs(mean) + (F * valid + 2) * 2.0 ** -52 * mean_abs).all(), (fill_host, mean)
			assert fill_host[0] == 0.0
		else:
			assert (fill_host == np.float32(fill)).all()
		want = A.spec_augment(x, want_masks, fm, valid, fill_host)
		assert torch.equal(out.cpu(), torch.from_numpy(want))
		covered = A.spec_covered(want_masks, fm, F, T, valid)
		assert np.array_equal(out.cpu().numpy()[~covered].view(np.uint32), x[~covered].view(np.uint32))  # unmasked values and the frames past valid: bit for bit
		assert not covered[0].any() and all(not covered[b][:, valid[b]:].any() for b in range(5))
		if fm == 16:
			assert covered[2].any() and covered[3].any()
		again = ops.spec_augment(dx, dxlen, dkeys, depoch, 21, fm, fw, tm, tw, frac, fill)
		assert torch.equal(again[0], out) and torch.equal(again[1], fill_out)


def test_a_captured_spec_augment_draws_fresh_masks_from_rewritten_buffers():
	from convasr_amd import augment, train
	d = dev()
	F, T = 64, 300
	x, xlen, keys, valid = spec_case(F, T, 9)
	dx, dxlen = torch.from_numpy(x).to(d), torch.from_numpy(xlen).to(d)
	spec = augment.SpecAugment(seed = 3, freq_masks = 2, freq_width = 20, time_masks = 2, time_width = 40, time_fraction = 0.2, max_batch = 8).to(d)
	assert not list(spec.parameters()) and not spec.state_dict()
	eager = []
	side = torch.cuda.Stream()
	side.wait_stream(torch.cuda.current_stream())
	with torch.cuda.stream(side):
		for k, e in ((keys, 0), (keys + 100, 1)):
			spec.set_keys(k, e)
			eager.append(spec(dx, dxlen).clone())
	torch.cuda.current_stream().wait_stream(side)
	assert not torch.equal(eager[0], eager[1])
	graph = torch.cuda.CUDAGraph()
	with torch.cuda.graph(graph):
		static = spec(dx, dxlen)
		kinds = train.capture_node_kinds(d)
	assert kinds == {'kernel': 1}, kinds  # a single kernel node: nothing to run in parallel
	for (k, e), want in zip(((keys, 0), (keys + 100, 1)), eager):
		spec.set_keys(k, e)
		graph.replay()
		torch.cuda.synchronize()
		assert torch.equal(static, want)


# ------------------------------------------------------------------------------------------------ through the model and the training loop

def tiny_model(num_classes, d, seed = 0):
	import convasr_amd as ca
	torch.manual_seed(seed)
	fe = ca.models.LogFilterBankFrontend(64, 8000, 0.02, 0.01, 'hann_window')
	return ca.models.Wav2Letter(64, [num_classes], frontend = fe, dropout = 0, base_width = 64, check_time_dim_padded = False).to(d)


def test_feature_transform_runs_in_training_mode_only():
	from convasr_amd import augment
	d = dev()
	model = tiny_model(38, d)
	assert model.feature_transform is None
	keys_before = set(model.state_dict())
	B, T = 3, 4096
	x = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (B, T)).astype(np.float32)).to(d)
	xlen = torch.tensor([1.0, 0.8, 0.5], device = d)
	model.eval()
	with torch.no_grad():
		bare = model(x, xlen)['logits'][0].clone()
	spec = augment.SpecAugment(seed = 1, freq_masks = 2, freq_width = 15, time_masks = 2, time_width = 20, time_fraction = 0.5)
	model.feature_transform = spec
	model.to(d)
	assert set(model.state_dict()) == keys_before  # non-persistent buffers: the state-dict layout is unchanged
	spec.set_keys([4, 5, 6], 0)
	with torch.no_grad():
		assert torch.equal(model(x, xlen)['logits'][0], bare)  # eval() never augments

	def train_logits(epoch):
		model.train()
		spec.set_keys([4, 5, 6], epoch)
		return model(x, xlen)['logits'][0].detach().clone()

	first, second, first_again = train_logits(0), train_logits(1), train_logits(0)
	assert torch.equal(first, first_again) and not torch.equal(first, second)
	model.feature_transform = None
	model.train()
	assert not torch.equal(model(x, xlen)['logits'][0].detach(), first)


def test_augmented_batches_train_through_train_epoch_and_repeat_bit_for_bit(tmp_path):
	import convasr_amd as ca
	from convasr_amd import audio, augment, datasets, train
	from convasr_amd.transcript_generators import CharTokenizerLegacy
	d = dev()
	rng = np.random.default_rng(6)
	manifest = []
	for i, (n, ref) in enumerate([(4000, 'ab c'), (3100, 'cab'), (3600, 'b a')]):
		path = str(tmp_path / f'{i}.wav')
		audio.write_audio(path, torch.from_numpy(rng.uniform(-0.5, 0.5, (1, n)).astype(np.float32)), 8000)
		manifest.append(dict(audio_path = path, ref = ref))
	(tmp_path / 'manifest.json').write_text(json.dumps(manifest))
	tokenizer = CharTokenizerLegacy('abc')
	ds = datasets.AudioTextDataset(str(tmp_path / 'manifest.json'), tokenizer, sample_rate = 8000, time_padding_multiple = 128)
	noise = torch.from_numpy(rng.uniform(-0.1, 0.1, (2, 1000)).astype(np.float32)).to(d)

	def run():
		model = tiny_model(tokenizer.vocab_size, d, seed = 3).train()
		model.feature_transform = augment.SpecAugment(seed = 2, time_fraction = 0.2).to(d)
		opt = train.SGD(train.FlatParameters(model), lr = 1e-3, momentum = 0.9, weight_decay = 1e-3)
		wave = augment.WaveformAugment(seed = 2, noise = noise, noise_prob = 1.0)
		seen, losses = [], []
		batches = augment.batches(datasets.gpu_batches(ds, [[0, 1, 2], [2, 0, 1]], d), waveform = wave, spec = model.feature_transform, epoch = 1, samples_per_label = 160)
		n = train.train_epoch(model, opt, batches, on_step = lambda it, batch, res: (seen.append((batch[2].clone(), batch[3].clone())), losses.append(res['loss'].clone())))
		torch.cuda.synchronize()
		return n, seen, [float(l) for l in losses], losses

	n, seen, values, losses = run()
	assert n == 2 and all(math.isfinite(v) for v in values), values
	assert seen[0][0].shape == (3, 4096) and seen[0][0].dtype == torch.float32
	# the second batch holds the same utterances in another order: the same epoch augments each of them the same way
	order = [2, 0, 1]
	assert torch.equal(seen[1][0], seen[0][0][order]) and torch.equal(seen[1][1], seen[0][1][order])
	plain = next(iter(datasets.gpu_batches(ds, [[0, 1, 2]], d)))
	assert not torch.equal(plain[2], seen[0][0])
	_, seen2, values2, losses2 = run()
	assert all(torch.equal(a, b) for a, b in zip(losses, losses2)) and torch.equal(seen[0][0], seen2[0][0])
	# SyntheticAudioTextDataset carries example_id too
	syn = datasets.SyntheticAudioTextDataset(4, min_duration = 0.2, max_duration = 0.4, sample_rate = 8000)
	got = list(augment.batches(datasets.gpu_batches(syn, [[0, 1], [2, 3]], d), waveform = augment.WaveformAugment(seed = 1), epoch = 0))
	assert len(got) == 2 and got[0][2].ndim == 2 and got[0][2].dtype == torch.float32


def test_envelope_violations_raise_and_launch_nothing():
	from convasr_amd import augment, ops, _lib
	d = dev()
	E = _lib.ConvasrHipError
	xlen, keys = torch.ones(2, device = d), torch.zeros(2, dtype = torch.int64, device = d)
	x = torch.zeros(2, 100, device = d)
	with pytest.raises(E, match = 'speeds'):
		augment.WaveformAugment(1, speed = (0.4, 1.0))
	with pytest.raises(E, match = 'speeds'):
		augment.WaveformAugment(1, speed = tuple([1.0] * 33))
	with pytest.raises(E, match = 'steps'):
		augment.WaveformAugment(1, gain_steps = 5000)
	with pytest.raises(E, match = r'outside \[0.5, 2\]'):
		ops.augment_params(xlen, keys, 100, 1, 0, [1 << 30])
	with pytest.raises(E, match = 'speeds'):
		ops.augment_params(xlen, keys, 100, 1, 0, [A.ONE] * 33)
	with pytest.raises(E, match = 'gain steps'):
		ops.augment_params(xlen, keys, 100, 1, 0, [A.ONE], gain_steps = 4097)
	with pytest.raises(E, match = 'SNR steps'):
		ops.augment_params(xlen, keys, 100, 1, 0, [A.ONE], noise_shape = (1, 10), snr_steps = 0)
	with pytest.raises(E, match = r'2\^31'):
		ops.augment_params(xlen, keys, 1 << 31, 1, 0, [A.ONE])
	with pytest.raises(E, match = r'2\^31'):
		ops.augment_params(xlen, keys, 100, 1, 0, [A.ONE], noise_shape = (1, 1 << 31))
	with pytest.raises(E, match = 'epoch'):
		ops.augment_params(xlen, keys, 100, 1, -1, [A.ONE])
	with pytest.raises(E, match = 'lives on'):
		augment.WaveformAugment(1, noise = torch.zeros(2, 50))(x, xlen, keys)
	p, _ = ops.augment_params(xlen, keys, 100, 1, 0, [A.ONE])
	with pytest.raises(E, match = 'LDS'):
		ops.augment_waveform(x, p, table = torch.zeros(1, 300, ops.augment_phases() + 1, device = d))
	with pytest.raises(E, match = 'taps'):
		ops.augment_waveform(x, p, table = torch.zeros(1, 151, ops.augment_phases() + 1, device = d))
	with pytest.raises(ValueError):
		ops.augment_waveform(x.double(), p)
	f = torch.zeros(2, 8, 50, device = d)
	epoch = torch.zeros(1, dtype = torch.int64, device = d)
	with pytest.raises(E, match = 'masks'):
		ops.spec_augment(f, xlen, keys, epoch, 1, freq_masks = 17)
	with pytest.raises(E, match = 'masks'):
		ops.spec_augment(f, xlen, keys, epoch, 1, time_masks = 17)
	with pytest.raises(E, match = 'widths'):
		ops.spec_augment(f, xlen, keys, epoch, 1, freq_width = -1)
	with pytest.raises(ValueError):
		ops.spec_augment(f, xlen, keys[:1], epoch, 1)
	with pytest.raises(E, match = 'max_batch'):
		augment.SpecAugment(1, max_batch = 1).to(d)(f, xlen)
	# a parameter tensor of the caller's own making with indices outside every table reads as "nothing drawn"
	wild = torch.tensor([[7, 1 << 40, 99, 99, -5, 99, 100, 100], [0, 1 << 32, -1, -1, 0, 0, 1000, 1000]], dtype = torch.int64, device = d)
	x = torch.rand(2, 100, device = d)
	out, scales = ops.augment_waveform(x, wild, gain_table = torch.ones(4, device = d), noise = torch.ones(1, 10, device = d), snr_table = torch.ones(2, device = d))
	assert torch.equal(out, x) and not bool(scales.any())
	torch.cuda.synchronize()
