"""convasr_resample (csrc/resample.hip) through ops.resample, audio.read_audio / audio.resample and datasets.AudioTextDataset.

Tolerance, derived: per output sample |y_gpu - y_ref| <= (n_k + 2) 2^-24 A, with n_k the taps inside the signal and A = s sum_k |x[k] h[k]| from
the float64 restatement (tests/_resample_ref.py, itself checked on the CPU by tests/test_resample_ref.py): the bound of an fp32 sequential sum
of n_k products (n_k 2^-24 A; it holds with fma) plus one rounding of every coefficient (2^-24 A), one more 2^-24 A to spare for the second-order
terms.  Everything else is exact equality: two runs, the three routes, the equal-rate path against the reference's decode, the guards."""
import json
import os

import numpy as np
import pytest
import torch

import _resample_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TILE = 256  # convasr_resample_tile(), asserted below

# rates, and whether the tile route takes them (48 -> 1 kHz needs a span of 75 KB per workgroup: the direct route)
RATIOS = [(8000, 16000, True), (16000, 8000, True), (48000, 16000, True), (44100, 16000, True), (8000, 11025, True), (48000, 1000, False)]
LENGTHS = [1, 2, 63, 64, 65, 1000, 4097]


def dev():
	return torch.device('cuda:0')


def lengths_for(sr_in, sr_out):
	"""The listed input lengths plus those whose output length is TILE - 1, TILE, TILE + 1 and 2 TILE + 1 (where the ratio reaches them: an
	upsampling by 2 only gives even lengths, there the next one above)."""
	out = list(LENGTHS)
	L, M = R.ratio(sr_in, sr_out)
	for target in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
		T_in = target * M // L
		while R.out_len(T_in, sr_in, sr_out) < target:
			T_in += 1
		out.append(T_in)
	return sorted(set(out))


_cache = {}


def case(sr_in, sr_out, T_in):
	"""Inputs and float64 references of one (ratio, length), computed once: rows 0-1 a planar fp32 pair uniform in [-1, 1], row 2 its fp32 mean,
	rows 3-4 a full-scale int16 pair decoded, row 5 its fp32 mean."""
	key = (sr_in, sr_out, T_in)
	if key not in _cache:
		rng = np.random.default_rng(sr_in * 7 + sr_out * 3 + T_in)
		f = rng.uniform(-1, 1, (2, T_in)).astype(np.float32)
		pcm = rng.integers(-32768, 32768, (T_in, 2)).astype(np.int16)
		pcm[rng.integers(0, T_in, 2), rng.integers(0, 2, 2)] = [32767, -32768]
		d = R.decode_int16(pcm)
		rows = np.concatenate([f, R.mono_mean(f), d, R.mono_mean(d)])
		y, n_k, A = R.resample(rows, sr_in, sr_out)
		_cache[key] = dict(f = f, pcm = pcm, y = y, bound = (n_k[None] + 2) * 2.0 ** -24 * A)
	return _cache[key]


def check(got, c, rows, what):
	got = got.cpu().numpy().astype(np.float64)
	want, bound = c['y'][rows], c['bound'][rows]
	assert got.shape == want.shape, (what, got.shape, want.shape)
	excess = np.abs(got - want) - bound
	assert (excess <= 0).all(), f'{what}: worst excess {excess.max():.3e} over a bound of {bound.flat[excess.argmax()]:.3e} at {np.unravel_index(excess.argmax(), excess.shape)}'


@pytest.mark.parametrize('sr_in,sr_out,tiled', RATIOS)
def test_every_layout_and_length_is_within_the_fp32_bound_and_the_routes_agree_bit_for_bit(sr_in, sr_out, tiled):
	from convasr_amd import ops, _lib
	assert ops.resample_tile() == TILE
	d = dev()
	for T_in in lengths_for(sr_in, sr_out) if tiled else (1, 65, 1000, 4097):
		c = case(sr_in, sr_out, T_in)
		f, pcm = torch.from_numpy(c['f']).to(d), torch.from_numpy(c['pcm']).to(d)
		T_out = R.out_len(T_in, sr_in, sr_out)
		runs = [('planar fp32', f, False, [0, 1]), ('planar fp32, mono', f, True, [2]), ('int16 C = 2', pcm, False, [3, 4]), ('int16 C = 2, mono', pcm, True, [5]),
		        ('int16 C = 1', pcm[:, :1].contiguous(), False, [3]), ('int16 C = 1, mono', pcm[:, :1].contiguous(), True, [3])]
		for what, x, mono, rows in runs:
			what = f'{sr_in} -> {sr_out}, T_in {T_in}, {what}'
			y = ops.resample(x, sr_in, sr_out, mono = mono)
			assert y.shape == (len(rows), T_out) and y.dtype == torch.float32, what
			check(y, c, rows, what)
			assert torch.equal(y, ops.resample(x, sr_in, sr_out, mono = mono)), what + ': two runs differ'
			assert torch.equal(y, ops.resample(x, sr_in, sr_out, mono = mono, route = 2)), what + ': the direct route differs'
			if tiled:
				assert torch.equal(y, ops.resample(x, sr_in, sr_out, mono = mono, route = 1)), what + ': the tile route differs'
	if not tiled:
		with pytest.raises(_lib.ConvasrHipError, match = 'LDS'):
			ops.resample(f, sr_in, sr_out, route = 1)


def test_equal_rates_only_decode_and_mix_exactly_as_the_reference():
	from convasr_amd import ops, audio
	g = np.load(os.path.join(GOLDEN, 'audio_read.npz'), allow_pickle = False)
	d = dev()
	pcm = torch.from_numpy(np.ascontiguousarray(audio.decode_audio(os.path.join(GOLDEN, 'audio_stereo.wav'), None)[0])).to(d)
	assert np.array_equal(ops.resample(pcm, 8000, 8000).cpu().numpy(), g['stereo'])
	assert np.array_equal(ops.resample(pcm, 8000, 8000, mono = True).cpu().numpy(), g['stereo_mono'])
	fl = torch.from_numpy(g['float']).to(d)
	assert np.array_equal(ops.resample(fl, 16000, 16000).cpu().numpy(), g['float'])
	assert np.array_equal(ops.resample(fl, 16000, 16000, mono = True).cpu().numpy(), g['float_mono'])
	# every int16 value
	every = torch.arange(-32768, 32768, dtype = torch.int32).to(torch.int16).reshape(-1, 1)
	assert np.array_equal(ops.resample(every.to(d), 16000, 16000).cpu().numpy(), R.decode_int16(every.numpy()))
	# through read_audio, file rate kept (sample_rate None or equal)
	for m in json.loads(str(g['meta'])):
		if m['name'] == 'unreadable':
			continue
		signal, rate = audio.read_audio(os.path.join(GOLDEN, m['file']), None, **m['kwargs'])
		assert signal.is_cuda and rate == m['sample_rate'] and str(signal.dtype) == 'torch.' + m['dtype'] and np.array_equal(signal.cpu().numpy(), g[m['name']]), m['name']


def test_empty_inputs_launch_nothing_and_unreadable_files_give_the_empty_result(capsys):
	from convasr_amd import ops, audio
	d = dev()
	for x, mono in ((torch.zeros(0, 2, dtype = torch.int16, device = d), False), (torch.zeros(0, 2, dtype = torch.int16, device = d), True), (torch.zeros(2, 0, device = d), False)):
		for rates in ((8000, 16000), (44100, 16000), (16000, 16000)):
			y = ops.resample(x, *rates, mono = mono)
			assert y.shape == (1 if mono else 2, 0) and y.dtype == torch.float32
	signal, rate = audio.read_audio('/no/such/file.wav', 16000)
	assert signal.shape == (1, 0) and signal.dtype == torch.float32 and signal.is_cuda and rate == 16000
	assert 'Error when reading' in capsys.readouterr().out


def test_guards_around_the_output_are_untouched():
	from convasr_amd import ops, _lib
	d = dev()
	guard = 4096
	for sr_in, sr_out, T_in, mono, route in ((8000, 16000, 1000, False, 1), (44100, 16000, 4097, True, 1), (48000, 16000, 769, False, 1), (8000, 11025, 187, False, 2), (16000, 16000, 513, False, 0)):
		c = case(sr_in, sr_out, T_in) if sr_in != sr_out else None
		pcm = torch.from_numpy(c['pcm'] if c else np.random.default_rng(1).integers(-32768, 32768, (T_in, 2)).astype(np.int16)).to(d)
		T_out, rows = R.out_len(T_in, sr_in, sr_out), 1 if mono else 2
		table = ops.resample_table(sr_in, sr_out).to(d) if c else None
		buf = torch.full((guard + rows * T_out + guard, ), 7.25, device = d)
		out = buf[guard:guard + rows * T_out]
		_lib.call('convasr_resample', pcm.data_ptr(), _lib.I16, T_in, 2, int(mono), _lib.ptr(table), 0 if table is None else table.shape[0], sr_in, sr_out, out.data_ptr(), T_out, route, _lib.stream_ptr())
		assert bool((buf[:guard] == 7.25).all()) and bool((buf[guard + rows * T_out:] == 7.25).all()), (sr_in, sr_out, T_in)
		assert torch.equal(out.view(rows, T_out), ops.resample(pcm, sr_in, sr_out, mono = mono))


def test_envelope_violations_raise_and_launch_nothing():
	from convasr_amd import ops, _lib
	d = dev()
	with pytest.raises(_lib.ConvasrHipError, match = 'channels'):
		ops.resample(torch.zeros(100, 9, dtype = torch.int16, device = d), 8000, 16000)
	with pytest.raises(_lib.ConvasrHipError, match = 'channels'):
		ops.resample(torch.zeros(9, 100, device = d), 16000, 16000, mono = True)
	with pytest.raises(_lib.ConvasrHipError, match = '2\\^22'):
		ops.resample(torch.zeros(2, 100, device = d), 44101, 16000)
	with pytest.raises(ValueError):
		ops.resample(torch.zeros(2, 100, dtype = torch.float64, device = d), 8000, 16000)
	torch.cuda.synchronize()


def test_read_audio_and_resample_through_the_public_interface():
	from convasr_amd import ops, audio
	g = np.load(os.path.join(GOLDEN, 'audio_read.npz'), allow_pickle = False)
	d = dev()
	wav = os.path.join(GOLDEN, 'audio_stereo.wav')
	for rate in (16000, 11025, 4000):
		signal, sr = audio.read_audio(wav, rate, mono = False)
		assert sr == rate and signal.is_cuda and torch.equal(signal, ops.resample(torch.from_numpy(g['stereo']).to(d), 8000, rate))
		signal, sr = audio.read_audio(wav, rate)
		assert sr == rate and signal.shape[0] == 1 and torch.equal(signal, ops.resample(torch.from_numpy(g['stereo_mono']).to(d), 8000, rate))
	signal, sr = audio.read_audio(wav, 16000, mono = False, offset = 0.0123, duration = 0.0171)
	assert torch.equal(signal, ops.resample(torch.from_numpy(g['slice']).to(d), 8000, 16000))
	signal, sr = audio.read_audio(os.path.join(GOLDEN, 'audio_pcm.raw'), 16000, mono = False, raw_sample_rate = 8000, raw_num_channels = 2)
	assert sr == 16000 and torch.equal(signal, ops.resample(torch.from_numpy(g['stereo']).to(d), 8000, 16000))
	signal, sr = audio.read_audio(os.path.join(GOLDEN, 'audio_float.wav'), 8000)
	assert sr == 8000 and torch.equal(signal, ops.resample(torch.from_numpy(g['float_mono']).to(d), 16000, 8000))
	# int16 out: no mix, no rate change
	with pytest.raises(AssertionError):
		audio.read_audio(wav, 16000, mono = False, dtype = 'int16')
	with pytest.raises(AssertionError):
		audio.read_audio(wav, 8000, mono = True, dtype = 'int16')
	# audio.resample: a CPU tensor goes to the current device and the result stays there
	x = torch.from_numpy(g['stereo'])
	on_cpu, sr = audio.resample(x, 8000, 16000)
	on_gpu, _ = audio.resample(x.to(d), 8000, 16000)
	assert sr == 16000 and on_cpu.is_cuda and on_cpu.shape == (2, 662) and torch.equal(on_cpu, on_gpu)
	with pytest.raises(AssertionError):
		audio.resample(x.to(torch.int16), 8000, 16000)


def test_audio_text_dataset_through_the_gpu_collate(tmp_path):
	from convasr_amd import audio, datasets
	from convasr_amd.transcript_generators import CharTokenizerLegacy
	d = dev()
	stereo, mono = os.path.join(GOLDEN, 'audio_stereo.wav'), os.path.join(GOLDEN, 'audio_mono.wav')
	manifest = [dict(audio_path = stereo, ref = 'ab c'), dict(audio_path = mono, ref = 'cab', begin = 0.001, end = 0.005), dict(audio_path = stereo, ref = 'b', channel = 1)]
	path = tmp_path / 'manifest.json'
	path.write_text(json.dumps(manifest))
	tokenizer = CharTokenizerLegacy('abc')
	ds = datasets.AudioTextDataset(str(path), tokenizer, sample_rate = 16000, time_padding_multiple = 128)
	assert len(ds) == 3 and ds.bucket.tolist() == [1, 1, 1] and ds.duration.tolist() == pytest.approx([331 / 8000, 0.004, 331 / 8000])
	sample = ds[1]
	assert not sample[2].is_cuda and sample[2].dtype == torch.int16 and sample[2].shape == (1, int(0.005 * 44100) - int(0.001 * 44100)) and sample[0]['sample_rate'] == 44100
	assert len(datasets.BucketingBatchSampler(ds, batch_size = 3)) == 1
	batches = list(datasets.gpu_batches(ds, [[0, 1, 2]], d))
	assert len(batches) == 1
	meta, s, x, xlen, y, ylen = batches[0]
	by_hand = [audio.read_audio(stereo, 16000)[0], audio.read_audio(mono, 16000, offset = 0.001, duration = 0.004)[0], audio.read_audio(stereo, 16000, mono = False)[0][1:2]]
	lengths = [w.shape[1] for w in by_hand]
	assert lengths == [662, R.out_len(176, 44100, 16000), 662]
	Tpad = 768
	want = torch.zeros(3, Tpad, device = d)
	for b, w in enumerate(by_hand):
		want[b, :lengths[b]] = w[0]
	assert x.shape == (3, Tpad) and torch.equal(x, want)
	assert torch.equal(xlen.cpu(), torch.tensor([l / Tpad for l in lengths], dtype = torch.float32))
	assert ylen.tolist() == [[4], [3], [1]] and y.shape == (3, 1, 128) and y[0, 0, :4].tolist() == tokenizer.encode(['ab c'])[0] and int(y[:, :, 4:].abs().sum()) == 0
	assert [m['sample_rate'] for m in meta] == [8000, 44100, 8000]


def test_transcribe_file_reads_the_file_and_calls_transcribe_batch():
	import types
	from convasr_amd import audio, transcribe
	from convasr_amd.transcript_generators import CharTokenizerLegacy, GreedyCTCGenerator
	d = dev()
	pipeline = transcribe.TextPipeline(CharTokenizerLegacy('abc'))
	seen = []

	def model(x, xlen):
		seen.append(x)
		frames = x.shape[-1] // 16
		gen = torch.Generator().manual_seed(3)
		log_probs = torch.randn(x.shape[0], pipeline.tokenizer.vocab_size, frames, generator = gen).log_softmax(dim = 1).to(d)
		return log_probs, log_probs, torch.full((x.shape[0], ), frames, dtype = torch.int64, device = d)

	wav = os.path.join(GOLDEN, 'audio_stereo.wav')
	for mono, channels in ((True, 1), (False, 2)):
		args = types.SimpleNamespace(device = 'cuda:0', sample_rate = 16000, mono = mono)
		out = transcribe.transcribe_file(args, pipeline, model, GreedyCTCGenerator(), wav)
		signal, _ = audio.read_audio(wav, 16000, mono = mono)
		assert torch.equal(seen[-1], signal) and len(out.hyp) == channels
		want = transcribe.transcribe_batch(args, pipeline, model, GreedyCTCGenerator(), signal, torch.ones(channels), torch.zeros(channels), torch.full((channels, ), 662 / 16000))
		assert out.hyp == want.hyp and out.hyp_segments == want.hyp_segments
