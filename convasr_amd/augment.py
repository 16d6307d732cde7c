"""Training-time data augmentation on the GPU: speed, gain, room reverberation and noise on the collated waveforms, SpecAugment on the log-mel
features.

The reference trains without augmentation (its frontend's dither is commented out), so what is here is the project's own, defined in
include/convasr_hip.h and unpinned against torchaudio, NeMo or Kaldi.  Every random decision is a pure function of (seed, epoch,
meta['example_id'], purpose, index) through a counter-based generator (Philox4x32-10): it does not depend on the utterance's place in the batch,
on the batch's composition, on the rank or on the steps that ran before, so a resumed or re-sharded run augments every utterance exactly as the
uninterrupted run would.  Augmentation is off unless asked for, and a model in eval() mode never augments.

	wave = augment.WaveformAugment(seed = 1, noise = noise_bank)          # (N, L) float32 device tensor, or None
	rir, rir_lengths = augment.synthetic_rirs(200, 16000)                  # or augment.load_rirs(paths, 16000)
	wave = augment.WaveformAugment(seed = 1, noise = noise_bank, rir = rir.to(device), rir_lengths = rir_lengths)
	spec = augment.SpecAugment(seed = 1)
	model.feature_transform = spec
	batches = augment.batches(datasets.gpu_batches(dataset, sampler, device), waveform = wave, spec = spec, epoch = epoch, samples_per_label = 320)
	train.train_epoch(model, optimizer, batches, ...)
"""
import math

import torch
from torch import nn

from . import _lib, ops

RIR_MAX_LEN = 32768  # include/convasr_hip.h: the longest impulse response convasr_augment_reverb takes (2 s at 16 kHz)


class WaveformAugment:
	"""Speed perturbation, gain, room reverberation and noise mixing of a collated batch, in that order per utterance (include/convasr_hip.h:
	convasr_augment_params, convasr_augment_waveform, convasr_augment_reverb, convasr_augment_mix): two launches, three with a noise bank, four
	more with a bank of impulse responses, no host synchronisation.  The batch keeps its padded length, so bucket-padded batches keep one shape
	per bucket.

	speed: at most 32 factors in [0.5, 2.0], one drawn per utterance with probability speed_prob; an utterance whose new length would exceed the
	padded length or fall below min_out_len keeps speed 1.0.  gain_db: gain_steps values evenly spaced in dB between the two ends (None: no
	gain), one drawn with probability gain_prob.  Under the frontend's peak normalisation (normalize_signal = True) the gain cancels, so it
	matters only relative to the mixed noise, which is added after it.  noise: a (N, L) float32 device tensor of recordings; with probability
	noise_prob a row, a start offset (the row wraps) and one of snr_steps signal-to-noise ratios evenly spaced in dB over snr_db are drawn.
	rir: a (R, Lmax) float32 device tensor of room impulse responses, rir_lengths their (R,) lengths (None: Lmax each), at most 32768 taps; with
	probability reverb_prob a row is drawn and the utterance convolved with it, shifted by the row's direct path (its first largest |tap|) and
	cut at its own length, so lengths and labels stay aligned; the noise is added afterwards, at an SNR relative to the reverberated speech.
	normalize_rir scales every row to unit energy (float64 on the host, rounded once)."""

	def __init__(self, seed, speed = (0.9, 1.0, 1.1), speed_prob = 1.0, gain_db = (-6.0, 6.0), gain_steps = 64, gain_prob = 1.0, noise = None, snr_db = (5.0, 25.0), snr_steps = 64, noise_prob = 0.5,
	             rir = None, rir_lengths = None, reverb_prob = 0.5, normalize_rir = True):
		self.seed = int(seed)
		speed = tuple(float(s) for s in speed)
		if not 1 <= len(speed) <= 32 or any(not 0.5 <= s <= 2.0 for s in speed):
			raise _lib.ConvasrHipError(f'WaveformAugment: 1 to 32 speeds in [0.5, 2.0] expected, got {speed}')
		if gain_db is not None and not 1 <= int(gain_steps) <= 4096 or noise is not None and not 1 <= int(snr_steps) <= 4096:
			raise _lib.ConvasrHipError(f'WaveformAugment: gain_steps {gain_steps} / snr_steps {snr_steps} outside [1, 4096]')
		if noise is not None and (noise.ndim != 2 or noise.dtype != torch.float32 or noise.shape[0] < 1 or noise.shape[1] < 1):
			raise ValueError(f'WaveformAugment: noise must be a (N, L) float32 tensor with N, L >= 1, got {tuple(noise.shape)} {noise.dtype}')
		self.steps = ops.augment_steps(speed)
		self.table, self.taps = ops.augment_table(self.steps)
		self.gain_table = None if gain_db is None else ops.db_table(gain_db[0], gain_db[1], gain_steps)
		self.snr_table = None if noise is None else ops.db_table(snr_db[0], snr_db[1], snr_steps, sign = -1.0)
		self.noise = noise
		self.speed_thr, self.gain_thr, self.noise_thr = ops.prob_threshold(speed_prob), ops.prob_threshold(gain_prob) if gain_db is not None else 0, ops.prob_threshold(noise_prob) if noise is not None else 0
		self._on = {}
		self.rir = self.rir_len = self.rir_delay = self.rir_host = None
		self.reverb_thr = 0
		if rir is not None:
			self._set_rirs(rir, rir_lengths, normalize_rir)
			self.reverb_thr = ops.prob_threshold(reverb_prob)

	def _set_rirs(self, rir, rir_lengths, normalize):
		if rir.ndim != 2 or rir.dtype != torch.float32 or rir.shape[0] < 1 or rir.shape[1] < 1:
			raise ValueError(f'WaveformAugment: rir must be a (R, Lmax) float32 tensor with R, Lmax >= 1, got {tuple(rir.shape)} {rir.dtype}')
		R, Lmax = rir.shape
		lengths = torch.full((R,), Lmax, dtype = torch.int64) if rir_lengths is None else torch.as_tensor(rir_lengths).detach().cpu().to(torch.int64).reshape(-1)
		if lengths.shape != (R,) or int(lengths.min()) < 1 or int(lengths.max()) > Lmax:
			raise ValueError(f'WaveformAugment: rir_lengths must be {R} integers in [1, {Lmax}]')
		if int(lengths.max()) > RIR_MAX_LEN:
			raise _lib.ConvasrHipError(f'WaveformAugment: an impulse response of {int(lengths.max())} taps > {RIR_MAX_LEN}')
		h = rir.detach().cpu().to(torch.float64) * (torch.arange(Lmax)[None, :] < lengths[:, None])  # (nothing behind a row's length is read: zeroed for the energy)
		if normalize:
			energy = (h * h).sum(dim = 1, keepdim = True)
			h = h / torch.where(energy > 0, energy.sqrt(), torch.ones_like(energy))
		h = h.to(torch.float32)
		self.rir_host = (lengths.contiguous(), ops.rir_delays(h, lengths))
		self.rir = h.to(rir.device)
		self.rir_len, self.rir_delay = self.rir_host[0].to(rir.device), self.rir_host[1].to(rir.device)

	def _tables(self, device):
		t = self._on.get(device)
		if t is None:
			t = self._on[device] = tuple(None if h is None else h.to(device) for h in (self.table, self.gain_table, self.snr_table))
		return t

	def params(self, xlen, keys, T, epoch = 0, min_out_len = None):
		"""The drawn integers as device tensors: (dict of (B,) int64 tensors named ops.AUG_FIELDS, xlen_out (B,) float32)."""
		p, xlen_out = self._params(xlen, keys, T, epoch, min_out_len)
		named = {name: p[:, i] for i, name in enumerate(ops.AUG_FIELDS)}
		if self.rir is not None:
			named['rir_row'] = self._rir_row(keys, epoch)
		return named, xlen_out

	def _rir_row(self, keys, epoch):
		return ops.reverb_params(keys, self.seed, epoch, self.rir.shape[0], self.reverb_thr)

	def _params(self, xlen, keys, T, epoch, min_out_len):
		if self.noise is not None and self.noise.device != xlen.device:
			raise _lib.ConvasrHipError(f'WaveformAugment: the noise bank lives on {self.noise.device}, the batch on {xlen.device}')
		if self.rir is not None and self.rir.device != xlen.device:
			raise _lib.ConvasrHipError(f'WaveformAugment: the bank of impulse responses lives on {self.rir.device}, the batch on {xlen.device}')
		return ops.augment_params(xlen, keys, T, self.seed, epoch, self.steps, self.speed_thr, 0 if self.gain_table is None else self.gain_table.numel(), self.gain_thr,
		                          None if self.noise is None else self.noise.shape, 1 if self.snr_table is None else self.snr_table.numel(), self.noise_thr, min_out_len)

	def __call__(self, x, xlen, keys, epoch = 0, min_out_len = None, return_scales = False):
		"""x (B, T) float32 or int16 and xlen (B,) as gpu_batches yields them, keys (B,) int64 -> (x_out (B, T) float32, xlen_out (B,) float32)."""
		_lib.require_cuda(x, xlen, keys)
		p, xlen_out = self._params(xlen, keys, x.shape[-1], epoch, min_out_len)
		table, gain_table, snr_table = self._tables(x.device)
		if self.rir is None:
			out, scales = ops.augment_waveform(x, p, table, gain_table, self.noise, snr_table)
		else:
			out, scales = ops.augment_waveform(x, p, table, gain_table, self.noise, snr_table, rir = self.rir, rir_len = self.rir_len, rir_delay = self.rir_delay, rir_row = self._rir_row(keys, epoch),
			                                   rir_host = self.rir_host)
		return (out, xlen_out, scales) if return_scales else (out, xlen_out)


class SpecAugment(nn.Module):
	"""Frequency and time masks on (B, F, T) log-mel features (include/convasr_hip.h: convasr_spec_augment), one launch.  No parameters; the keys
	and the epoch live in non-persistent buffers, so a model's state dict is unchanged and a captured graph that holds the launch draws fresh
	masks on every replay after set_keys (a device-side copy in stream order).  fill = 'mean' is the utterance's own mean over all channels and
	valid frames, neutral under the MaskedInstanceNorm1d that follows."""

	def __init__(self, seed, freq_masks = 2, freq_width = 10, time_masks = 2, time_width = 50, time_fraction = 0.05, fill = 'mean', max_batch = 1024):
		super().__init__()
		self.seed, self.freq_masks, self.freq_width, self.time_masks, self.time_width, self.time_fraction, self.fill = int(seed), int(freq_masks), int(freq_width), int(time_masks), int(time_width), float(time_fraction), fill
		self.register_buffer('keys', torch.zeros(int(max_batch), dtype = torch.int64), persistent = False)
		self.register_buffer('epoch', torch.zeros(1, dtype = torch.int64), persistent = False)

	def set_keys(self, keys, epoch = 0):
		"""keys: (B,) integers (a tensor on either side, or a list), B <= max_batch.  Written into the buffers in stream order, without a
		host synchronisation."""
		keys = torch.as_tensor(keys, dtype = torch.int64)
		if keys.ndim != 1 or keys.shape[0] > self.keys.shape[0]:
			raise _lib.ConvasrHipError(f'SpecAugment.set_keys: {tuple(keys.shape)} keys for buffers of {self.keys.shape[0]} (max_batch)')
		self.keys[:keys.shape[0]].copy_(keys, non_blocking = True)
		self.epoch.fill_(int(epoch))

	def forward(self, features, xlen):
		if features.shape[0] > self.keys.shape[0]:
			raise _lib.ConvasrHipError(f'SpecAugment: a batch of {features.shape[0]} for buffers of {self.keys.shape[0]} (max_batch)')
		if xlen is None:
			xlen = torch.ones(features.shape[0], dtype = torch.float32, device = features.device)
		return ops.spec_augment(features, xlen, self.keys, self.epoch, self.seed, self.freq_masks, self.freq_width, self.time_masks, self.time_width, self.time_fraction, self.fill)[0]


def _philox_uniforms(seed, row, count):
	"""`count` float64 uniforms in (0, 1) for impulse response `row`: the words of the Philox4x32-10 blocks with counter (k, row, 0, 'RIR') and key
	(seed low word, seed high word), (word + 0.5) / 2^32.  Plain integer arithmetic on the host: the section's generator, restated."""
	import numpy as np
	mask = np.uint64(0xffffffff)
	nblocks = (int(count) + 3) // 4
	c = [np.arange(nblocks, dtype = np.uint64) & mask, np.full(nblocks, int(row) & 0xffffffff, dtype = np.uint64), np.zeros(nblocks, dtype = np.uint64), np.full(nblocks, 0x00524952, dtype = np.uint64)]
	seed = int(seed) & 0xffffffffffffffff
	k0, k1 = np.uint64(seed & 0xffffffff), np.uint64(seed >> 32)
	for _ in range(10):
		p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
		c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
		k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
	return ((np.stack(c, axis = 1).reshape(-1)[:int(count)].astype(np.float64) + 0.5) / 4294967296.0)


def synthetic_rirs(n, sample_rate, rt60 = (0.2, 0.8), seed = 0):
	"""`n` synthetic room impulse responses: (bank (n, Lmax) float32, lengths (n,) int64), CPU tensors.  Row i draws a reverberation time uniform
	in rt60 (seconds), has floor(rt60_i * sample_rate) taps (at least 1, at most 32768), a unit direct path at tap 0 and behind it Gaussian noise
	of standard deviation 0.2 that decays by 60 dB over its length, clipped to +-0.9 so that the direct path stays the largest tap.  Built in
	float64 from the section's counter-based generator (Box-Muller), so it depends on nothing but (n, sample_rate, rt60, seed)."""
	import numpy as np
	lo, hi = float(rt60[0]), float(rt60[1])
	if int(n) < 1 or not 0.0 < lo <= hi:
		raise ValueError(f'synthetic_rirs: n >= 1 and 0 < rt60[0] <= rt60[1] expected, got {n} and {rt60}')
	rows = []
	for i in range(int(n)):
		t60 = lo + (hi - lo) * float(_philox_uniforms(seed, i, 1)[0])
		L = min(max(int(math.floor(t60 * float(sample_rate))), 1), RIR_MAX_LEN)
		u = _philox_uniforms(seed, i, 4 + 2 * L)[4:]
		g = np.sqrt(-2.0 * np.log(u[0::2])) * np.cos(2.0 * np.pi * u[1::2])
		h = np.clip(0.2 * g * np.exp(-math.log(1000.0) * np.arange(L, dtype = np.float64) / L), -0.9, 0.9)
		h[0] = 1.0
		rows.append(h)
	lengths = torch.tensor([len(h) for h in rows], dtype = torch.int64)
	bank = np.zeros((len(rows), int(lengths.max())), dtype = np.float32)
	for i, h in enumerate(rows):
		bank[i, :len(h)] = h.astype(np.float32)
	return torch.from_numpy(bank), lengths


def load_rirs(paths, sample_rate, max_len = RIR_MAX_LEN):
	"""Recorded room impulse responses: every file read as mono at `sample_rate` through audio.read_audio (resampled on the GPU where its rate
	differs) and cut at max_len taps -> (bank (n, Lmax) float32, lengths (n,) int64), CPU tensors, rows zero-padded."""
	from . import audio
	rows = [audio.read_audio(path, sample_rate, mono = True)[0].reshape(-1)[:int(max_len)].cpu() for path in paths]
	if not rows or any(r.numel() < 1 for r in rows):
		raise ValueError('load_rirs: at least one file, each with at least one sample, expected')
	lengths = torch.tensor([r.numel() for r in rows], dtype = torch.int64)
	bank = torch.zeros(len(rows), int(lengths.max()), dtype = torch.float32)
	for i, r in enumerate(rows):
		bank[i, :r.numel()] = r
	return bank, lengths


def batches(batches, waveform = None, spec = None, epoch = 0, samples_per_label = None):
	"""A generator around datasets.gpu_batches' (meta, s, x, xlen, y, ylen): the keys come from meta[i]['example_id'], `waveform` (a
	WaveformAugment) replaces x and xlen, `spec` (a SpecAugment, also set as the model's feature_transform) receives the keys and the epoch.
	Yields the same six-tuple, so train.train_epoch consumes it unchanged.  samples_per_label: when given, an utterance is not sped up below
	samples_per_label * (its longest target) samples -- the waveform length its CTC target needs through the model's total stride."""
	for meta, s, x, xlen, y, ylen in batches:
		keys = torch.tensor([int(m['example_id']) for m in meta], dtype = torch.int64)
		if waveform is not None:
			dev_keys = keys.to(x.device, non_blocking = True)
			min_out_len = None if samples_per_label is None or ylen.numel() == 0 else ylen.to(torch.int64).max(dim = 1).values * int(samples_per_label)
			x, xlen = waveform(x, xlen, dev_keys, epoch = epoch, min_out_len = min_out_len)
		if spec is not None:
			spec.set_keys(keys, epoch)
		yield meta, s, x, xlen, y, ylen
