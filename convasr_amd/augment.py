"""Training-time data augmentation on the GPU: speed, gain and noise on the collated waveforms, SpecAugment on the log-mel features.

The reference trains without augmentation (its frontend's dither is commented out), so what is here is the project's own, defined in
include/convasr_hip.h and unpinned against torchaudio, NeMo or Kaldi.  Every random decision is a pure function of (seed, epoch,
meta['example_id'], purpose, index) through a counter-based generator (Philox4x32-10): it does not depend on the utterance's place in the batch,
on the batch's composition, on the rank or on the steps that ran before, so a resumed or re-sharded run augments every utterance exactly as the
uninterrupted run would.  Augmentation is off unless asked for, and a model in eval() mode never augments.

	wave = augment.WaveformAugment(seed = 1, noise = noise_bank)          # (N, L) float32 device tensor, or None
	spec = augment.SpecAugment(seed = 1)
	model.feature_transform = spec
	batches = augment.batches(datasets.gpu_batches(dataset, sampler, device), waveform = wave, spec = spec, epoch = epoch, samples_per_label = 320)
	train.train_epoch(model, optimizer, batches, ...)
"""
import torch
from torch import nn

from . import _lib, ops


class WaveformAugment:
	"""Speed perturbation, gain and noise mixing of a collated batch, in that order per utterance (include/convasr_hip.h: convasr_augment_params,
	convasr_augment_waveform, convasr_augment_mix): two launches, three with a noise bank, no host synchronisation.  The batch keeps its padded
	length, so bucket-padded batches keep one shape per bucket.

	speed: at most 32 factors in [0.5, 2.0], one drawn per utterance with probability speed_prob; an utterance whose new length would exceed the
	padded length or fall below min_out_len keeps speed 1.0.  gain_db: gain_steps values evenly spaced in dB between the two ends (None: no
	gain), one drawn with probability gain_prob.  Under the frontend's peak normalisation (normalize_signal = True) the gain cancels, so it
	matters only relative to the mixed noise, which is added after it.  noise: a (N, L) float32 device tensor of recordings; with probability
	noise_prob a row, a start offset (the row wraps) and one of snr_steps signal-to-noise ratios evenly spaced in dB over snr_db are drawn."""

	def __init__(self, seed, speed = (0.9, 1.0, 1.1), speed_prob = 1.0, gain_db = (-6.0, 6.0), gain_steps = 64, gain_prob = 1.0, noise = None, snr_db = (5.0, 25.0), snr_steps = 64, noise_prob = 0.5):
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

	def _tables(self, device):
		t = self._on.get(device)
		if t is None:
			t = self._on[device] = tuple(None if h is None else h.to(device) for h in (self.table, self.gain_table, self.snr_table))
		return t

	def params(self, xlen, keys, T, epoch = 0, min_out_len = None):
		"""The drawn integers as device tensors: (dict of (B,) int64 tensors named ops.AUG_FIELDS, xlen_out (B,) float32)."""
		p, xlen_out = self._params(xlen, keys, T, epoch, min_out_len)
		return {name: p[:, i] for i, name in enumerate(ops.AUG_FIELDS)}, xlen_out

	def _params(self, xlen, keys, T, epoch, min_out_len):
		if self.noise is not None and self.noise.device != xlen.device:
			raise _lib.ConvasrHipError(f'WaveformAugment: the noise bank lives on {self.noise.device}, the batch on {xlen.device}')
		return ops.augment_params(xlen, keys, T, self.seed, epoch, self.steps, self.speed_thr, 0 if self.gain_table is None else self.gain_table.numel(), self.gain_thr,
		                          None if self.noise is None else self.noise.shape, 1 if self.snr_table is None else self.snr_table.numel(), self.noise_thr, min_out_len)

	def __call__(self, x, xlen, keys, epoch = 0, min_out_len = None, return_scales = False):
		"""x (B, T) float32 or int16 and xlen (B,) as gpu_batches yields them, keys (B,) int64 -> (x_out (B, T) float32, xlen_out (B,) float32)."""
		_lib.require_cuda(x, xlen, keys)
		p, xlen_out = self._params(xlen, keys, x.shape[-1], epoch, min_out_len)
		table, gain_table, snr_table = self._tables(x.device)
		out, scales = ops.augment_waveform(x, p, table, gain_table, self.noise, snr_table)
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
